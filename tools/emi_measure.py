"""EMI step measurements on one GPU: ms per step from the library's event timers, PCG iterations per step, and the
achieved bandwidth of the scalar node SpMV against its byte count.

    python tools/emi_measure.py square512 [--steps 20] [--warmup 5] [--pc hypre] [--fp32 0|1] [--out file.json]

HH membrane with the synaptic stimulus, dt 5e-5, C_M 0.02, micrometre mesh, rtol 1e-8 (unpreconditioned norm), one process;
prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "knp-emi-cgx_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pc", default="hypre")
    ap.add_argument("--fp32", type=int, default=0)
    ap.add_argument("--setup", default="host")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from cgx_hip.emi_models import g_syn
    from cgx_hip.emi_problem import ProblemEMI
    from cgx_hip.emi_solver import SolverEMI
    cfg = {"problem_type": "EMI", "dt": 5e-5, "time_steps": a.steps + a.warmup, "C_M": 0.02, "quiet": True,
           "cell_tag_file": a.mesh + ".xdmf", "facet_tag_file": a.mesh + ".xdmf", "mesh_conversion_factor": 1e-6,
           "ics_tags": [1], "ecs_tags": [2], "membrane_tags": [4]}
    p = ProblemEMI(cfg)
    p.add_ionic_model("HH", stim_fun=g_syn)
    p.init_ionic_model()

    class S(SolverEMI):
        ksp_rtol, norm_type, pc_type, amg_fp32, amg_setup, ksp_max_it = 1e-8, "unpreconditioned", a.pc, bool(a.fp32), a.setup, 20000
    s = S(p, use_direct_solver=False)
    s.solve()
    w = a.warmup
    step_ms = 1e3 * (np.array(s.assembly_time) + np.array(s.solve_time))[w:]
    be = s.backend
    # SpMV: 8 B value + 4 B column per stored entry, the row pointer, the gathered x once and y
    nnz = be.n_pairs + 2 * be.n_gamma_pairs
    bytes_spmv = 12.0 * nnz + be.n_nodes * (4.0 + 8.0 + 8.0)
    x = torch.randn(be.n_nodes, dtype=torch.float64, device=be.device)
    y = torch.empty_like(x)
    for _ in range(10):
        be.spmv(x, y)
    reps, times = 50, []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            be.spmv(x, y)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / reps)
    spmv_us = 1e3 * float(np.median(times))
    out = {"mesh": a.mesh, "unknowns": be.n_nodes, "stored_entries": nnz, "pc": a.pc, "amg_fp32": bool(a.fp32), "rtol": 1e-8,
           "steps": a.steps, "warmup": w, "ms_per_step_median": float(np.median(step_ms)), "ms_per_step_min_max": [float(step_ms.min()), float(step_ms.max())],
           "solve_ms_median": 1e3 * float(np.median(s.solve_time[w:])), "rhs_ms_median": 1e3 * float(np.median(s.assembly_time[w:])),
           "iterations": s.iterations[w:], "iterations_mean": float(np.mean(s.iterations[w:])),
           # counted from the code of knp_emi_cg_solve, not measured: SpMV, x/r update, [inner products after the V-cycle], p update;
           # with Dirichlet nodes the AMG application adds two k_emi_mask launches (none in these pure Neumann runs)
           "launches_per_iteration_outside_pc_from_code": 4 if a.pc in ("hypre", "amg") else 3,
           "spmv_us_back_to_back": spmv_us, "spmv_bytes": bytes_spmv, "spmv_TBps": bytes_spmv / (spmv_us * 1e-6) / 1e12,
           "hierarchy": s.hierarchy.describe() if a.pc in ("hypre", "amg") else None}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
