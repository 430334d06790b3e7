"""Field sampling measurements on one GPU ("Fields on grids and slices"): the time to build a sampling plan, the time
of one record, and the step time of the run the grid would be recorded in.

    python tools/sample_measure.py cube 64 256 [--steps 6] [--out file.json]       256 x 256 mid-plane slice of cube 64^3
    python tools/sample_measure.py square 512 512                                   512 x 512 grid over the 512^2 square

The CI physics runs `--steps` steps without `sample_grids`; the step time is the mean of assembly + solve of the steps after the first,
from the solver's own event timers.  Then, on that problem: the plan build (host wall clock around a synchronous call, split into the
NumPy binning and the rest), the first record and the mean of 7 x 50 records of the four merged fields (device events).  Prints one
JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "knp-emi-cgx_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=["square", "cube"])
    ap.add_argument("N", type=int)
    ap.add_argument("G", type=int, help="grid points per axis")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    from cgx_hip.configs import ci_config, make_problem
    from cgx_hip.sampling import GridSampler, bin_points, merged_functions
    p = make_problem(ci_config(N=a.N, steps=a.steps, kind=a.kind), "ci")
    p.solver_config["view_ksp"] = False
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    s.solve()
    step_ms = 1e3 * (np.array(s.assembly_time) + np.array(s.solve_time))[1:]
    lm = p.local_mesh
    lo, hi = lm.coords.min(axis=0), lm.coords.max(axis=0)
    if a.kind == "cube":
        origin = np.array([lo[0], lo[1], 0.5 * (lo[2] + hi[2])])
        axes = [[hi[0] - lo[0], 0.0, 0.0], [0.0, hi[1] - lo[1], 0.0]]
    else:
        origin, axes = lo, [[hi[0] - lo[0], 0.0], [0.0, hi[1] - lo[1]]]
    builds = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gs = GridSampler(p, origin, axes, (a.G, a.G))
        builds.append(time.perf_counter() - t0)
        gs.close()
    t0 = time.perf_counter()
    bin_points(gs.points)
    t_bin = time.perf_counter() - t0
    gs = GridSampler(p, origin, axes, (a.G, a.G))
    _, f_i, f_e = merged_functions(p)
    out = torch.empty((4, a.G, a.G), dtype=torch.float64, device=s.backend.device)

    def timed(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            gs(f_i, f_e, out=out)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    first = timed(1)
    for _ in range(10):
        gs(f_i, f_e, out=out)
    rec = [timed(50) for _ in range(7)]
    res = {"mesh": f"{a.kind}{a.N}", "cells": int(lm.cells.shape[0]), "grid": [a.G, a.G], "found": int(gs.found.sum()),
           "bins": [int(v) for v in gs.bins["shape"]], "plan_build_s": [round(b, 5) for b in builds], "of_which_binning_s": round(t_bin, 5),
           "first_record_ms": round(first, 4), "record_ms_mean": round(float(np.mean(rec)), 5), "record_ms_min_max": [round(min(rec), 5), round(max(rec), 5)],
           "step_ms_mean": round(float(step_ms.mean()), 4), "step_ms": [round(float(v), 4) for v in step_ms], "iterations": [int(i) for i in s.iterations],
           "record_bytes": 4 * a.G * a.G * 8}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
