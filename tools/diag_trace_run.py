"""Developer tool (GPU box, repo root): a short run of one tissue surrogate with the device-side traces on -- the stimulus
current (save_dat) and, with --fluxes, the membrane ion fluxes (save_fluxes) -- meant to run under
``rocprofv3 --kernel-trace --stats`` so that k_diag_facets, k_diag_fluxes and k_diag_combine show up side by side.
    python tools/diag_trace_run.py <dim> <N> <m> [--width W] [--steps K] [--fluxes] [--out DIR]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "knp-emi-cgx_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("dim", type=int)
ap.add_argument("N", type=int)
ap.add_argument("m", type=int)
ap.add_argument("--width", type=int, default=None)
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--fluxes", action="store_true")
ap.add_argument("--all-tags", type=int, default=0, metavar="R", help="after the run, R passes of membrane_fluxes() over every membrane tag")
ap.add_argument("--out", type=str, default="bench_outputs/diag_trace")
ap.add_argument("--host-amg", action="store_true", help="build the hierarchy on the host: keeps torch's kernels out of a trace")
a = ap.parse_args()

from cgx_hip.configs import make_problem, tissue_config  # noqa: E402
from cgx_hip.solver import SolverKNPEMI  # noqa: E402

cfg = tissue_config(a.dim, a.N, a.m, steps=a.steps, rtol=1e-9, pc="btcc" if a.dim == 3 else "hypre", stimulus=True, width=a.width)
cfg["output_dir"] = a.out.rstrip("/") + "/"
cfg["solver"]["output"].update({"save_dat": True, "save_fluxes": bool(a.fluxes)})
if a.host_amg:
    cfg["solver"]["ksp_settings"]["amg_setup"] = "host"
t0 = time.perf_counter()
p = make_problem(cfg, "ci")
p.solver_config["view_ksp"] = False
s = SolverKNPEMI(p, solver_config=p.solver_config)
s.solve()
for r in range(a.all_tags):
    t1 = time.perf_counter()
    out = p.membrane_fluxes()
    print(f"membrane_fluxes() over {len(out['tag'])} tags: {1e3 * (time.perf_counter() - t1):.1f} ms"
          + (" (with the record build)" if r == 0 else ""), flush=True)
n_sel = int((p.gamma_facet_tags == p.membrane_data_tag).sum())
print(f"tissue{a.dim}d_{a.N}_{a.m}: {len(p.gamma_facet_tags)} membrane facets, {n_sel} on the membrane-data tag, "
      f"{a.steps} steps, its {s.iterations}, wall {time.perf_counter() - t0:.1f} s", flush=True)
