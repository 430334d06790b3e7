"""Developer tool (GPU box, repo root): the per-tag membrane-potential reduction next to the flux pass and the stimulus-trace
integral on the facet map of one tissue surrogate, without a solve.  Meant to run under ``rocprofv3 --kernel-trace``:

    python tools/phim_trace_run.py run <dim> <N> <m> [--width W] [--reps R]
        phase 1, one group per membrane tag: 1 + R times membrane_potential() and membrane_fluxes()
        phase 2, all tags merged into one group: 1 + R times membrane_potential(), membrane_fluxes() and membrane_integral()
        (k_diag_facets + the one-wave k_diag_combine<DiagSum<1>> of the stimulus trace)
    python tools/phim_trace_run.py summarise <kernel_trace.csv> [--reps R]
        per phase and diagnostics kernel: calls, average / min / max ns over the R launches after each phase's first one, as CSV

The run also checks the merged result against the per-tag one (min of mins, max of maxes, sum of integrals)."""
import argparse
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "knp-emi-cgx_amd"))

ap = argparse.ArgumentParser()
sub = ap.add_subparsers(dest="cmd", required=True)
r = sub.add_parser("run")
r.add_argument("dim", type=int)
r.add_argument("N", type=int)
r.add_argument("m", type=int)
r.add_argument("--width", type=int, default=None)
r.add_argument("--reps", type=int, default=5)
s = sub.add_parser("summarise")
s.add_argument("trace")
s.add_argument("--reps", type=int, default=5)
a = ap.parse_args()

KERNELS = ("k_diag_phim<", "k_diag_combine_long<DiagPhim>", "k_diag_combine<DiagPhim>", "k_diag_fluxes<", "k_diag_combine<DiagSum<6>", "k_diag_facets<",
           "k_diag_combine<DiagSum<1>")
MERGED_ONLY = ("k_diag_combine_long<DiagPhim>", "k_diag_facets<", "k_diag_combine<DiagSum<1>")

if a.cmd == "summarise":
    rows = []
    with open(a.trace) as f:
        for q in csv.DictReader(f):
            rows.append((int(q["Start_Timestamp"]), int(q["End_Timestamp"]), q["Kernel_Name"]))
    rows.sort()
    w = csv.writer(sys.stdout, quoting=csv.QUOTE_ALL)
    w.writerow(["Phase", "Name", "Calls", "AverageNs", "MinNs", "MaxNs"])
    for k in KERNELS:
        d = [e - b for b, e, n in rows if k in n]
        name = next((n for _, _, n in rows if k in n), k).split("(")[0]
        phases = [("merged", d)] if k in MERGED_ONLY else [("per_tag", d[:1 + a.reps]), ("merged", d[1 + a.reps:])]
        for ph, v in phases:
            v = v[1:]                         # the phase's first launch warms the caches
            if v:
                w.writerow([ph, name, len(v), f"{sum(v) / len(v):.0f}", min(v), max(v)])
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cgx_hip.configs import make_problem, tissue_config  # noqa: E402
from cgx_hip.diagnostics import membrane_program  # noqa: E402

t0 = time.perf_counter()
cfg = tissue_config(a.dim, a.N, a.m, steps=1, rtol=1e-9, pc="btcc" if a.dim == 3 else "hypre", stimulus=True, width=a.width)
p = make_problem(cfg, "ci")
be = p.create_backend()
rng = np.random.default_rng(5)
n = p.local_mesh.coords.shape[0]
for side in range(2):
    for j in range(p.N_ions + 1):
        lo, hi = ((1.0, 150.0) if j < p.N_ions else (-0.1, 0.1))
        p.wh[side][j].x.array.copy_(torch.from_numpy(rng.uniform(lo, hi, n)).to(be.device))
p.phi_m_prev.x.array.copy_(p.wh[0][p.N_ions].x.array - p.wh[1][p.N_ions].x.array)
tags = [int(t) for t in p.gamma_tags]
print(f"tissue{a.dim}d_{a.N}_{a.m}: {len(p.gamma_facet_tags)} membrane facets, {len(tags)} tags, setup {time.perf_counter() - t0:.1f} s", flush=True)

spec = membrane_program(p, p.stim_ufl_expr)
be.set_diag_program(spec)
stim = torch.zeros(1, dtype=torch.float64, device=be.device)
res = {}
for phase, groups in (("per_tag", [[t] for t in tags]), ("merged", [tags])):
    t1 = time.perf_counter()
    be.set_phim_groups(groups)
    be.set_flux_groups(groups)
    if phase == "merged":
        be.set_facet_groups(groups)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for _ in range(1 + a.reps):
        out = be.membrane_potential()
        be.membrane_fluxes()
        if phase == "merged":
            be.membrane_integral(stim)
    torch.cuda.synchronize()
    res[phase] = out.cpu().numpy()
    print(f"{phase}: maps {1e3 * (t2 - t1):.0f} ms, {1 + a.reps} passes {1e3 * (time.perf_counter() - t2):.1f} ms", flush=True)
pt, mg = res["per_tag"], res["merged"]
S = float(np.abs(p.phi_m_prev.numpy()).max()) * float(be.phim_layout().area.sum())
print(f"merged against per tag: min {mg[0, 1] == pt[:, 1].min()}, max {mg[0, 2] == pt[:, 2].max()}, "
      f"|I - sum I_t| / (max|phi| A) = {abs(mg[0, 0] - pt[:, 0].sum()) / S:.2e}", flush=True)
