"""Developer tool (GPU box, repo root): the kernels of the activation map (csrc/knp_activation.inc) on the membrane of one tissue
surrogate, without a solve.  Meant to run under ``rocprofv3 --kernel-trace``:

    python tools/activation_trace_run.py run <dim> <N> <m> [--width W] [--reps R]
        arm(), then 1 + R times: a new random phi_m, update(), velocity(), the summary with one group per membrane tag and the
        summary with all tags merged into one group (the maps are set once, before the passes)
    python tools/activation_trace_run.py summarise <kernel_trace.csv>
        per kernel of the activation map: calls, average / min / max ns over the launches after its first one, as CSV

The run also checks the merged summary against the per-tag one (sums of the areas, min of mins, max of maxes)."""
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
a = ap.parse_args()

KERNELS = ("k_activation_arm", "k_activation_step", "k_activation_velocity<", "k_diag_activation<", "k_diag_combine<DiagActivation>",
           "k_diag_combine_long<DiagActivation>")

if a.cmd == "summarise":
    rows = []
    with open(a.trace) as f:
        for q in csv.DictReader(f):
            rows.append((int(q["Start_Timestamp"]), int(q["End_Timestamp"]), q["Kernel_Name"]))
    rows.sort()
    w = csv.writer(sys.stdout, quoting=csv.QUOTE_ALL)
    w.writerow(["Name", "Calls", "AverageNs", "MinNs", "MaxNs", "FirstNs"])
    for k in KERNELS:
        d = [e - b for b, e, n in rows if k in n]
        if not d:
            continue
        name = next(n for _, _, n in rows if k in n).split("(")[0]
        v = d[1:] or d                        # the first launch warms the caches (the arm kernel runs once)
        w.writerow([name, len(v), f"{sum(v) / len(v):.0f}", min(v), max(v), d[0]])
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cgx_hip.activation import ActivationMap  # noqa: E402
from cgx_hip.configs import make_problem, tissue_config  # noqa: E402

t0 = time.perf_counter()
cfg = tissue_config(a.dim, a.N, a.m, steps=1, rtol=1e-9, pc="btcc" if a.dim == 3 else "hypre", stimulus=True, width=a.width)
p = make_problem(cfg, "ci")
be = p.create_backend()
gen = torch.Generator(device=be.device)
gen.manual_seed(5)
n = p.local_mesh.coords.shape[0]
phi = p.phi_m_prev.x.array
phi.copy_(torch.rand(n, generator=gen, device=be.device, dtype=torch.float64) * 0.2 - 0.1)
t1 = time.perf_counter()
amap = ActivationMap(p, 0.0, -0.02)
tags = list(amap.tags)
print(f"tissue{a.dim}d_{a.N}_{a.m}: {len(amap.facets)} membrane facets, {len(amap.vertices)} membrane vertices, {len(tags)} tags, "
      f"setup {t1 - t0:.1f} s, map {time.perf_counter() - t1:.2f} s", flush=True)
per_tag = [(t,) for t in tags]
t2 = time.perf_counter()
for k in range(1 + a.reps):
    phi.copy_(torch.rand(n, generator=gen, device=be.device, dtype=torch.float64) * 0.2 - 0.1)
    p.t.value = float(p.t.value) + 2.5e-5
    amap.update()
    vel = amap.velocity()
    rows, _ = amap.summary(per_tag)
    one, _ = amap.summary([tags])             # replaces the map: a synchronous upload per call, outside the kernels' times
torch.cuda.synchronize()
print(f"{1 + a.reps} passes {1e3 * (time.perf_counter() - t2):.1f} ms (with the map uploads)", flush=True)
rows, one = rows.cpu().numpy(), one.cpu().numpy()[0]
res = amap.result()
print(f"fired {int((res['count'] > 0).sum())} of {len(amap.vertices)} vertices, valid facets {int((~torch.isnan(vel[:, 0])).sum())}", flush=True)
A = float(amap.area.sum())
print(f"merged against per tag: min {one[2] == rows[:, 2].min()}, max {one[3] == rows[:, 3].max()}, "
      f"|sum - sum_t| / A = {max(abs(one[c] - rows[:, c].sum()) for c in (0, 4)) / A:.2e}", flush=True)
