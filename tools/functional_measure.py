"""Volume functional measurement on one GPU (DESIGN, "Volume functionals"): one knp_functional_eval of phi^2 at degree 2 per side
against knp_l2_norms on the same fields, between the library's own timer events, after a warm-up call of each.

    python tools/functional_measure.py cube 64 [--reps 7] [--out file.json]

Random fields on the CI mesh, no time step.  Prints one JSON line (milliseconds)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "knp-emi-cgx_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=["square", "cube"])
    ap.add_argument("N", type=int)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from cgx_hip.configs import ci_config, make_problem
    from cgx_hip.functionals import VolumeFunctional
    p = make_problem(ci_config(N=a.N, steps=1, kind=a.kind), "ci")
    be = p.create_backend()
    rng = np.random.default_rng(3)
    n = p.local_mesh.coords.shape[0]
    phi = [p.wh[s][p.N_ions] for s in range(2)]
    for f in phi:
        f.x.array.copy_(torch.from_numpy(rng.uniform(-0.1, 0.1, n)).to(f.x.array.device))
    Fi, Fe = VolumeFunctional(p, integrand_i=phi[0] * phi[0]), VolumeFunctional(p, integrand_e=phi[1] * phi[1])
    oi, oe = Fi(), Fe()
    ni, ne = be.l2_norms_sq()
    torch.cuda.synchronize()
    rel = [abs(float(oi.sum()) / ni - 1.0), abs(float(oe.sum()) / ne - 1.0)]
    rows = []
    for _ in range(a.reps):
        be.timer_mark()
        Fi(out=oi)
        be.timer_mark()
        Fe(out=oe)
        be.timer_mark()
        be.l2_norms_sq()
        be.timer_mark()
        rows.append(1e3 * be.timer_read()[:3])
    rows = np.array(rows)
    regs = [sp.spec.code[:, 1].max() + 1 for F in (Fi, Fe) for sp in F.spec.sides]
    res = {"mesh": f"{a.kind}{a.N}", "cells_intra": int((p.cell_side == 0).sum()), "cells_extra": int((p.cell_side == 1).sum()),
           "points_per_cell": int(Fi.spec.q_w.shape[0]), "program_registers": [int(r) for r in regs],
           "lds_bytes_per_block": [int(r) * 128 * 8 + 512 + 512 + 1024 * Fi.n_out for r in regs],      # registers, constants, keys, scan
           "functional_intra_ms": [round(float(v), 4) for v in rows[:, 0]], "functional_extra_ms": [round(float(v), 4) for v in rows[:, 1]],
           "l2_norms_ms": [round(float(v), 4) for v in rows[:, 2]], "rel_difference": rel}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
