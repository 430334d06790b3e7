"""Membrane functional measurement on one GPU (DESIGN, "Membrane functionals"): per round, between the library's own timer events and
after a warm-up call of each,
  the stimulus expression through a MembraneFunctional at degree 10 / the same program through knp_diag_membrane_integral,
  the six flux forms written with dot (two functionals of three outputs) / knp_diag_membrane_fluxes.

    python tools/membrane_functional_measure.py cube 64 [--reps 7] [--out file.json]

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
    from cgx_hip import fem
    from cgx_hip.configs import ci_config, make_problem
    from cgx_hip.diagnostics import membrane_program
    from cgx_hip.functionals import MembraneFunctional
    p = make_problem(ci_config(N=a.N, steps=1, kind=a.kind), "ci")
    be = p.create_backend()
    rng = np.random.default_rng(3)
    n = p.local_mesh.coords.shape[0]
    write = lambda fn, v: fn.x.array.copy_(torch.from_numpy(v).to(fn.x.array.device))
    for s in range(2):
        for j in range(p.N_ions):
            write(p.wh[s][j], rng.uniform(1.0, 150.0, n))
        write(p.wh[s][p.N_ions], rng.uniform(-0.1, 0.1, n))
    write(p.phi_m_prev, p.wh[0][p.N_ions].numpy() - p.wh[1][p.N_ions].numpy())
    group = tuple(int(t) for t in p.stimulus_tags)
    S = MembraneFunctional(p, p.stim_ufl_expr, tags=[group], degree=10)
    be.set_diag_program(membrane_program(p, p.stim_ufl_expr))
    be.set_facet_groups([group])
    nrm = fem.FacetNormal(p.mesh)
    flux = []
    for s, r in enumerate("+-"):
        N = [c(r) for c in nrm]
        dphi = fem.dot([g(r) for g in fem.grad(p.wh[s][p.N_ions])], N)
        flux.append(MembraneFunctional(p, [-ion["Di"] * (fem.dot([g(r) for g in fem.grad(p.wh[s][j])], N) + (ion["z"] / p.psi) * p.wh[s][j] * dphi)
                                           for j, ion in enumerate(p.ion_list)]))
    be.set_flux_groups([[int(t)] for t in p.gamma_tags])
    so, ho = S(), torch.zeros(1, dtype=torch.float64, device=be.device)
    be.membrane_integral(ho)
    fo = [F() for F in flux]
    hf = be.membrane_fluxes()
    torch.cuda.synchronize()
    rel = {"stimulus": abs(float(so[0, 0]) / float(ho[0]) - 1.0),
           "fluxes": float(np.max(np.abs(np.stack([f.cpu().numpy() for f in fo], axis=1) / hf.cpu().numpy() - 1.0)))}
    rows = []
    for _ in range(a.reps):
        be.timer_mark()
        S(out=so)
        be.timer_mark()
        be.membrane_integral(ho)
        be.timer_mark()
        for F, o in zip(flux, fo):
            F(out=o)
        be.timer_mark()
        be.membrane_fluxes(out=hf)
        be.timer_mark()
        rows.append(1e3 * be.timer_read()[:4])
    rows = np.array(rows)
    regs = [int(F.spec.spec.code[:, 1].max()) + 1 for F in [S] + flux]
    ms = lambda k: [round(float(v), 4) for v in rows[:, k]]
    res = {"mesh": f"{a.kind}{a.N}", "membrane_facets": int(len(p._fv)), "points_per_facet": int(S.spec.q_w.shape[0]),
           "program_registers": regs, "lds_bytes_per_block": [r * 128 * 8 + 512 + 512 + 1024 * F.n_out for r, F in zip(regs, [S] + flux)],
           "stimulus_functional_ms": ms(0), "stimulus_membrane_integral_ms": ms(1), "flux_functionals_ms": ms(2), "membrane_fluxes_ms": ms(3),
           "rel_difference": rel}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
