"""Enqueue-ahead form of a GMRES cycle start (csrc/knp_krylov.inc, knp_gmres_solve; KNP_GMRES_AHEAD, default on): v_0 and iteration 0 are
launched before the host has read ||B r_0||, and the host waits once, for iteration 0's reduction.  The same kernels run on the same data
in the same stream order, so against KNP_GMRES_AHEAD=0 (the in-order form) EVERYTHING is equal bit for bit: iteration counts, reasons,
residual norms, ||B b||, the solution vector and the unpacked fields -- also when iteration 0 is discarded (converged or out of budget at
the entry, a cancellation flag in one of the two opening norms).  Only the read-back counter differs: one wait less per cycle start.

The switch is read at knp_pc_setup, so both forms run in this process, each on a solver of its own.  Both build their hierarchy on the
host (``amg_setup: host``): the device-side setup sums its sparse products in an order that changes from run to run (two runs of the SAME
form then differ in the 12th digit of ||B b||), and a comparison of bits needs the same preconditioner in both runs."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from parity_utils import ci_config, fp32_stored, make_problem

pytestmark = pytest.mark.gpu

SQUARE = dict(N=32, steps=5, rtol=1e-10, kind="square", pc="hypre")


def _solver(monkeypatch, ahead, ks=None, **cfg):
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    monkeypatch.delenv("KNP_GMRES_AHEAD", raising=False)
    if not ahead:
        monkeypatch.setenv("KNP_GMRES_AHEAD", "0")   # read at knp_pc_setup (first step)
    c = ci_config(**cfg)
    c["solver"]["ksp_settings"].update(dict(ks or {}, amg_setup="host"))
    p = make_problem(c)
    p.solver_config["view_ksp"] = False
    return SolverKNPEMI(p, solver_config=p.solver_config)


def _fields(p):
    """every unpacked field as a host tensor"""
    out = [torch.as_tensor(p.wh[side][j].numpy().copy()) for side in (0, 1) for j in range(4)]
    return out + [torch.as_tensor(p.phi_m_prev.numpy().copy())]


def _run(monkeypatch, ahead, ks=None, **cfg):
    """the run of ``SolverKNPEMI.solve()``, recording every step's (its, reason, rnorm, ||B b||)"""
    s = _solver(monkeypatch, ahead, ks, **cfg)
    s.prepare()
    log = []
    for i in range(1, s.time_steps + 1):
        s.step(i)
        log.append((s.ksp.its, s.ksp.reason, s.ksp.rnorm, s.backend.stats()["bnorm"]))
    s.finish()
    return {"s": s, "log": log, "x": s.backend.x.clone(), "fields": _fields(s.problem), "stats": s.backend.stats()}


def _same_bits(a, b):
    print("ahead", a["log"], a["stats"], "\nin-order", b["log"], b["stats"])
    assert a["log"] == b["log"]        # its, reason, rnorm and ||B b|| of every step, as floats: equal bits (or both NaN-free and equal)
    assert torch.equal(a["x"], b["x"])
    assert len(a["fields"]) == len(b["fields"]) == 9
    for fa, fb in zip(a["fields"], b["fields"]):
        assert torch.equal(fa, fb)
    assert a["stats"]["bnorm"] == b["stats"]["bnorm"]
    assert a["stats"]["norm_fallbacks"] == b["stats"]["norm_fallbacks"]
    assert a["stats"]["allreduces"] == b["stats"]["allreduces"]


CASES = {
    "square32-two-levels": (None, SQUARE),                        # reduction in k_multi_dot
    "square32-three-levels": ({"amg_coarse_size": 200}, SQUARE),    # first reduction stage in the cycle's last leg
    "cube8-btcc": (None, dict(N=8, steps=5, rtol=1e-10, kind="cube", pc="btcc")),   # two hierarchies, the d_t2 swap
}


@pytest.mark.parametrize("name", list(CASES))
def test_same_bits(monkeypatch, name):
    ks, cfg = CASES[name]
    a, b = _run(monkeypatch, True, ks, **cfg), _run(monkeypatch, False, ks, **cfg)
    _same_bits(a, b)
    n_levels = [len(h.levels) for h in a["s"].hierarchies]
    if name == "square32-three-levels":
        assert n_levels[0] >= 3 and a["stats"]["fused_dots"] > 0, (n_levels, a["stats"])
    if name == "cube8-btcc":
        assert len(n_levels) == 2
    # no restart and no discarded iteration in these runs (every solve converges inside its first cycle): one cycle start per solve
    its = [l[0] for l in a["log"]]
    assert all(0 < i < a["s"].gmres_restart for i in its) and all(l[1] > 0 for l in a["log"]), a["log"]
    assert b["stats"]["readbacks"] - a["stats"]["readbacks"] == len(its), (a["stats"], b["stats"])


@pytest.mark.parametrize("prepare", [False, True])
def test_converged_at_entry(monkeypatch, prepare):
    """A second solve of the system just solved: beta <= ttol at the entry, iteration 0 (already run) is discarded, x is not touched."""
    out = []
    for ahead in (True, False):
        s = _solver(monkeypatch, ahead, **dict(SQUARE, steps=2))
        s.prepare()
        for i in (1, 2):
            s.step(i)
        be = s.backend
        x0 = be.x.clone()
        if prepare:
            be.gmres_prepare()
        res = be.gmres(s._rtol, 1e-50, s.ksp_max_it, s.gmres_restart)
        assert torch.equal(be.x, x0)
        out.append((res, be.stats()["bnorm"], be.x.clone()))
    print(out[0][:2], out[1][:2])
    assert out[0][0][0] == 0 and out[0][0][1] > 0      # its = 0, converged
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert torch.equal(out[0][2], out[1][2])


@pytest.mark.parametrize("max_it", [0, 1])
def test_budget(monkeypatch, max_it):
    """max_it = 0: the in-order form runs (nothing may be enqueued ahead of a zero budget); max_it = 1: iteration 0 is the budget."""
    a, b = _run(monkeypatch, True, {"ksp_max_it": max_it}, **SQUARE), _run(monkeypatch, False, {"ksp_max_it": max_it}, **SQUARE)
    _same_bits(a, b)
    assert all(l[0] == max_it for l in a["log"]), a["log"]


def test_restart(monkeypatch):
    """restart = 2 at rtol 1e-12: many cycle starts of every solve run ahead (the later ones have no side cycle to join).  GMRES(2)
    stagnates above this tolerance on the rounding floor, so every solve runs into max_it: 2 500 cycle starts each."""
    ks = {"gmres_restart": 2}
    cfg = dict(SQUARE, rtol=1e-12)
    a, b = _run(monkeypatch, True, ks, **cfg), _run(monkeypatch, False, ks, **cfg)
    _same_bits(a, b)
    its = [l[0] for l in a["log"]]
    assert max(its) > 4, its      # three cycle starts or more in one solve
    assert a["stats"]["readbacks"] < b["stats"]["readbacks"]


# ---- cancellation flags of the two opening norms ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gauge_rhs():
    """r with B r = ns on the 24 x 24 square (2 692 unknowns), B = the oracle's fused, fp32-stored cycle on the hierarchy the solver
    uploads (host setup), as a dense matrix.  Checked here with that cycle alone: z = B r has z.z - s^2/cnt < 1e-10 z.z, a factor 100
    inside the guard GM_CANCEL = 1e-8 of the one-reduction norm."""
    import knpemi_oracle as K
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    c = ci_config(N=24, steps=1, rtol=1e-10, kind="square", pc="hypre")
    c["solver"]["ksp_settings"]["amg_setup"] = "host"
    p = make_problem(c)
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    s.prepare()
    n = s.backend.n_dof_owned
    assert n == 2692
    h = fp32_stored(s.hierarchy)
    cycle = K.pc_amg_vcycle(h.levels, h.coarse_inv, s.amg_pre, s.amg_post, s.amg_cheby_degree, fused=True)
    B = np.empty((n, n))
    e = np.zeros(n)
    for k in range(n):
        e[k] = 1.0
        B[:, k] = cycle(e)
        e[k] = 0.0
    ns = np.zeros(n)
    ns[3::4] = 1.0
    r = np.linalg.solve(B, ns)
    z = cycle(r)
    cnt = n // 4
    zz, sm = float(z @ z), float(z[3::4].sum())
    print(f"gauge right-hand side: |r| = {np.linalg.norm(r):.3e}, z.z = {zz:.6e}, z.z - s^2/cnt = {zz - sm * sm / cnt:.3e}")
    assert zz - sm * sm / cnt < 1e-10 * zz
    return r


@pytest.mark.parametrize("prepare", [False, True])
def test_cancellation(monkeypatch, gauge_rhs, prepare):
    """b = r, x = 0: B b and B r_0 are the gauge vector up to rounding, both one-reduction norms raise their flag.  ``prepare``: ||B b||
    runs on the side stream (its in-line repair overwrites the residual chain once more); without, it is computed in line before the
    first cycle start and only the residual norm's flag reaches the enqueue-ahead form."""
    out = []
    for ahead in (True, False):
        s = _solver(monkeypatch, ahead, N=24, steps=1, rtol=1e-10, kind="square", pc="hypre")
        s.prepare()
        s.step(1)
        be = s.backend
        assert bool(be.stats()["fused"])
        f0 = be.stats()["norm_fallbacks"]
        be.b.copy_(torch.as_tensor(gauge_rhs, device=be.device))
        be.x.zero_()
        if prepare:
            be.gmres_prepare()
        its, rnorm, reason = be.gmres(1e-10, 1e-50, 3, s.gmres_restart)
        st = be.stats()
        out.append((its, reason, st["norm_fallbacks"] - f0, be.x.clone(), rnorm, st["bnorm"]))
    print([o[:3] + o[4:] for o in out])
    assert out[0][2] > 0 and out[1][2] > 0
    assert out[0][2] >= 2      # the residual norm's flag among them
    assert out[0][:3] == out[1][:3]
    assert torch.equal(out[0][3], out[1][3])


# ---- the two-kernel reduction branch (KNP_FIN=0) -----------------------------------------------------------------------------------------
FIN0_CHILD = """
import sys; sys.path[:0] = ['tests', 'oracle', 'knp-emi-cgx_amd']; import conftest, os, json, torch
from parity_utils import ci_config, make_problem
from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
out = []
for ahead in (True, False):
    os.environ.pop('KNP_GMRES_AHEAD', None)
    if not ahead:
        os.environ['KNP_GMRES_AHEAD'] = '0'
    c = ci_config(N=32, steps=3, rtol=1e-10, kind='square', pc='hypre')
    c['solver']['ksp_settings']['amg_setup'] = 'host'
    p = make_problem(c)
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    s.prepare()
    log = []
    for i in (1, 2, 3):
        s.step(i)
        log.append((s.ksp.its, s.ksp.reason, s.ksp.rnorm, s.backend.stats()['bnorm']))
    out.append((log, s.backend.x.clone(), s.backend.stats()))
(la, xa, sa), (lb, xb, sb) = out
print('RESULT' + json.dumps({'same_log': la == lb, 'same_x': bool(torch.equal(xa, xb)), 'its': [l[0] for l in la],
                             'readbacks': [sa['readbacks'], sb['readbacks']], 'fused_dots': [sa['fused_dots'], sb['fused_dots']]}))
"""


def test_two_kernel_reduction_branch():
    """KNP_FIN=0 (k_reduce_partials + k_proj_norm / k_givens, what distributed runs use) on one GPU takes the enqueue-ahead form as well:
    those kernels publish the same mirror slots and sequence word.  The switch is read once per process, so this is a child process
    that runs both forms; same bits, one read-back less per solve."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("KNP_FIN", "KNP_GMRES_AHEAD")}
    out = subprocess.run([sys.executable, "-c", FIN0_CHILD], cwd=root, env=dict(env, KNP_FIN="0"), capture_output=True, text=True, timeout=120)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
    assert out.returncode == 0 and line, f"exit status {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    r = json.loads(line[0][6:])
    print(r)
    assert r["fused_dots"] == [0, 0]      # the other branch ran: no first stage folded into a neighbouring kernel
    assert r["same_log"] and r["same_x"]
    assert r["readbacks"][1] - r["readbacks"][0] == len(r["its"])
