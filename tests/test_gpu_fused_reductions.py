"""The first stage of the GMRES reductions folded into the last leg of the node-blocked V-cycle (KNP_FUSED_DOTS, default on; hypre
form, hierarchies of three levels or more), and no Schur diagonal for the kinds that never read it.  Against KNP_FUSED_DOTS=0
(k_multi_dot): the same iteration counts, the same norm fallbacks and exchanges, and the same solution up to summation order -- the
partial sums are partitioned differently, so the Gram-Schmidt coefficients differ in their last bits, and after five solves at
rtol 1e-10 the fields differ by ~1e-11 of their scale.  The fold counter of knp_get_stats shows that the folded leg ran."""
from __future__ import annotations

import numpy as np
import pytest

from parity_utils import ci_config, run_native

pytestmark = pytest.mark.gpu


def _run(monkeypatch, env, coarse=None, **cfg):
    for k in ("KNP_FUSED_DOTS", "KNP_NO_PREPARE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # read at knp_pc_setup / knp_gmres_prepare
    c = ci_config(**cfg)
    if coarse is not None:   # a real multilevel cycle on a small mesh: the folded leg needs three levels or more
        c["solver"]["ksp_settings"]["amg_coarse_size"] = coarse
    s = run_native(c)
    return list(s.iterations), s.backend.x.cpu().numpy(), s.backend.stats()


def _compare(monkeypatch, coarse=None, **cfg):
    its1, x1, st1 = _run(monkeypatch, {}, coarse, **cfg)
    its0, x0, st0 = _run(monkeypatch, {"KNP_FUSED_DOTS": "0"}, coarse, **cfg)
    assert st0["fused_dots"] == 0
    assert its1 == its0
    assert st1["norm_fallbacks"] == st0["norm_fallbacks"]
    assert st1["allreduces"] == st0["allreduces"] and st1["readbacks"] == st0["readbacks"]
    for f in range(4):
        scale = np.max(np.abs(x0[f::4]))
        assert np.max(np.abs(x1[f::4] - x0[f::4])) <= 1e-10 * scale, (f, np.max(np.abs(x1[f::4] - x0[f::4])) / scale)
    return its1, st1


def test_fused_reductions_hypre(monkeypatch):
    """hypre form on a three-level hierarchy: every GMRES iteration of these short cycles takes the folded leg (basis vectors <= 3:
    its G = 3 form), and so do the two preconditioned norms of every solve."""
    its, st = _compare(monkeypatch, coarse=200, N=32, steps=5, rtol=1e-10, kind="square", pc="hypre")
    assert st["blocked"] == 1
    assert st["fused_dots"] >= sum(min(i, 8) for i in its) + len(its), (its, st)


def test_fused_reductions_btcc(monkeypatch):
    """btcc: the cycle ends in the potential hierarchy, so the leg is not folded and the Schur diagonal is still written: the
    switch changes nothing, bit for bit."""
    its1, x1, st1 = _run(monkeypatch, {}, None, N=8, steps=5, rtol=1e-10, kind="cube", pc="btcc")
    its0, x0, st0 = _run(monkeypatch, {"KNP_FUSED_DOTS": "0"}, None, N=8, steps=5, rtol=1e-10, kind="cube", pc="btcc")
    assert st1["fused_dots"] == 0 and its1 == its0 and np.array_equal(x1, x0)


def test_fused_reductions_long_cycles(monkeypatch):
    """A tighter tolerance: cycles long enough for the leg's form with up to 8 basis vectors (G = 8, from the 4th iteration).  (At
    rtol 1e-13 the solve sits on the rounding floor and summation order alone moves the iteration count by one.)"""
    its, st = _compare(monkeypatch, coarse=200, N=32, steps=2, rtol=1e-12, kind="square", pc="hypre")
    assert max(its) >= 7, its
    assert st["fused_dots"] >= sum(min(i, 8) for i in its), (its, st)


def test_hypre_side_stream_norm_takes_the_folded_leg(monkeypatch):
    """The side-stream ||B b|| (knp_gmres_prepare) takes the folded leg like the in-line norm: same iteration counts, and the same
    solution to the tolerance of the comparisons above."""
    a = _run(monkeypatch, {}, 200, N=32, steps=3, rtol=1e-10, kind="square", pc="hypre")
    b = _run(monkeypatch, {"KNP_NO_PREPARE": "1"}, 200, N=32, steps=3, rtol=1e-10, kind="square", pc="hypre")
    assert a[2]["fused_dots"] > 0 and b[2]["fused_dots"] > 0
    assert a[0] == b[0]
    for f in range(4):
        scale = np.max(np.abs(b[1][f::4]))
        assert np.max(np.abs(a[1][f::4] - b[1][f::4])) <= 1e-10 * scale, f
