"""Fused tail of a GMRES solve and what hangs on it (csrc/knp_krylov.inc, knp_gmres_solve):
  * KNP_FUSED_TAIL (default on): the update x += V y of the cycle after which the solve returns also unpacks x into the registered fields
    and writes the node-indexed concentration copy (k_lincomb_unpack instead of k_lincomb_solve + k_unpack + k_nodal_conc); the next
    matrix assembly skips k_nodal_conc when cgx_hip.backend promises that torch did not write the fields in between;
  * KNP_UPDATE_EARLY (default on): k_update_scale returns at once on the converging iteration.
The same operations run in the same order on the same data, so against the same build with the switches off EVERYTHING is equal bit for
bit.  Both switches are read at knp_pc_setup, so all forms run in this process, each on a solver of its own; the hierarchies are built on
the host (the device-side setup is not reproducible to the last bit from run to run, see test_gpu_gmres_ahead.py)."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from parity_utils import ci_config, make_problem
from cgx_hip import _lib as L

pytestmark = pytest.mark.gpu

SQUARE8 = dict(N=8, steps=5, rtol=1e-10, kind="square", pc="hypre")
SQUARE32 = dict(N=32, steps=5, rtol=1e-10, kind="square", pc="hypre")
CUBE4 = dict(N=4, steps=5, rtol=1e-10, kind="cube", pc="btcc")
# (the cube at rtol 1e-10 takes 8 to 12 iterations: long cycles, which keep the separate kernels, next to a fused one in the same run)
CASES = {"square8": SQUARE8, "square32": SQUARE32, "cube4-btcc": CUBE4, "cube4-btcc-1e-6": dict(CUBE4, rtol=1e-6)}
SWITCHES = ("KNP_FUSED_TAIL", "KNP_UPDATE_EARLY")


class _NoTailCalls:
    """the library as a caller sees it that never calls knp_set_unpack_target or knp_fields_unchanged"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in ("knp_set_unpack_target", "knp_fields_unchanged"):
            return lambda *a: 0
        return getattr(self._lib, name)


def _solver(tail, early, ks=None, direct=False, **cfg):
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    for k, on in zip(SWITCHES, (tail, early)):
        os.environ.pop(k, None)
        if not on:
            os.environ[k] = "0"      # read at knp_pc_setup (first step)
    c = ci_config(direct=direct, **cfg)
    c["solver"]["ksp_settings"].update(dict(ks or {}, amg_setup="host"))
    p = make_problem(c)
    p.solver_config["view_ksp"] = False
    return SolverKNPEMI(p, solver_config=p.solver_config)


def _state(p):
    """every unpacked field, phi_m_prev and the gates as host tensors"""
    out = [torch.as_tensor(p.wh[side][j].numpy().copy()) for side in (0, 1) for j in range(4)]
    out.append(torch.as_tensor(p.phi_m_prev.numpy().copy()))
    return out + [torch.as_tensor(getattr(p, g).numpy().copy()) for g in ("n", "m", "h")]


def _matrix_values(be):
    va = np.empty(be.nnz, dtype=np.float64)
    be.check(be.lib.knp_get_csr_values(be.ctx, va.ctypes.data_as(L.f64p)))
    return va


def _run(tail, early, ks=None, direct=False, between=None, abi_only=False, **cfg):
    """``SolverKNPEMI.solve()`` step by step.  Recorded per step: (its, reason, rnorm, ||B b||), x, the state, A's values and b (A and b of
    step i + 1 are assembled from the fields step i unpacked).  At the end one more matrix assembly, then the node-indexed concentration
    copy and A once more: what the NEXT step would start from.  ``between(i, solver)`` runs after step i."""
    real_load = L.load
    try:
        if abi_only:      # the backend is created inside prepare(): it only ever sees the library without the two entry points
            L.load = lambda: _NoTailCalls(real_load())
        s = _solver(tail, early, ks, direct, **cfg)
        s.prepare()
        L.load = real_load
        be = s.backend
        assert isinstance(be.lib, _NoTailCalls) == abi_only
        log, xs, states, mats, rhs = [], [], [], [], []
        for i in range(1, s.time_steps + 1):
            s.step(i)
            log.append((s.ksp.its, s.ksp.reason, s.ksp.rnorm, be.stats()["bnorm"]))
            xs.append(be.x.clone())
            states.append(_state(s.problem))
            mats.append(_matrix_values(be))
            rhs.append(be.b.clone())
            if between is not None:
                between(i, s)
        s.finish()
        stats = be.stats()      # before the extra assembly below, which may skip once more
        be.assemble_matrix()
        return {"s": s, "log": log, "x": xs, "state": states, "A": mats, "b": rhs, "stats": stats, "knod": be.nodal_conc(), "A_next": _matrix_values(be)}
    finally:
        L.load = real_load
        for k in SWITCHES:
            os.environ.pop(k, None)


def _same_bits(a, b):
    print("a:", a["log"], {k: a["stats"][k] for k in ("fused_tails", "knod_skips")}, "\nb:", b["log"], {k: b["stats"][k] for k in ("fused_tails", "knod_skips")})
    assert a["log"] == b["log"]        # its, reason, rnorm and ||B b|| of every step
    assert len(a["x"]) == len(b["x"])
    for i in range(len(a["x"])):
        assert torch.equal(a["x"][i], b["x"][i]), f"x of step {i + 1}"
        assert len(a["state"][i]) == len(b["state"][i]) == 12
        for k, (fa, fb) in enumerate(zip(a["state"][i], b["state"][i])):
            assert torch.equal(fa, fb), f"field {k} after step {i + 1}"
        assert np.array_equal(a["A"][i], b["A"][i]), f"A of step {i + 1}"
        assert torch.equal(a["b"][i], b["b"][i]), f"b of step {i + 1}"
    assert np.array_equal(a["knod"], b["knod"])
    assert np.array_equal(a["A_next"], b["A_next"])


def _knod_from_fields(r):
    """what k_nodal_conc writes from the final fields: {k0, k1, k2, 0} of the node's own side at its vertex"""
    s = r["s"]
    be, st = s.backend, r["state"][-1]
    ref = np.zeros((be.n_nodes, 4))
    for side, nodes in ((0, be.node_i), (1, be.node_e)):
        v = np.nonzero(nodes >= 0)[0]
        for j in range(3):
            ref[nodes[v], j] = st[4 * side + j].numpy()[v]
    return ref


_cache = {}


def _cached(name, tail, early):
    key = (name, tail, early)
    if key not in _cache:
        _cache[key] = _run(tail, early, **CASES[name])
    return _cache[key]


# ---- 1: five steps, all four switch settings -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("tail,early", [(True, True), (True, False), (False, True)])
def test_five_steps_same_bits(name, tail, early):
    a, b = _cached(name, tail, early), _cached(name, False, False)
    _same_bits(a, b)
    assert b["stats"]["fused_tails"] == 0 and b["stats"]["knod_skips"] == 0
    assert (a["stats"]["fused_tails"] > 0) == tail
    assert np.array_equal(a["knod"], _knod_from_fields(a))      # and the copy is what k_nodal_conc makes of the final fields


# ---- 2, 3: the counters ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_counters(name):
    a = _cached(name, True, True)
    its = [l[0] for l in a["log"]]
    assert all(l[1] > 0 for l in a["log"]), a["log"]
    short = [0 < i <= 8 for i in its]      # restart 30: such a solve ends in one short cycle, whose update is the fused one
    assert any(short), its
    if name != "cube4-btcc":
        assert all(short), its
    assert a["stats"]["fused_tails"] == sum(short)
    # nothing touches the fields between the steps: the assembly of step i + 1 skips iff the solve of step i ended in a fused tail
    assert a["stats"]["knod_skips"] == sum(short[:-1])
    assert a["s"].backend.stats()["knod_skips"] == sum(short)      # ... and so did the extra assembly of _run
    tm = a["s"].backend.traffic_model()["assembly_matrix"]
    tm0 = _cached(name, False, False)["s"].backend.traffic_model()["assembly_matrix"]
    assert tm0 - tm == 56.0 * a["s"].backend.n_nodes      # the copy pass leaves the byte model exactly where it is skipped


# ---- 4: several cycles per solve -----------------------------------------------------------------------------------------------------------
def test_restart_2_fuses_only_the_last_cycle():
    ks = {"gmres_restart": 2, "ksp_max_it": 40}      # (GMRES(2) may stagnate: a solve that runs out of iterations ends in a fused cycle too)
    cfg = dict(SQUARE32)
    a, b = _run(True, True, ks, **cfg), _run(False, False, ks, **cfg)
    _same_bits(a, b)
    its = [l[0] for l in a["log"]]
    assert max(its) > 2, its      # a second cycle in at least one solve
    assert 1 <= a["stats"]["fused_tails"] <= len(its)      # at most one fused update per solve, whatever its number of cycles


# ---- 5: out of iterations ----------------------------------------------------------------------------------------------------------------
def test_max_it_1_still_fuses():
    ks = {"ksp_max_it": 1}
    a, b = _run(True, True, ks, **SQUARE32), _run(False, False, ks, **SQUARE32)
    _same_bits(a, b)
    assert all(l[0] == 1 and l[1] < 0 for l in a["log"]), a["log"]
    assert a["stats"]["fused_tails"] == len(a["log"])


# ---- 6: converged at entry ---------------------------------------------------------------------------------------------------------------
def test_converged_at_entry_unpacks_with_the_plain_kernel():
    s = _solver(True, True, **dict(SQUARE32, steps=2))
    s.prepare()
    for i in (1, 2):
        s.step(i)
    be, p = s.backend, s.problem
    want = _state(p)[:9]
    tails = be.stats()["fused_tails"]
    its, _, reason = be.gmres(s._rtol, 1e-50, s.ksp_max_it, s.gmres_restart)
    assert its == 0 and reason > 0
    for side in (0, 1):      # wipe the fields behind the library's back (raw fill: no version change a backend could notice)
        for j in range(4):
            p.wh[side][j].x.array.data.zero_()
    p.phi_m_prev.x.array.data.zero_()
    be.unpack()
    assert be.stats()["fused_tails"] == tails      # no update kernel ran at all
    for fa, fb in zip(_state(p)[:9], want):
        assert torch.equal(fa, fb)


# ---- 7: emulated direct solve: project_nullspace(x) follows the solve ----------------------------------------------------------------------
def test_direct_solver_projection_invalidates_the_tail():
    a, b = _run(True, True, direct=True, **dict(SQUARE8, steps=3)), _run(False, False, direct=True, **dict(SQUARE8, steps=3))
    _same_bits(a, b)
    assert a["stats"]["knod_skips"] == 0      # x changed after the tail: its concentration copy is never trusted
    phi = torch.cat([a["state"][-1][3][torch.as_tensor(a["s"].backend.node_i >= 0)], a["state"][-1][7][torch.as_tensor(a["s"].backend.node_e >= 0)]])
    assert abs(float(phi.mean())) <= 1e-12 * float(phi.abs().max())      # the fields are those of the PROJECTED x


# ---- 8, 9: torch writes a field / rebinds phi_m_prev between two steps ---------------------------------------------------------------------
def _scale_a_concentration(i, s):
    if i == 2:
        s.problem.wh[0][0].x.array[...] *= 1.01


_kept = []


def _rebind_phi_m_prev(i, s):
    if i == 2:
        _kept.append(s.problem.phi_m_prev)      # the library keeps the old pointer (struct cached by the backend): keep the memory alive
        s.problem.set_initial_conditions()
        assert s.problem.phi_m_prev is not _kept[-1]


@pytest.mark.parametrize("between", [_scale_a_concentration, _rebind_phi_m_prev])
def test_a_write_between_steps_runs_the_copy_pass(between):
    cfg = dict(SQUARE32, steps=3)
    a, b = _run(True, True, between=between, **cfg), _run(False, False, between=between, **cfg)
    _same_bits(a, b)
    assert a["stats"]["fused_tails"] == 3
    assert a["stats"]["knod_skips"] == 1      # the assembly of step 2 skipped, that of step 3 (after the write) did not


# ---- 10: the flexible driver ---------------------------------------------------------------------------------------------------------------
def test_fgmres_has_no_fused_tail():
    ks = {"ksp_type": "fgmres", "norm_type": "unpreconditioned"}
    a, b = _run(True, True, ks, **SQUARE32), _run(False, False, ks, **SQUARE32)
    _same_bits(a, b)
    assert a["stats"]["fused_tails"] == 0 and a["stats"]["knod_skips"] == 0


# ---- 11: a caller that never registers a target --------------------------------------------------------------------------------------------
def test_pure_abi_caller_keeps_the_separate_kernels():
    a, b = _run(True, True, abi_only=True, **SQUARE32), _cached("square32", False, False)
    _same_bits(a, b)
    assert a["stats"]["fused_tails"] == 0 and a["stats"]["knod_skips"] == 0
