"""Matrix assembly ahead of the caller (KNP_ASM_AHEAD, default on; csrc/knp_kernels.hip: speculate_asm, adopt_ahead, drop_ahead).

Once a matrix assembly has skipped its copy pass (the caller leaves the fields alone between unpack and assembly: the context is
ARMED), a knp_gmres_solve that ends in the fused tail enqueues the next step's matrix assembly itself, behind k_lincomb_unpack on the
assembly stream, into a second buffer; the caller's next knp_assemble_matrix(_async) adopts it (buffer swap, nothing launched) if the
promise and the recorded pointers hold, and discards it otherwise.

The same kernels run on the same inputs in the same stream order; only the buffer and the enqueue time differ.  So every comparison
below is against the same build with KNP_ASM_AHEAD=0 in the same process and is exact, bit for bit, with no tolerance.  The switch is
read at knp_pc_setup (first step), so each run has a solver of its own; the hierarchies are built on the host (the device-side setup
is not reproducible to the last bit from run to run, see test_gpu_gmres_ahead.py).

A's values are read AFTER each step: that is the matrix step i solved with, read while the speculative assembly of step i + 1 is
pending or done in the other buffer (which is NaN wherever that assembly does not write)."""
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
CASES = {"square8": SQUARE8, "square32": SQUARE32, "cube4-btcc": CUBE4}
SWITCH = "KNP_ASM_AHEAD"
COUNTERS = ("fused_tails", "knod_skips", "asm_ahead", "asm_ahead_discarded")


def _solver(ahead, ks=None, direct=False, env=None, extra=None, **cfg):
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    os.environ.pop(SWITCH, None)
    if not ahead:
        os.environ[SWITCH] = "0"      # read at knp_pc_setup (first step)
    for k, v in (env or {}).items():
        os.environ[k] = v
    c = ci_config(direct=direct, **cfg)
    c.update(extra or {})
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


def _run(ahead, ks=None, direct=False, between=None, env=None, extra=None, after_prepare=None, **cfg):
    """``SolverKNPEMI.solve()`` step by step.  Recorded per step: (its, reason, rnorm, ||B b||), x, the state, A's values and b, and
    the counters.  ``between(i, solver, rec)`` runs after step i.  At the end one more matrix assembly (which adopts what the last
    solve enqueued), then the node-indexed concentration copy and A once more: what the NEXT step would start from."""
    try:
        s = _solver(ahead, ks, direct, env, extra, **cfg)
        s.prepare()
        be = s.backend
        if after_prepare is not None:
            after_prepare(s)
        rec = {"s": s, "log": [], "x": [], "state": [], "A": [], "b": [], "counts": [], "extra": []}
        for i in range(1, s.time_steps + 1):
            s.step(i)
            rec["log"].append((s.ksp.its, s.ksp.reason, s.ksp.rnorm, be.stats()["bnorm"]))
            rec["x"].append(be.x.clone())
            rec["state"].append(_state(s.problem))
            rec["A"].append(_matrix_values(be))
            rec["b"].append(be.b.clone())
            rec["counts"].append({k: be.stats()[k] for k in COUNTERS})
            if between is not None:
                between(i, s, rec)
        s.finish()
        rec["stats"] = be.stats()      # before the extra assembly below, which may adopt once more
        be.assemble_matrix()
        rec.update(knod=be.nodal_conc(), A_next=_matrix_values(be), stats_next=be.stats())
        return rec
    finally:
        os.environ.pop(SWITCH, None)
        for k in (env or {}):
            os.environ.pop(k, None)


def _same_bits(a, b):
    print("a:", a["log"], a["counts"], "\nb:", b["log"], b["counts"])
    assert a["log"] == b["log"]        # its, reason, rnorm and ||B b|| of every step
    assert len(a["x"]) == len(b["x"])
    for i in range(len(a["x"])):
        assert torch.equal(a["x"][i], b["x"][i]), f"x of step {i + 1}"
        assert len(a["state"][i]) == len(b["state"][i]) == 12
        for k, (fa, fb) in enumerate(zip(a["state"][i], b["state"][i])):
            assert torch.equal(fa, fb), f"field {k} after step {i + 1}"
        assert np.isfinite(a["A"][i]).all(), f"A of step {i + 1} holds an entry no assembly wrote"
        assert np.array_equal(a["A"][i], b["A"][i]), f"A of step {i + 1}"
        assert torch.equal(a["b"][i], b["b"][i]), f"b of step {i + 1}"
    assert len(a["extra"]) == len(b["extra"])
    for ea, eb in zip(a["extra"], b["extra"]):
        assert np.array_equal(ea, eb)
    assert np.array_equal(a["knod"], b["knod"])
    assert np.isfinite(a["A_next"]).all()
    assert np.array_equal(a["A_next"], b["A_next"])
    assert [c["knod_skips"] for c in a["counts"]] == [c["knod_skips"] for c in b["counts"]]
    assert a["stats_next"]["knod_skips"] == b["stats_next"]["knod_skips"]
    assert b["stats_next"]["asm_ahead"] == 0 and b["stats_next"]["asm_ahead_discarded"] == 0      # switch off: never


def _expected(short, no_promise=()):
    """(adopted, discarded, pending after the last step) from the contract alone.  ``short[i]``: the solve of step i + 1 ended in the
    fused tail (one cycle of at most 8 iterations); ``no_promise``: steps (from 0) whose assembly follows a torch write.  The
    assembly of the very first step never carries the promise (nothing was unpacked before it)."""
    armed = pending = knod = False
    adopted = discarded = 0
    for i, sh in enumerate(short):
        promise = i >= 1 and i not in no_promise
        if pending:
            skip = promise
            if promise:
                adopted += 1
            else:
                discarded += 1
                armed = False
        else:
            skip = promise and knod
        armed = armed or skip
        knod = sh
        pending = armed and knod
    return adopted, discarded, pending


def _short(r):
    return [0 < l[0] <= 8 for l in r["log"]]


_cache = {}


def _cached(name, ahead):
    key = (name, ahead)
    if key not in _cache:
        _cache[key] = _run(ahead, **CASES[name])
    return _cache[key]


# ---- 1, 2, 8: five steps bit for bit, the counters, and the adoption after the last step -----------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_steps_same_bits_and_counters(name):
    a, b = _cached(name, True), _cached(name, False)
    _same_bits(a, b)
    short = _short(a)
    assert any(short), a["log"]
    adopted, discarded, pending = _expected(short)
    if name != "cube4-btcc":      # every solve short: armed by the assembly of step 2, so steps 3 .. N adopt
        assert all(short) and adopted == len(short) - 2 and pending
    assert a["stats"]["asm_ahead"] == adopted
    assert a["stats"]["asm_ahead_discarded"] == 0 == discarded
    assert a["stats"]["knod_skips"] == b["stats"]["knod_skips"] == sum(short[:-1])
    # after the last step: the extra assembly adopts what the last solve enqueued (knod and A_next compared in _same_bits)
    assert a["stats_next"]["asm_ahead"] == adopted + int(pending)
    assert a["stats_next"]["asm_ahead_discarded"] == 0


# ---- 3: one torch write / one rebinding between two steps --------------------------------------------------------------------------------------
def _scale_a_concentration(i, s, rec):
    if i == 2:
        s.problem.wh[0][0].x.array[...] *= 1.01


_kept = []


def _rebind_phi_m_prev(i, s, rec):
    if i == 2:
        _kept.append(s.problem.phi_m_prev)      # the library keeps the old pointer (struct cached by the backend): keep the memory alive
        s.problem.set_initial_conditions()
        assert s.problem.phi_m_prev is not _kept[-1]


@pytest.mark.parametrize("between", [_scale_a_concentration, _rebind_phi_m_prev])
def test_a_write_between_steps_discards_once_and_rearms(between):
    a, b = _run(True, between=between, **SQUARE32), _run(False, between=between, **SQUARE32)
    _same_bits(a, b)
    assert all(_short(a)), a["log"]
    d = [c["asm_ahead_discarded"] for c in a["counts"]]
    n = [c["asm_ahead"] for c in a["counts"]]
    assert d == [0, 0, 1, 1, 1]      # exactly one discard, by the assembly of step 3
    # step 3 ran the copy pass (disarmed), step 4 skipped it again (armed), the solve of step 4 ran ahead, step 5 adopted
    assert n == [0, 0, 0, 0, 1]
    assert (n[-1], d[-1], True) == _expected(_short(a), no_promise=(2,))
    assert a["stats_next"]["asm_ahead"] == 2 and a["stats_next"]["asm_ahead_discarded"] == 1


# ---- 4: a write after every step -------------------------------------------------------------------------------------------------------------
def _scale_after_every_step(i, s, rec):
    if i >= 2:      # (step 2 is the first whose assembly can skip and arm: a write after step 1 already would never arm at all)
        s.problem.wh[0][0].x.array[...] *= 1.001


def test_a_write_after_every_step_costs_one_discard():
    a, b = _run(True, between=_scale_after_every_step, **SQUARE32), _run(False, between=_scale_after_every_step, **SQUARE32)
    _same_bits(a, b)
    assert [c["asm_ahead_discarded"] for c in a["counts"]] == [0, 0, 1, 1, 1]      # one in the whole run, none after it
    assert a["stats_next"]["asm_ahead_discarded"] == 1
    assert a["stats_next"]["asm_ahead"] == 0


# ---- 5: what drops a pending speculation ----------------------------------------------------------------------------------------------------
def test_direct_solver_projection_never_speculates():
    cfg = dict(SQUARE8, steps=3)
    a, b = _run(True, direct=True, **cfg), _run(False, direct=True, **cfg)
    _same_bits(a, b)
    # knp_project_nullspace(x) follows every solve: no assembly ever skips, the context is never armed
    assert a["stats_next"]["asm_ahead"] == 0 and a["stats_next"]["asm_ahead_discarded"] == 0 and a["stats_next"]["knod_skips"] == 0


def test_project_nullspace_drops_a_pending_speculation():
    def between(i, s, rec):
        if i == 3:
            s.backend.project_nullspace(s.backend.x)
            s.backend.unpack()
    a, b = _run(True, between=between, **SQUARE32), _run(False, between=between, **SQUARE32)
    _same_bits(a, b)
    assert [c["asm_ahead"] for c in a["counts"]] == [0, 0, 1, 1, 1]      # step 3 adopted; the one pending after step 3 was dropped
    assert [c["asm_ahead_discarded"] for c in a["counts"]][-1] == 1
    assert a["stats_next"]["asm_ahead_discarded"] == 1


def _halve_dt(i, s, rec):
    if i == 2:
        s.problem.dt.value = 0.5 * float(s.problem.dt.value)
        s.backend.set_params()
        rec["dropped"] = s.backend.stats()["asm_ahead_discarded"]


def test_set_params_with_another_dt_drops_the_speculation():
    a, b = _run(True, between=_halve_dt, **SQUARE32), _run(False, between=_halve_dt, **SQUARE32)
    _same_bits(a, b)
    assert a["dropped"] == 1 and b["dropped"] == 0      # dropped inside knp_set_params, before any assembly could adopt it
    assert a["counts"][2]["asm_ahead"] == 0             # step 3 assembled every block itself, with the new dt
    assert a["stats_next"]["asm_ahead_discarded"] == 1


def test_reassemble_P_same_bits():
    ks = {"reassemble_P": True}      # every step from the second on
    a, b = _run(True, ks, **SQUARE32), _run(False, ks, **SQUARE32)
    _same_bits(a, b)
    # in SolverKNPEMI.step the preconditioner is re-assembled AFTER the step's matrix assembly, which has adopted by then: nothing is
    # pending when knp_assemble_precond runs, nothing is dropped
    assert a["stats_next"]["asm_ahead_discarded"] == 0


def _reassemble_now(i, s, rec):
    if i == 3:
        s.reassemble_preconditioner()      # knp_assemble_precond rewrites d_knod from its own fields; knp_pc_setup follows
        rec["dropped"] = s.backend.stats()["asm_ahead_discarded"]


def test_assemble_precond_drops_a_pending_speculation():
    a, b = _run(True, between=_reassemble_now, **SQUARE32), _run(False, between=_reassemble_now, **SQUARE32)
    _same_bits(a, b)
    assert a["dropped"] == 1 and b["dropped"] == 0
    assert [c["asm_ahead"] for c in a["counts"]] == [0, 0, 1, 1, 1]      # never adopted: step 4 assembled itself
    assert a["stats_next"]["asm_ahead_discarded"] == 1


# ---- 6: forms that never speculate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["asm_full", "fgmres", "dirichlet", "class_timing"])
def test_no_speculation(what):
    kw = {"asm_full": dict(env={"KNP_ASM_FULL": "1"}),
          "fgmres": dict(ks={"ksp_type": "fgmres", "norm_type": "unpreconditioned"}),
          "dirichlet": dict(extra={"dirichlet_bcs": True}),
          "class_timing": dict(after_prepare=lambda s: s.backend.profile_enable(0x1f))}[what]
    cfg = dict(SQUARE32, steps=4)
    a, b = _run(True, **kw, **cfg), _run(False, **kw, **cfg)
    _same_bits(a, b)
    assert all(l[1] > 0 for l in a["log"]), a["log"]
    assert a["stats_next"]["asm_ahead"] == 0 and a["stats_next"]["asm_ahead_discarded"] == 0


# ---- 7: readers of A between two steps see the current matrix -------------------------------------------------------------------------------
def _read_A(i, s, rec):
    if i in (2, 3):
        be = s.backend
        v = torch.linspace(-1.0, 1.0, be.x.numel(), dtype=torch.float64, device=be.x.device)
        y = torch.empty_like(v)
        be.spmv(v, y)
        A = be.csr()
        rec["extra"] += [y.cpu().numpy(), A.data.copy(), np.array([be.matrix_max_abs()])]
        # the matrix step i solved with (csr() sorts each row's columns, knp_get_csr_values keeps the library's order) ...
        assert np.array_equal(np.sort(A.data), np.sort(rec["A"][-1]))
        assert np.array_equal(_matrix_values(be), rec["A"][-1])          # ... and still that after the reads
        ref = A @ v.cpu().numpy()
        assert np.allclose(y.cpu().numpy(), ref, rtol=0, atol=1e-12 * np.abs(A).dot(np.abs(v.cpu().numpy())).max())


def test_readers_between_steps_see_the_current_matrix():
    a, b = _run(True, between=_read_A, **SQUARE32), _run(False, between=_read_A, **SQUARE32)
    _same_bits(a, b)      # (the reads themselves, in `extra`, and every following step)
    assert len(a["extra"]) == 6
    assert a["stats"]["asm_ahead"] == 3 and a["stats"]["asm_ahead_discarded"] == 0      # reading A costs no adoption
