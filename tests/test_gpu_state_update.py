"""The state variables of membrane mechanisms on the GPU (``k_state_update``, knp_state_* in csrc/knp_states.inc):

1. the raw entry point with Hodgkin-Huxley's gates as three programs against ``knp_hh_update`` (|d| <= 1e-12 absolute, the
   tolerance test_gpu_parity.py holds ``k_hh_update`` to), at counts around the lane, wave and block edges of 128 lanes per block;
2. gates and general states of every keyword form through ``ProblemKNPEMI`` against tests/state_program_ref.py (long double),
   1e-12 relative to max |y|;
3. three steps of ``SolverKNPEMI`` with the gates declared through ``add_state`` against the built-in ``HodgkinHuxley``, interpreter
   and run-time compiled currents;
4. the same through ``SolverEMI`` against ``HH_model``;
5. repeatability, no knp_state_* call without states, the checkpoint; 6. the argument errors of the ABI.

The end-to-end tolerances are measured in the test, on existing code: ten times the spread, per field and relative to the field's
maximum, between two runs of the BUILT-IN model -- ``KNP_JIT=0`` against ``KNP_JIT=1`` for KNP-EMI, PCG at rtol 1e-12 against
1e-13 for EMI.  The tests print the spread and the difference of every field.

Measured on MI355X (also in DESIGN.md section 10):
  1. largest |state programs - k_hh_update| over the 24 cases: 1.1e-16;
  2. largest error relative to max |y| against the long-double reference: 1.1e-15;
  3. square 8: built-in spread 6e-16 .. 1.1e-10 over the eight fields and phi_m (largest: phi_e), 3.8e-16 / 5.2e-16 / 1.6e-16 for
     n / m / h; cube 4: 7e-9 .. 2.6e-7 over the fields, 6.6e-11 / 5.5e-10 / 1.0e-12 for the gates (GMRES at rtol 1e-9).  Declared
     gates against the built-in model, either engine: 0 in every field, at most 3.8e-16 / 9.1e-16 / 1.6e-16 in n / m / h;
  4. EMI square 8: HH_model spread 5.9e-13 / 1.5e-12 / 7.3e-13 for phi_i / phi_e / phi_M, 4.0e-14 / 2.7e-13 / 5.2e-14 for n / m / h;
     declared gates against HH_model: 0 in the potentials, 1.7e-16 / 4.4e-16 / 1.7e-16 in the gates.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

import state_models as M
import state_program_ref as R
from parity_utils import ci_config, make_problem

from cgx_hip import _lib

pytestmark = pytest.mark.gpu
MODES = [(True, 25), (False, 1), (False, 25)]       # (Rush-Larsen, sub-steps)
SENTINEL = -7.25


@contextlib.contextmanager
def _jit(value):
    saved = os.environ.get("KNP_JIT")
    os.environ["KNP_JIT"] = value
    try:
        yield
    finally:
        os.environ.pop("KNP_JIT", None)
        if saved is not None:
            os.environ["KNP_JIT"] = saved


def _dev(a, be):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=be.device)


def _i32(a):
    return a.ctypes.data_as(_lib.i32p)


def _f64(a):
    return a.ctypes.data_as(_lib.f64p) if a.size else None


def _set_programs(be, states):
    be.check(be.lib.knp_state_reset(be.ctx, len(states)))
    for s, st in enumerate(states):
        code, consts = np.ascontiguousarray(st.spec.code, dtype=np.int32), st.spec.constants()
        be.check(be.lib.knp_state_set_program(be.ctx, s, st.kind, st.aux_index, code.shape[0], _i32(code), consts.shape[0], _f64(consts)))


# ------------------------------------------------------------------------------------------ 1. raw entry point
@pytest.fixture(scope="module")
def raw():
    """a context on square 16 (289 vertices) and the three gate programs of Hodgkin-Huxley, compiled by the product"""
    p = make_problem(ci_config(N=16, steps=1), M.hh_from_states_models())
    be = p.create_backend()
    _set_programs(be, p.state_variables)
    return p, be


@pytest.mark.parametrize("count", [1, 63, 64, 65, 127, 128, 129, 257])
@pytest.mark.parametrize("rush_larsen,substeps", MODES)
def test_raw_update_against_knp_hh_update(raw, count, rush_larsen, substeps):
    p, be = raw
    rng = np.random.default_rng(1000 * count + substeps + int(rush_larsen))
    rest, dt = float(p.phi_rest.value), float(p.dt.value)
    pad = 64
    phi_h = np.concatenate([M.away_from_singularities(rng, count, rest), np.full(pad, SENTINEL)])
    gates_h = [np.concatenate([rng.uniform(0.01, 0.99, count), np.full(pad, SENTINEL)]) for _ in range(3)]
    other_h = rng.uniform(-1.0, 1.0, count + pad)
    phi, other = _dev(phi_h, be), _dev(other_h, be)
    mine, ref = [_dev(g, be) for g in gates_h], [_dev(g, be) for g in gates_h]
    f = _lib.Fields()                       # no concentrations: the programs read none
    f.phi_m = phi.data_ptr()
    f.aux[3] = other.data_ptr()             # an aux field that is not a state
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in mine])
    be.check(be.lib.knp_state_update(be.ctx, C.byref(f), ptrs, count, dt, int(rush_larsen), substeps))
    be.check(be.lib.knp_hh_update(be.ctx, C.c_void_p(phi.data_ptr()), *[C.c_void_p(t.data_ptr()) for t in ref], count, dt, rest,
                                  int(rush_larsen), substeps))
    torch.cuda.synchronize()
    for nm, a, b, g0 in zip("nmh", mine, ref, gates_h):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        err = float(np.max(np.abs(a[:count] - b[:count])))
        print(f"count {count}, RL {rush_larsen}, {substeps} sub-steps, {nm}: max |state program - k_hh_update| = {err:.3e}")
        assert np.all(np.isfinite(b[:count])) and not np.array_equal(b[:count], g0[:count])
        assert err <= 1e-12
        assert np.array_equal(a[count:], np.full(pad, SENTINEL))
    assert np.array_equal(phi.cpu().numpy(), phi_h) and np.array_equal(other.cpu().numpy(), other_h)


# ------------------------------------------------------------------------------------------ 2. against state_program_ref
def _mixed_problem(kind, N, seed=4):
    """the mechanism of every keyword form on a mesh, random phi_m and concentrations on the device"""
    p = make_problem(ci_config(N=N, steps=1, kind=kind), lambda q: [M.Mixed(q)])
    rng = np.random.default_rng(seed)
    n = p.mesh.num_vertices
    p.phi_m_prev.x.array[:] = torch.as_tensor(rng.uniform(-0.1, 0.05, n), device=p.mesh.device)
    for side in (0, 1):
        for j in range(3):
            p.wh[side][j].x.array[:] = torch.as_tensor(rng.uniform(3.0, 150.0, n), device=p.mesh.device)
    return p


def _reference_step(p, y, rush_larsen, substeps):
    x = p.mesh.geometry.x
    return R.state_step(p.state_variables, y, p.phi_m_prev.numpy(), float(p.dt.value), rush_larsen, substeps,
                        ki=[p.wh[0][j].numpy() for j in range(3)], ke=[p.wh[1][j].numpy() for j in range(3)],
                        x=[x[:, d] for d in range(x.shape[1])])


def _two_updates(kind, N, rush_larsen, substeps):
    """two steps on the device, the Constant ``drive`` changed in between; the values after each"""
    p = _mixed_problem(kind, N)
    p.state_rush_larsen, p.state_substeps = rush_larsen, substeps
    be = p.create_backend()
    model = p.ionic_models[0]
    y0 = [st.function.numpy().copy() for st in p.state_variables]
    got = []
    for drive in (1.0, 0.25):
        model.drive.value = drive
        be.state_update()
        got.append([st.function.numpy().copy() for st in p.state_variables])
    return p, model, y0, got


@pytest.mark.parametrize("kind,N,n_vertices", [("square", 8, 81), ("cube", 4, 125)])
@pytest.mark.parametrize("rush_larsen,substeps", MODES)
def test_every_keyword_form_against_the_reference(kind, N, n_vertices, rush_larsen, substeps):
    p, model, y, got = _two_updates(kind, N, rush_larsen, substeps)
    assert p.mesh.num_vertices == n_vertices and p.backend.state_calls > 0
    for step, drive in enumerate((1.0, 0.25)):
        model.drive.value = drive
        y = _reference_step(p, y, rush_larsen, substeps)
        for st, a, b in zip(p.state_variables, got[step], y):
            scale = float(np.max(np.abs(b)))
            err = float(np.max(np.abs(a - b.astype(np.float64)))) / scale
            print(f"{kind}{N}, RL {rush_larsen}, {substeps} sub-steps, call {step + 1}, {st.name}: max |y| = {scale:.3e}, relative error {err:.3e}")
            assert err <= 1e-12
    # the second call saw the new constant: u' = W v drive
    assert not np.array_equal(got[0][3], got[1][3])


# ------------------------------------------------------------------------------------------ 3. end to end, KNP-EMI
FIELDS = ["Na_i", "K_i", "Cl_i", "phi_i", "Na_e", "K_e", "Cl_e", "phi_e", "phi_m", "n", "m", "h"]
_RUNS = {}


def _knp_run(kind, N, models, jit, out_dir=None):
    """three steps of SolverKNPEMI; the twelve fields on the host, the backend's knp_state_* call count"""
    key = (kind, N, models, jit, out_dir)
    if key not in _RUNS:
        from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
        cfg = ci_config(N=N, steps=3, kind=kind)
        if out_dir:
            cfg["output_dir"] = out_dir
            cfg["solver"]["output"].update({"save_cpoints": True, "save_interval": 1})
        with _jit(jit):
            p = make_problem(cfg, "ci" if models == "builtin" else M.hh_from_states_models())
            p.solver_config["view_ksp"] = False
            s = SolverKNPEMI(p, solver_config=p.solver_config)
            s.solve()
            status = s.backend.lib.knp_jit_status(s.backend.ctx).decode()
        assert all(r > 0 for r in s.reasons)
        vals = [p.wh[side][j].numpy().copy() for side in (0, 1) for j in range(4)] + [f.numpy().copy() for f in (p.phi_m_prev, p.n, p.m, p.h)]
        _RUNS[key] = (dict(zip(FIELDS, vals)), s.backend.state_calls, status, len(s.ode_time))
    return _RUNS[key]


@pytest.mark.parametrize("kind,N", [("square", 8), ("cube", 4)])
@pytest.mark.parametrize("jit", ["0", "1"])
def test_knpemi_with_declared_gates_against_the_built_in_model(kind, N, jit):
    base0, calls0, st0, _ = _knp_run(kind, N, "builtin", "0")
    base1, calls1, st1, _ = _knp_run(kind, N, "builtin", "1")
    got, calls, status, n_ode = _knp_run(kind, N, "states", jit)
    ref = base0 if jit == "0" else base1
    assert calls0 == calls1 == 0 and calls > 0 and n_ode == 3
    print(f"{kind}{N}: jit status built-in {st0!r} / {st1!r}, declared gates {status!r}")
    # the allowance is the spread between the interpreter and the run-time compiled code: both engines must have run
    assert "KNP_JIT=0" in st0 and st1 == "native" and (status == "native") == (jit == "1")
    bad = []
    for nm in FIELDS:
        scale = float(np.max(np.abs(ref[nm])))
        spread = float(np.max(np.abs(base0[nm] - base1[nm]))) / scale
        err = float(np.max(np.abs(got[nm] - ref[nm]))) / scale
        print(f"{kind}{N} KNP_JIT={jit} {nm}: built-in spread interpreter / compiled {spread:.3e}, declared gates - built-in {err:.3e}")
        if not err <= 10.0 * spread:
            bad.append(nm)
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 4. end to end, EMI
EMI_FIELDS = ["phi_i", "phi_e", "phi_M", "n", "m", "h"]


def _emi_run(models, direct_rtol, pc_type="jacobi"):
    """``pc_type`` None: the solver's default"""
    from cgx_hip.emi_models import g_syn
    from cgx_hip.emi_problem import ProblemEMI
    from cgx_hip.emi_solver import SolverEMI
    # The mesh stays in the config's units (conversion factor 1): the matrix then has a condition number of 1e3 and PCG reaches
    # rtol 1e-13 in some 20 iterations.  Scaled to micrometres (the other EMI tests) it is 2e5 and PCG stalls at 3e-12 of ||b||, so
    # the finer of the two reference runs would not exist.  The preconditioner is point Jacobi: a step takes some 20 iterations, of
    # which the last brings about a decade, so the two tolerances stop at different iterates.  With the AMG cycle one iteration
    # crosses both thresholds and the two reference runs are the same bits -- no spread to measure.
    cfg = {"problem_type": "EMI", "dt": 5e-5, "time_steps": 3, "C_M": 0.02, "sigma_i": 0.7, "sigma_e": 1.3, "quiet": True,
           "cell_tag_file": "square8.xdmf", "facet_tag_file": "square8.xdmf", "ics_tags": [1], "ecs_tags": [2], "membrane_tags": [4]}
    p = ProblemEMI(cfg)
    if models == "builtin":
        p.add_ionic_model("HH", stim_fun=g_syn)
        p.init_ionic_model()
    else:
        p.init_ionic_model([M.HHStatesEMI(p, stim_fun=g_syn)])

    class S(SolverEMI):
        pass
    S.direct_rtol = direct_rtol
    if pc_type is not None:
        S.pc_type = pc_type
    s = S(p, use_direct_solver=True)
    s.solve()
    assert all(r > 0 for r in s.reasons) and len(s.iterations) == 3
    gates = (p.n, p.m, p.h) if models == "builtin" else tuple(getattr(p.ionic_models[0], g) for g in "nmh")
    vals = [p.wh[0].numpy().copy(), p.wh[1].numpy().copy(), p.phi_M.numpy().copy()] + [g.numpy().copy() for g in gates]
    return dict(zip(EMI_FIELDS, vals)), s.backend.state_calls


def test_emi_with_declared_gates_against_hh_model():
    ref, calls_ref = _emi_run("builtin", 1e-12)
    finer, _ = _emi_run("builtin", 1e-13)
    got, calls = _emi_run("states", 1e-12)
    assert calls_ref == 0 and calls > 0
    assert np.max(np.abs(ref["phi_M"] + 0.06774)) > 1e-4           # the stimulus moved the membrane
    assert not np.array_equal(ref["phi_M"], finer["phi_M"])        # ... and the two reference runs differ: there is a spread
    bad = []
    for nm in EMI_FIELDS:
        scale = float(np.max(np.abs(ref[nm])))
        spread = float(np.max(np.abs(ref[nm] - finer[nm]))) / scale
        err = float(np.max(np.abs(got[nm] - ref[nm]))) / scale
        print(f"EMI square8 {nm}: HH_model spread rtol 1e-12 / 1e-13 {spread:.3e}, declared gates - HH_model {err:.3e}")
        if not err <= 10.0 * spread:
            bad.append(nm)
    assert not bad, bad
    # the solver as users get it (pc_type hypre: the AMG cycle), same allowance: the spread above is that of HH_model itself
    ref_amg, _ = _emi_run("builtin", 1e-12, None)
    got_amg, calls_amg = _emi_run("states", 1e-12, None)
    assert calls_amg > 0
    for nm in EMI_FIELDS:
        scale = float(np.max(np.abs(ref[nm])))
        spread = float(np.max(np.abs(ref[nm] - finer[nm]))) / scale
        err = float(np.max(np.abs(got_amg[nm] - ref_amg[nm]))) / scale
        print(f"EMI square8 {nm}, default preconditioner: declared gates - HH_model {err:.3e} (allowance 10 x {spread:.3e})")
        if not err <= 10.0 * spread:
            bad.append(nm)
    assert not bad, bad


# ------------------------------------------------------------------------------------------ 5. repeatability, idleness, checkpoint
def test_two_identical_runs_give_identical_bits():
    a = _two_updates("cube", 4, False, 25)[3]
    b = _two_updates("cube", 4, False, 25)[3]
    for step in range(2):
        for x, y in zip(a[step], b[step]):
            assert np.array_equal(x, y)


def test_checkpoint_holds_the_states_and_a_run_without_states_calls_nothing(tmp_path):
    """the states q, g, y, u, v of ``Mixed`` are no attributes of the problem: only the loop over the declared states writes them"""
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    out = str(tmp_path) + os.sep
    cfg = ci_config(N=8, steps=2)
    cfg["output_dir"] = out
    cfg["solver"]["output"].update({"save_cpoints": True, "save_interval": 1})
    p = make_problem(cfg, lambda q: [M.Mixed(q)])
    p.solver_config["view_ksp"] = False
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    s.solve()
    assert all(r > 0 for r in s.reasons) and s.backend.state_calls > 0 and not any(hasattr(p, g) for g in "nmh")
    ck = np.load(os.path.join(out, "checkpoints", "step_000002_rank0.npz"))
    nvo = p.local_mesh.n_vertices_owned
    assert [st.name for st in p.state_variables] == ["q", "g", "y", "u", "v"]
    for st in p.state_variables:
        assert st.name in ck.files and np.array_equal(ck[st.name], st.function.numpy()[:nvo])
    first = np.load(os.path.join(out, "checkpoints", "step_000001_rank0.npz"))
    assert not np.array_equal(first["y"], ck["y"]) and not np.array_equal(first["u"], ck["u"])      # the states moved between the two
    _, calls0, _, n_ode = _knp_run("square", 8, "builtin", "0")
    assert calls0 == 0 and n_ode == 3


def test_zero_rates_keep_a_rush_larsen_gate():
    """alpha = beta = 0 on half of the mesh: the gate stays there (no 0 / 0); elsewhere it follows the reference"""
    p = make_problem(ci_config(N=8, steps=1), lambda q: [M.MaskedGate(q)])
    be = p.create_backend()
    y0 = [st.function.numpy().copy() for st in p.state_variables]
    be.state_update()
    got = [st.function.numpy().copy() for st in p.state_variables]
    want = _reference_step(p, y0, True, 25)
    off = p.mesh.geometry.x[:, 0] <= 0.5e-6
    assert 0 < off.sum() < off.size and np.array_equal(got[0][off], y0[0][off]) and not np.any(got[0][~off] == y0[0][~off])
    for a, b in zip(got, want):
        assert np.all(np.isfinite(a)) and np.max(np.abs(a - b.astype(np.float64))) <= 1e-12 * float(np.max(np.abs(b)))


def test_backend_created_before_the_programs_are_compiled():
    """problem -> models -> backend -> setup_variational_form: the backend takes the state programs when they exist"""
    from cgx_hip.problem import ProblemKNPEMI
    p = ProblemKNPEMI(ci_config(N=8, steps=1))
    p.set_initial_conditions()
    p.init_ionic_models([M.Mixed(p)])
    be = p.create_backend()
    assert be.state_calls == 0 and all(st.spec is None for st in p.state_variables)
    p.setup_variational_form()
    assert be.state_calls == 1 + len(p.state_variables)
    be.state_update()
    torch.cuda.synchronize()
    assert np.all(np.isfinite(p.ionic_models[0].y.numpy())) and not np.all(p.ionic_models[0].y.numpy() == 0.05)


# ------------------------------------------------------------------------------------------ 6. ABI errors
def test_invalid_calls_return_an_error_and_launch_nothing(raw):
    p, be = raw
    lib, ctx = be.lib, be.ctx
    states = p.state_variables
    code, consts = np.ascontiguousarray(states[0].spec.code, dtype=np.int32), states[0].spec.constants()
    n = 64
    phi = _dev(np.full(n, -0.065), be)
    bufs = [_dev(np.full(n, 0.5), be) for _ in range(3)]
    f = _lib.Fields()
    f.phi_m = phi.data_ptr()
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in bufs])
    dt = 2.5e-5

    def refused(rc, code_wanted, *words):
        msg = lib.knp_last_error(ctx).decode()
        assert rc == code_wanted and msg and all(w in msg for w in words), (rc, msg)

    E_ARG, E_STATE = -1, -3
    refused(lib.knp_state_reset(ctx, -1), E_ARG, "number of states")
    refused(lib.knp_state_reset(ctx, _lib.KNP_MAX_AUX + 1), E_ARG, "number of states")
    # update before set
    be.check(lib.knp_state_reset(ctx, 0))
    refused(lib.knp_state_update(ctx, C.byref(f), ptrs, n, dt, 1, 25), E_STATE, "no states")
    be.check(lib.knp_state_reset(ctx, 3))
    refused(lib.knp_state_update(ctx, C.byref(f), ptrs, n, dt, 1, 25), E_STATE, "not set")
    set_program = lambda slot, kind, aux, n_instr, cd, nc=consts.shape[0]: lib.knp_state_set_program(ctx, slot, kind, aux, n_instr, _i32(cd), nc, _f64(consts))
    refused(set_program(3, 0, 0, code.shape[0], code), E_ARG, "slot out of range")
    refused(set_program(-1, 0, 0, code.shape[0], code), E_ARG, "slot out of range")
    refused(set_program(0, 2, 0, code.shape[0], code), E_ARG, "kind")
    refused(set_program(0, 0, _lib.KNP_MAX_AUX, code.shape[0], code), E_ARG, "aux_index")
    refused(set_program(0, 0, -1, code.shape[0], code), E_ARG, "aux_index")
    long_code = np.ascontiguousarray(np.tile(code, (_lib.KNP_STATE_MAX_INSTR // code.shape[0] + 1, 1)))
    refused(set_program(0, 0, 0, long_code.shape[0], long_code), E_ARG, "too long")
    bad = code.copy()
    bad[0, 1] = _lib.KNP_MAX_PROG_REGS          # a register past the file
    refused(set_program(0, 0, 0, bad.shape[0], bad), E_ARG, "invalid membrane program instruction")
    refused(lib.knp_state_set_program(ctx, 0, 0, 0, code.shape[0], None, consts.shape[0], _f64(consts)), E_ARG, "bad state program")
    be.check(set_program(0, 0, 0, code.shape[0], code))
    refused(set_program(1, 0, 0, code.shape[0], code), E_ARG, "share aux slot")
    refused(lib.knp_state_set_constants(ctx, 0, consts.shape[0] + 1, _f64(consts)), E_ARG, "mismatch")
    refused(lib.knp_state_set_constants(ctx, 1, consts.shape[0], _f64(consts)), E_ARG, "mismatch")      # slot 1 has no program yet
    refused(lib.knp_state_set_constants(ctx, 5, consts.shape[0], _f64(consts)), E_ARG, "slot out of range")
    _set_programs(be, states)
    refused(lib.knp_state_update(ctx, C.byref(f), ptrs, -1, dt, 1, 25), E_ARG, "count")
    refused(lib.knp_state_update(ctx, C.byref(f), ptrs, p.mesh.num_vertices + 1, dt, 1, 25), E_ARG, "count")
    refused(lib.knp_state_update(ctx, C.byref(f), ptrs, n, 0.0, 1, 25), E_ARG, "dt > 0")
    refused(lib.knp_state_update(ctx, C.byref(f), ptrs, n, dt, 1, 0), E_ARG, "substeps")
    refused(lib.knp_state_update(ctx, None, ptrs, n, dt, 1, 25), E_ARG, "null fields")
    refused(lib.knp_state_update(ctx, C.byref(_lib.Fields()), ptrs, n, dt, 1, 25), E_ARG, "phi_m")
    refused(lib.knp_state_update(ctx, C.byref(f), None, n, dt, 1, 25), E_ARG, "null state pointer")
    holes = (C.c_void_p * 3)(bufs[0].data_ptr(), None, bufs[2].data_ptr())
    refused(lib.knp_state_update(ctx, C.byref(f), holes, n, dt, 1, 25), E_ARG, "null state buffer 1")
    # a program that reads a concentration, and fields without one: an error, not a fault
    q = _mixed_problem("square", 8)
    g = next(st for st in q.state_variables if st.name == "g")
    gc, gk = np.ascontiguousarray(g.spec.code, dtype=np.int32), g.spec.constants()
    be.check(lib.knp_state_reset(ctx, 1))
    be.check(lib.knp_state_set_program(ctx, 0, g.kind, 0, gc.shape[0], _i32(gc), gk.shape[0], _f64(gk)))
    refused(lib.knp_state_update(ctx, C.byref(f), ptrs, n, dt, 1, 25), E_ARG, "null concentration field")
    # nothing was launched: the buffers are as they were; count 0 is a successful no-op
    _set_programs(be, states)
    be.check(lib.knp_state_update(ctx, C.byref(f), ptrs, 0, dt, 1, 25))
    torch.cuda.synchronize()
    assert all(bool(torch.all(t == 0.5)) for t in bufs) and bool(torch.all(phi == -0.065))
    be.check(lib.knp_state_update(ctx, C.byref(f), ptrs, n, dt, 1, 25))        # and the context still works
    torch.cuda.synchronize()
    assert all(bool(torch.all(t != 0.5)) for t in bufs)
