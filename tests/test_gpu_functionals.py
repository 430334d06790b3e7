"""Volume functionals on the device (csrc/knp_functional.inc, cgx_hip/functionals.py): closed forms, the existing norm and budget
kernels, nonlinear integrands against the NumPy reference (tests/functional_ref.py), a tag longer than the wave combine, every error
of the raw ABI, the EMI model and a run that records functionals.

Tolerance throughout: |device - host| <= 1e-12 * sum |w f| per tag and output (``functional_ref.TOL``), the figure the ion-budget and
stimulus tests hold the same reduction to."""
import ctypes as C

import numpy as np
import pytest
import torch

import functional_ref
from functional_raw import RawVolume as _Raw
from functional_raw import _f64, _i32
from functional_ref import TOL
from parity_utils import ci_config, make_problem, tissue_config

pytestmark = pytest.mark.gpu


def _randomize(p, seed):
    """random fields, as tests/test_gpu_ion_budget.py::long_tags writes them, and one user Function"""
    from cgx_hip import fem
    rng = np.random.default_rng(seed)
    n = p.local_mesh.coords.shape[0]
    write = lambda fn, v: fn.x.array.copy_(torch.from_numpy(v).to(fn.x.array.device))
    for s in range(2):
        for j in range(p.N_ions):
            write(p.wh[s][j], rng.uniform(1.0, 150.0, n))
        write(p.wh[s][p.N_ions], rng.uniform(-0.1, 0.1, n))
    write(p.phi_m_prev, p.wh[0][p.N_ions].numpy() - p.wh[1][p.N_ions].numpy())
    user = fem.Function(p.V, "user")
    write(user, rng.uniform(-2.0, 3.0, n))
    return user


CONFIGS = {"square": lambda: ci_config(N=8, steps=1), "cube": lambda: ci_config(N=8, steps=1, kind="cube"),
           "tissue": lambda: tissue_config(2, 18, 3, steps=1)}


@pytest.fixture(scope="module")
def problems():
    made = {}

    def get(case):
        if case not in made:
            p = make_problem(CONFIGS[case](), "ci")
            be = p.create_backend()
            made[case] = (p, be, _randomize(p, 11 + len(made)))
        return made[case]
    return get


def _check(got, want, scale, what):
    got, want, scale = (np.asarray(a, dtype=np.float64) for a in (got, want, scale))
    err = np.abs(got - want)
    print(f"{what}: max |device - host| / sum|w f| = {np.max(err / np.maximum(scale, 1e-300)):.3e}")
    assert got.shape == want.shape and np.all(np.isfinite(got))
    assert np.all(err <= TOL * scale), (what, err, TOL * scale)


def _tag_cells(p, tag):
    lm = p.local_mesh
    nco = int(lm.n_cells_owned)
    return lm.cells[:nco][np.asarray(lm.cell_tags[:nco]) == tag]


CASES = ["square", "cube", "tissue"]


@pytest.mark.parametrize("case", CASES)
def test_integrand_one_gives_the_volumes(problems, case):
    from cgx_hip.functionals import VolumeFunctional
    p, be, _ = problems(case)
    F = VolumeFunctional(p, 1.0, 1.0)
    lay = be.budget_layout()
    assert np.array_equal(F.tags, lay.tags) and np.array_equal(F.side, lay.side)
    v = F.value()
    assert v.shape == (len(lay.tags), 1)
    if case == "tissue":
        assert (F.side == 0).sum() == 9      # many short tags, several per chunk of 128 cells
    _check(v[:, 0], F.volume, F.volume, "volume attribute")
    _check(v[:, 0], lay.volume, lay.volume, "budget layout volumes")
    assert F.total()[0] == pytest.approx(lay.volume.sum(), rel=1e-12)
    assert p.assemble_scalar(1.0, 1.0) == pytest.approx(lay.volume.sum(), rel=1e-12)


@pytest.mark.parametrize("case", CASES)
def test_mass_and_stiffness_closed_forms(problems, case):
    """u v at degree 2 is u^T M v, inner(grad u, grad v) is u^T K v: u a concentration (KI / KE), v the potential (an aux field)"""
    from cgx_hip import fem
    from cgx_hip.functionals import VolumeFunctional
    p, be, _ = problems(case)
    forms = [[p.wh[s][0] * p.wh[s][3], fem.inner(fem.grad(p.wh[s][0]), fem.grad(p.wh[s][3]))] for s in range(2)]
    F = VolumeFunctional(p, forms[0], forms[1], degree=2)
    got = F.value()
    tags, side, _, scale = functional_ref.reference(p, forms[0], forms[1], degree=2)
    assert np.array_equal(tags, F.tags) and np.array_equal(side, F.side)
    coords = p.local_mesh.coords
    want = np.array([[functional_ref.mass_form(coords, _tag_cells(p, t), p.wh[s][0].numpy(), p.wh[s][3].numpy())[0],
                      functional_ref.stiffness_form(coords, _tag_cells(p, t), p.wh[s][0].numpy(), p.wh[s][3].numpy())[0]]
                     for t, s in zip(tags, side)])
    assert np.abs(want).min() > 0
    _check(got[:, 0], want[:, 0], scale[:, 0], "u^T M v")
    _check(got[:, 1], want[:, 1], scale[:, 1], "u^T K v")


@pytest.mark.parametrize("case", CASES)
def test_cubic_integrand_needs_degree_three(problems, case):
    from cgx_hip.functionals import VolumeFunctional
    p, be, user = problems(case)
    forms = [p.wh[s][1] * p.wh[s][3] * user for s in range(2)]
    _, _, want, scale = functional_ref.reference(p, forms[0], forms[1], degree=3)
    F3 = VolumeFunctional(p, forms[0], forms[1], degree=3)
    assert F3.spec.q_w.shape[0] == 2 ** p.local_mesh.coords.shape[1]
    _check(F3.value(), want, scale, "u v w at degree 3")
    F1 = VolumeFunctional(p, forms[0], forms[1], degree=1)
    assert F1.spec.q_w.shape[0] == 1
    low = F1.value()
    _, _, want1, scale1 = functional_ref.reference(p, forms[0], forms[1], degree=1)
    _check(low, want1, scale1, "u v w at degree 1")
    assert np.all(np.abs(low - want) > 1e-6 * np.abs(want))


@pytest.mark.parametrize("case", CASES)
def test_against_the_norm_and_budget_kernels(problems, case):
    from cgx_hip.functionals import VolumeFunctional
    p, be, _ = problems(case)
    phi = [p.wh[s][p.N_ions] for s in range(2)]
    F = VolumeFunctional(p, phi[0] * phi[0], phi[1] * phi[1])
    v = F.value()[:, 0]
    ni, ne = be.l2_norms_sq()
    _, _, _, scale = functional_ref.reference(p, phi[0] * phi[0], phi[1] * phi[1])
    for s, norm in enumerate((ni, ne)):
        _check(v[F.side == s].sum(), norm, scale[F.side == s, 0].sum(), f"phi^2 against knp_l2_norms, side {s}")
    G = VolumeFunctional(p, list(p.wh[0][:3]), list(p.wh[1][:3]))
    amounts = be.ion_amounts().cpu().numpy()
    assert G.n_out == 3 and np.array_equal(G.tags, be.budget_layout().tags)
    _check(G.value(), amounts, np.abs(amounts), "three concentrations against knp_diag_volume_integrals")
    tot = p.assemble_scalar(list(p.wh[0][:3]), list(p.wh[1][:3]))
    assert tot.shape == (3,) and np.allclose(tot, amounts.sum(axis=0), rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", CASES)
def test_nonlinear_integrands_and_a_time_dependent_constant(problems, case):
    from cgx_hip import fem
    from cgx_hip.functionals import VolumeFunctional
    p, be, user = problems(case)
    x = fem.SpatialCoordinate(p.mesh)
    xc = float(p.local_mesh.coords[:, 0].mean())
    amp = fem.Constant(p.mesh, 0.25)
    forms = []
    for s in range(2):
        c, phi = p.wh[s][2], p.wh[s][p.N_ions]
        forms.append([c * fem.ln(c / 75.0), fem.exp(12.0 * phi) + fem.sqrt(abs(user) + 1.0),
                      amp * fem.conditional(fem.lt(x[0], xc), c, -2.0 * p.wh[s][0]) * phi ** 2])
    F = VolumeFunctional(p, forms[0], forms[1], degree=4)
    assert F.spec.q_w.shape[0] == 3 ** p.local_mesh.coords.shape[1]
    for value in (0.25, -1.75):
        amp.value = value
        _, _, want, scale = functional_ref.reference(p, forms[0], forms[1], degree=4)
        got = F.value()
        assert np.abs(want[:, 2]).min() > 0
        _check(got, want, scale, f"nonlinear integrands, amplitude {value}")
    assert abs(F.value()[0, 2] / want[0, 2] - 1.0) < 1e-9      # the second constant reached the device
    # a subset of the tags, in the caller's order within a side, and one side only
    some = [int(F.tags[-1]), int(F.tags[0])]
    H = VolumeFunctional(p, forms[0], forms[1], tags=some, degree=4)
    assert list(H.tags) == [some[1], some[0]]
    assert np.array_equal(H.value(), F.value()[[0, len(F.tags) - 1]])
    E = VolumeFunctional(p, integrand_e=forms[1][0], degree=4)
    assert list(E.side) == [1] * len(E.tags) and np.array_equal(E.value()[:, 0], F.value()[F.side == 1, 0])


def test_a_function_bound_to_another_tensor_is_read_where_it_is(problems):
    """the device pointers are taken at every call, not kept from the construction"""
    from cgx_hip.functionals import VolumeFunctional
    p, be, user = problems("square")
    F = VolumeFunctional(p, user * p.wh[0][0], user * p.wh[1][0])
    before = F.value()
    kept = user.x.array
    try:
        user.x.array = kept * 2.0                 # a new tensor; doubling is exact
        assert user.x.array.data_ptr() != kept.data_ptr()
        assert np.array_equal(F.value(), 2.0 * before)
    finally:
        user.x.array = kept
    assert np.array_equal(F.value(), before) and np.abs(before).min() > 0


@pytest.fixture(scope="module")
def long_tags():
    """tissue_config(3, 30, 5) with random fields: the extracellular tag has more chunks than the 64 lanes of the combine's wave"""
    p = make_problem(tissue_config(3, 30, 5, steps=1), "ci")
    be = p.create_backend()
    return p, be, _randomize(p, 29)


def test_a_tag_of_more_than_64_chunks(long_tags):
    from cgx_hip import fem
    from cgx_hip.functionals import VolumeFunctional
    p, be, user = long_tags
    forms = [[p.wh[s][0] * fem.ln(p.wh[s][1]), fem.inner(fem.grad(p.wh[s][3]), fem.grad(user))] for s in range(2)]
    F = VolumeFunctional(p, forms[0], forms[1])
    ext = F.spec.sides[1]
    chunks = (ext.seg_ptr[1] - 1) // 128 - ext.seg_ptr[0] // 128 + 1
    print("extracellular tag:", ext.seg_ptr[1] - ext.seg_ptr[0], "cells in", chunks, "chunks of 128")
    assert len(ext.tags) == 1 and chunks > 64
    intra = F.spec.sides[0]
    assert np.all(np.diff(intra.seg_ptr) // 128 + 2 <= 64)      # and the intracellular tags stay with the wave combine
    got = F.value()
    _, _, want, scale = functional_ref.reference(p, forms[0], forms[1])
    _check(got, want, scale, "long tag")
    assert F.value().tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------ the raw ABI
def test_every_error_of_the_raw_abi(problems):
    from cgx_hip import _lib
    from cgx_hip._lib import OPS
    p, be, user = problems("square")
    lib, ctx = be.lib, be.ctx
    nc, dim = int(p.local_mesh.n_cells_owned), 2
    raw = _Raw(be, nc, dim)
    E_ARG = -1
    code = raw.args["code"]

    def prog(*rows):
        return dict(code=np.array(rows, dtype=np.int32), n_instr=len(rows))
    bad = {
        "null id": dict(id=False), "null q_bary": dict(q_bary=None), "null q_w": dict(q_w=None), "null code": dict(code=None),
        "null consts": dict(n_consts=1, consts=None), "null aux_deriv": dict(aux_deriv=None), "null seg_ptr": dict(seg_ptr=None),
        "null cells": dict(cells=None),
        "n_q 0": dict(n_q=0), "n_q 126": dict(n_q=_lib.KNP_FUNCTIONAL_MAX_Q + 1, q_bary=np.zeros((126, 3)), q_w=np.full(126, 1 / 126)),
        "n_out 0": dict(n_out=0), "n_out 4": dict(n_out=4),
        "n_aux -1": dict(n_aux=-1), "n_aux 9": dict(n_aux=_lib.KNP_MAX_AUX + 1, aux_deriv=np.full(9, -1, dtype=np.int32)),
        "aux_deriv -2": dict(aux_deriv=np.array([-2], dtype=np.int32)), "aux_deriv dim": dict(aux_deriv=np.array([dim], dtype=np.int32)),
        "empty program": dict(n_instr=0),
        "unknown opcode": prog([99, 0, 0, 0], code[2]), "register 48": prog([OPS["AUX"], _lib.KNP_MAX_PROG_REGS, 0, 0], code[2]),
        "constant out of range": prog([OPS["CONST"], 0, 0, 0], [OPS["OUT"], 0, 0, 0]),
        "coordinate axis = dim": prog([OPS["X"], 0, dim, 0], [OPS["OUT"], 0, 0, 0]),
        "OUT index = n_out": prog(code[0], [OPS["OUT"], 0, 1, 0]), "aux slot = n_aux": prog([OPS["AUX"], 0, 1, 0], [OPS["OUT"], 0, 0, 0]),
        "65 constants": dict(n_consts=_lib.KNP_DIAG_MAX_CONSTS + 1, consts=np.zeros(65)), "negative constants": dict(n_consts=-1),
        "cell not owned": dict(cells=np.r_[np.arange(nc - 1), nc].astype(np.int32)),
        "negative cell": dict(cells=np.r_[np.arange(nc - 1), -1].astype(np.int32)),
        "cell listed twice": dict(cells=np.r_[np.arange(nc - 1), 0].astype(np.int32)),
        "seg_ptr[0] != 0": dict(seg_ptr=np.array([1, nc], dtype=np.int32)),
        "seg_ptr decreases": dict(n_tags=2, seg_ptr=np.array([0, 5, 3], dtype=np.int32)),
        "seg_ptr past the cells": dict(seg_ptr=np.array([0, nc + 1], dtype=np.int32), cells=np.arange(nc + 1, dtype=np.int32)),
        "negative n_tags": dict(n_tags=-1),
    }
    seen = set()
    for what, kw in bad.items():
        rc, fid = raw.create(**kw)
        msg = raw.error()
        assert rc == E_ARG and fid == -1 and msg, (what, rc, fid, msg)
        seen.add(msg)
    assert len(seen) >= 12      # the messages tell the causes apart
    # no plan was half-made: the first valid create takes slot 0
    rc, fid = raw.create()
    assert rc == 0 and fid == 0, raw.error()
    rc, second = raw.create(n_aux=2, aux_deriv=np.array([-1, 1], dtype=np.int32),
                            **prog(code[0], [OPS["AUX"], 1, 1, 0], [OPS["MUL"], 2, 0, 1], [OPS["OUT"], 0, 0, 2]))
    assert rc == 0 and second == 1, raw.error()
    # evaluation: only the pointers the code reads are needed
    sentinel = -123.25
    out = torch.full((1,), sentinel, dtype=torch.float64, device=be.device)
    optr = C.c_void_p(out.data_ptr())
    f = _lib.Fields()
    one = np.ones(1)

    def refused(rc, what):
        assert rc == E_ARG and raw.error(), (what, rc)
        torch.cuda.synchronize()
        assert float(out[0]) == sentinel, what      # nothing was launched
    refused(lib.knp_functional_eval(ctx, fid, C.byref(f), optr), "the aux field the code reads is null")
    refused(lib.knp_functional_eval(ctx, fid, None, optr), "null fields")
    refused(lib.knp_functional_eval(ctx, 7, C.byref(f), optr), "unknown id")
    refused(lib.knp_functional_eval(ctx, -1, C.byref(f), optr), "negative id")
    f.aux[0] = p.wh[0][3].data_ptr()
    refused(lib.knp_functional_eval(ctx, fid, C.byref(f), None), "null out")
    refused(lib.knp_functional_eval(ctx, second, C.byref(f), optr), "the second aux field is null")
    refused(lib.knp_functional_set_constants(ctx, fid, 1, _f64(one)), "constant count mismatch")
    refused(lib.knp_functional_set_constants(ctx, 7, 0, None), "unknown id")
    refused(lib.knp_functional_destroy(ctx, 7), "unknown id")
    assert lib.knp_functional_eval(ctx, fid, C.byref(f), optr) == 0, raw.error()      # concentrations and phi_m null: not read
    phi = p.wh[0][3]
    coords, cells = p.local_mesh.coords, p.local_mesh.cells[:nc]
    want, scale = functional_ref.mass_form(coords, cells, phi.numpy(), phi.numpy())
    assert abs(float(out[0]) - want) <= TOL * scale
    f.aux[1] = user.data_ptr()
    assert lib.knp_functional_eval(ctx, second, C.byref(f), optr) == 0, raw.error()
    G = functional_ref.simplex_gradients(coords[cells])
    w = functional_ref.cell_volumes(coords[cells]) * phi.numpy()[cells].mean(axis=1) * (G[:, :, 1] * user.numpy()[cells]).sum(axis=1)
    assert abs(float(out[0]) - w.sum()) <= TOL * np.abs(w).sum()
    assert lib.knp_functional_destroy(ctx, fid) == 0
    out.fill_(sentinel)
    refused(lib.knp_functional_eval(ctx, fid, C.byref(f), optr), "destroyed id")
    rc, again = raw.create()
    assert rc == 0 and again == fid      # the slot is reused
    # n_tags == 0 is a successful no-op
    rc, empty = raw.create(n_tags=0, seg_ptr=None, cells=None)
    assert rc == 0 and empty == 2, raw.error()
    assert lib.knp_functional_eval(ctx, empty, C.byref(f), optr) == 0
    torch.cuda.synchronize()
    assert float(out[0]) == sentinel
    for k in (again, second, empty):
        assert lib.knp_functional_destroy(ctx, k) == 0


def test_a_flat_cell_with_a_bound_derivative_is_a_mesh_error():
    """A hand-made mesh of three triangles, the third 1e-310 wide: its determinant is not zero, so the context builds, but the
    gradients of its barycentric coordinates overflow.  A functional that binds a derivative refuses the cell; one that does not
    takes it, and so does one with the derivative over the other cells."""
    from cgx_hip import _lib
    from cgx_hip._lib import OPS
    lib = _lib.load()
    torch.cuda.current_device()
    coords = np.array([[-1.0, -1.0], [0.0, -1.0], [-1.0, 0.0], [0.0, 0.0], [1e-310, 0.0], [0.0, 1.0]])
    cells = np.array([[0, 1, 2], [1, 3, 2], [3, 4, 5]], dtype=np.int32)
    side = np.array([0, 1, 1], dtype=np.uint8)
    gamma = np.array([[0, 0, 1, 1]], dtype=np.int32)
    gprog = np.zeros(1, dtype=np.int32)
    qp, qw = np.array([[0.5, 0.5]]), np.array([1.0])
    assert 0.0 < coords[4, 0] < 1.0 / np.finfo(np.float64).max      # its reciprocal overflows
    d = _lib.MeshDesc()
    d.dim, d.n_vertices, d.n_vertices_owned, d.n_cells, d.n_cells_owned = 2, 6, 6, 3, 3
    d.cells, d.coords, d.cell_side = _i32(cells), _f64(coords), side.ctypes.data_as(_lib.u8p)
    d.n_gamma, d.gamma, d.gamma_prog = 1, _i32(gamma), _i32(gprog)
    d.n_q, d.q_pts, d.q_w = 1, _f64(qp), _f64(qw)
    ctx = C.c_void_p()
    rc = lib.knp_create(C.byref(ctx), C.byref(d))
    assert rc == 0, lib.knp_last_error(ctx)
    try:
        class Be:
            pass
        be = Be()
        be.lib, be.ctx = lib, ctx
        raw = _Raw(be, 3, 2)
        deriv = dict(aux_deriv=np.array([0], dtype=np.int32))
        rc, fid = raw.create(**deriv)
        assert rc == -5 and fid == -1 and "flat" in raw.error()
        rc, fid = raw.create(seg_ptr=np.array([0, 2], dtype=np.int32), **deriv)      # the first two cells only
        assert rc == 0 and fid == 0, raw.error()
        rc, fid = raw.create()                                                        # no derivative: every cell
        assert rc == 0 and fid == 1, raw.error()
        # a derivative slot the code does not read binds nothing
        rc, fid = raw.create(n_aux=2, aux_deriv=np.array([-1, 1], dtype=np.int32))
        assert rc == 0 and fid == 2, raw.error()
    finally:
        lib.knp_destroy(ctx)      # frees the three plans that are left


# ------------------------------------------------------------------------------------------ EMI and whole runs
def test_emi_potential_norm():
    from cgx_hip.emi_models import g_syn
    from cgx_hip.emi_problem import ProblemEMI
    from cgx_hip.emi_solver import SolverEMI
    from cgx_hip.functionals import VolumeFunctional
    cfg = {"problem_type": "EMI", "dt": 5e-5, "time_steps": 2, "C_M": 0.02, "sigma_i": 0.7, "sigma_e": 1.3, "quiet": True,
           "cell_tag_file": "square8.xdmf", "facet_tag_file": "square8.xdmf", "mesh_conversion_factor": 1e-6,
           "ics_tags": [1], "ecs_tags": [2], "membrane_tags": [4]}
    p = ProblemEMI(cfg)
    p.add_ionic_model("HH", stim_fun=g_syn)
    p.init_ionic_model()
    s = SolverEMI(p)
    s.solve()
    ni, ne = s.potential_norms()
    assert ni > 0 and ne > 0
    got_i = p.assemble_scalar(integrand_i=p.wh[0] * p.wh[0])
    got_e = p.assemble_scalar(integrand_e=p.wh[1] * p.wh[1])
    assert isinstance(got_i, float)
    # positive integrands: sum |w f| is the integral itself
    print("EMI phi^2 against the squared norms:", abs(got_i / ni ** 2 - 1.0), abs(got_e / ne ** 2 - 1.0))
    assert abs(got_i - ni ** 2) <= TOL * ni ** 2 and abs(got_e - ne ** 2) <= TOL * ne ** 2
    # all functions of the EMI model are aux fields: potentials, phi_M and the gates
    F = VolumeFunctional(p, integrand_i=[p.phi_M * p.n, p.wh[0] * p.m], integrand_e=[p.wh[1], p.h])
    assert all(op != "KI" and op != "KE" for sp in F.spec.sides for op in _op_names(sp.spec))
    _, _, want, scale = functional_ref.reference(p, [p.phi_M * p.n, p.wh[0] * p.m], [p.wh[1], p.h])
    _check(F.value(), want, scale, "EMI aux fields")
    with pytest.raises(ValueError, match="other side"):
        p.assemble_scalar(integrand_i=p.wh[1])


def _op_names(spec):
    from cgx_hip._lib import OPS
    inv = {v: k for k, v in OPS.items()}
    return [inv[op] for op, _, _, _ in spec.code.tolist()]


def test_a_run_records_functionals(tmp_path):
    from cgx_hip import fem
    from cgx_hip.functionals import VolumeFunctional
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    cfg = ci_config(N=8, steps=3, rtol=1e-11)
    cfg["output_dir"] = str(tmp_path / "out") + "/"
    p = make_problem(cfg, "ci")
    p.solver_config["view_ksp"] = False
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    phi = [p.wh[k][p.N_ions] for k in range(2)]
    F = VolumeFunctional(p, [phi[0] * phi[0], fem.inner(fem.grad(phi[0]), fem.grad(phi[0]))],
                         [phi[1] * phi[1], fem.inner(fem.grad(phi[1]), fem.grad(phi[1]))])
    Q = VolumeFunctional(p, p.wh[0][0] - p.wh[0][2], p.wh[1][0] - p.wh[1][2])
    s.add_functional("potential", F)
    s.add_functional("charge", Q, interval=2)
    with pytest.raises(ValueError):
        s.add_functional("charge", Q)
    s.prepare()
    with pytest.raises(RuntimeError):
        s.add_functional("late", Q)
    first = F.value()
    for i in range(1, 4):
        s.step(i)
    s.finish()
    last, last_q = F.value(), Q.value()
    out = tmp_path / "out"
    rec, tags = np.load(out / "functional_potential.npy"), np.load(out / "functional_potential_tags.npy")
    assert rec.shape == (4, len(F.tags), 2) and tags.shape == (len(F.tags), 3)
    assert np.array_equal(tags[:, 0], F.tags) and np.array_equal(tags[:, 1], F.side) and np.array_equal(tags[:, 2], F.volume)
    assert rec[0].tobytes() == first.tobytes() and rec[-1].tobytes() == last.tobytes()
    assert np.all(rec[-1, :, 1] > 0) and not np.array_equal(rec[-1], rec[0])
    _, _, want, scale = functional_ref.reference(p, [phi[0] * phi[0], fem.inner(fem.grad(phi[0]), fem.grad(phi[0]))],
                                                 [phi[1] * phi[1], fem.inner(fem.grad(phi[1]), fem.grad(phi[1]))])
    _check(last, want, scale, "last record")
    rq = np.load(out / "functional_charge.npy")
    assert rq.shape == (2, len(Q.tags), 1) and np.load(out / "functional_charge_tags.npy").shape == (len(Q.tags), 3)      # steps 0 and 2
    assert np.all(np.isfinite(rq)) and last_q.shape == (len(Q.tags), 1)
