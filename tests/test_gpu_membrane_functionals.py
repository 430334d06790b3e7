"""Membrane functionals on the device (csrc/knp_membrane_functional.inc, cgx_hip/functionals.py): closed forms, the hard-wired
membrane reductions on the same fields, integrands against the NumPy reference (tests/membrane_functional_ref.py), a pooled row longer
than the wave combine, every error of the raw ABI, a flat adjacent cell, every instantiation of the two kinds' kernels, the two kinds'
plan tables side by side, the EMI model and a run that records functionals.

Tolerance throughout: |device - host| <= 1e-12 * sum |w f| per row and output (``functional_ref.TOL``), the bound of the volume
functionals: the same interpreter, the same reduction."""
import ctypes as C

import numpy as np
import pytest
import torch

import functional_ref
import membrane_functional_ref as mref
from functional_raw import RawMembrane as _Raw
from functional_raw import RawVolume as _RawVolume
from functional_raw import _f64, _i32
from functional_ref import TOL
from parity_utils import ci_config, make_problem, tissue_config
from test_gpu_functionals import _randomize

pytestmark = pytest.mark.gpu

CONFIGS = {"square": lambda: ci_config(N=8, steps=1), "cube": lambda: ci_config(N=8, steps=1, kind="cube"),
           "tissue2": lambda: tissue_config(2, 18, 3, steps=1), "tissue3": lambda: tissue_config(3, 12, 2, steps=1)}
CASES = list(CONFIGS)


@pytest.fixture(scope="module")
def problems():
    made = {}

    def get(case):
        if case not in made:
            p = make_problem(CONFIGS[case](), "ci")
            be = p.create_backend()
            made[case] = (p, be, _randomize(p, 41 + len(made)))
        return made[case]
    return get


def _check(got, want, scale, what):
    got, want, scale = (np.asarray(a, dtype=np.float64) for a in (got, want, scale))
    err = np.abs(got - want)
    print(f"{what}: max |device - host| / sum|w f| = {np.max(err / np.maximum(scale, 1e-300)):.3e}")
    assert got.shape == want.shape and np.all(np.isfinite(got))
    assert np.all(err <= TOL * scale), (what, err, TOL * scale)


def _normal(p, r="+"):
    from cgx_hip import fem
    return [c(r) for c in fem.FacetNormal(p.mesh)]


def _grad(f, r):
    from cgx_hip import fem
    return [g(r) for g in fem.grad(f)]


def _cells_of_membranes(p):
    """rows whose facets close around whole intracellular cells, and those cells' tags: the CI meshes have one membrane tag around
    their one cell tag, a tissue mesh tags every cell's membrane with the cell's own tag"""
    gt, it = [int(t) for t in p.gamma_tags], [int(t) for t in p.intra_tags]
    return ([tuple(gt)], [it]) if len(it) == 1 else ([(t,) for t in gt], [[t] for t in gt])


# ------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("case", CASES)
def test_integrand_one_gives_the_areas(problems, case):
    from cgx_hip.diagnostics import FacetGroupLayout
    from cgx_hip.functionals import MembraneFunctional
    p, be, _ = problems(case)
    F = MembraneFunctional(p, 1.0)
    lay = FacetGroupLayout(p, [(int(t),) for t in p.gamma_tags])
    assert np.array_equal(F.tags, lay.tags) and F.groups == lay.groups and F.n_out == 1
    v = F.value()
    assert v.shape == (len(lay.tags), 1) and np.all(lay.area > 0)
    _check(v[:, 0], lay.area, lay.area, "areas of the layout")
    _check(v[:, 0], F.area, F.area, "area attribute")
    assert F.total()[0] == pytest.approx(lay.area.sum(), rel=1e-12)
    assert p.assemble_scalar_membrane(1.0) == pytest.approx(lay.area.sum(), rel=1e-12)
    if len(lay.tags) > 2:      # pooled rows in the caller's order
        t = [int(x) for x in lay.tags]
        G = MembraneFunctional(p, 1.0, tags=[(t[2], t[0]), t[1]], degree=1)
        _check(G.value()[:, 0], [lay.area[2] + lay.area[0], lay.area[1]], G.area, "pooled areas")


@pytest.mark.parametrize("case", CASES)
def test_x_dot_n_gives_dim_times_the_cell_volume(problems, case):
    """the divergence theorem on a closed polyhedral membrane: the orientation of n('+')"""
    from cgx_hip import fem
    from cgx_hip.functionals import MembraneFunctional
    p, be, _ = problems(case)
    lm = p.local_mesh
    dim = lm.coords.shape[1]
    x = fem.SpatialCoordinate(p.mesh)
    groups, cell_tags = _cells_of_membranes(p)
    e = fem.inner(list(x), _normal(p))
    F = MembraneFunctional(p, [e, fem.inner(list(x), _normal(p, "-"))], tags=groups, degree=1)
    got = F.value()
    vol = functional_ref.cell_volumes(lm.coords[lm.cells])
    want = np.array([dim * vol[np.isin(lm.cell_tags, t)].sum() for t in cell_tags])
    _, _, scale = mref.reference(p, [e], tags=groups, degree=1)
    assert np.all(want > 0)
    _check(got[:, 0], want, scale[:, 0], "x . n('+') against dim * volume")
    _check(got[:, 1], -want, scale[:, 0], "x . n('-')")


@pytest.mark.parametrize("case", CASES)
def test_normal_derivatives_of_a_linear_function(problems, case):
    """a nodally linear f: grad f . n integrates to zero over a closed membrane, and the two sides' normal derivatives cancel"""
    from cgx_hip import fem
    from cgx_hip.functionals import MembraneFunctional
    p, be, _ = problems(case)
    lm = p.local_mesh
    dim = lm.coords.shape[1]
    rng = np.random.default_rng(3)
    a = rng.uniform(0.5, 1.5, dim) / np.ptp(lm.coords, axis=0).max()      # a . x of order one: f is linear to rounding
    lin = fem.Function(p.V, "lin")
    lin.x.array.copy_(torch.from_numpy(lm.coords @ a + 0.25).to(lin.x.array.device))
    groups, _ = _cells_of_membranes(p)
    dp, dm = fem.NormalDerivative(lin, "+"), fem.NormalDerivative(lin, "-")
    F = MembraneFunctional(p, [dp, dp + dm, fem.dot(_grad(lin, "+"), _normal(p, "-")) + dp], tags=groups, degree=1)
    got = F.value()
    _, want, scale = mref.reference(p, [dp, dm], tags=groups, degree=1)
    assert np.all(scale[:, 0] > 0)
    print("closed membrane: |int df/dn| / sum|w f| =", np.max(np.abs(got[:, 0]) / scale[:, 0]),
          " two sides:", np.max(np.abs(got[:, 1]) / (scale[:, 0] + scale[:, 1])))
    assert np.all(np.abs(got[:, 0]) <= TOL * scale[:, 0])
    assert np.all(np.abs(got[:, 1]) <= TOL * (scale[:, 0] + scale[:, 1]))
    assert np.all(np.abs(got[:, 2]) <= TOL * 2.0 * scale[:, 0])      # dot() with the other side's normal is the negative
    _check(got[:, 0], want[:, 0], scale[:, 0], "df/dn('+') against the reference")


# ------------------------------------------------------------------------------------------ the hard-wired kernels
@pytest.mark.parametrize("case", CASES)
def test_the_stimulus_expression_against_the_membrane_integral(problems, case):
    from cgx_hip.diagnostics import membrane_program
    from cgx_hip.functionals import MembraneFunctional
    p, be, _ = problems(case)
    group = tuple(int(t) for t in p.stimulus_tags)
    F = MembraneFunctional(p, p.stim_ufl_expr, tags=[group], degree=10)
    got = F.value()
    be.set_diag_program(membrane_program(p, p.stim_ufl_expr))
    be.set_facet_groups([group])
    hard = be.membrane_integral(torch.zeros(1, dtype=torch.float64, device=be.device)).cpu().numpy()
    _, want, scale = mref.reference(p, p.stim_ufl_expr, tags=[group], degree=10)
    assert got.shape == (1, 1) and abs(want[0, 0]) > 0
    _check(got[0], hard, scale[0], "stimulus current against knp_diag_membrane_integral")
    _check(got, want, scale, "stimulus current against the reference")


def _flux_forms(p):
    """the six forms of utils/calc_fluxes.py:88, unmasked, written with dot: per side three outputs"""
    from cgx_hip import fem
    forms = []
    for s, r in enumerate("+-"):
        phi = p.wh[s][p.N_ions]
        dphi = fem.dot(_grad(phi, r), _normal(p, r))
        forms.append([-ion["Di"] * (fem.dot(_grad(p.wh[s][j], r), _normal(p, r)) + (ion["z"] / p.psi) * p.wh[s][j] * dphi)
                      for j, ion in enumerate(p.ion_list)])
    return forms


@pytest.mark.parametrize("case", CASES)
def test_six_flux_integrands_against_the_flux_kernel(problems, case):
    from cgx_hip.functionals import MembraneFunctional
    p, be, _ = problems(case)
    forms = _flux_forms(p)
    hard = p.membrane_fluxes()
    for s, key in enumerate(("flux_i", "flux_e")):
        F = MembraneFunctional(p, forms[s])
        assert len(F.spec.spec.aux_functions) == 4 and sorted(F.spec.spec.aux_derivs) == [6 + s] * 4      # two slots per term, not nine
        got = F.value()
        tags, want, scale = mref.reference(p, forms[s])
        assert np.array_equal(tags, hard["tag"]) and np.abs(want).min() > 0
        _check(got, hard[key], scale, f"{key} against knp_diag_membrane_fluxes")
        _check(got, want, scale, f"{key} against the reference")


@pytest.mark.parametrize("case", CASES)
def test_phi_m_against_the_membrane_potential(problems, case):
    from cgx_hip.functionals import MembraneFunctional
    p, be, _ = problems(case)
    F = MembraneFunctional(p, p.phi_m_prev, degree=1)
    assert [op for op in _op_names(F.spec.spec) if op in ("PHIM", "AUX")] == ["PHIM"]
    got = F.value()[:, 0]
    hard = p.membrane_potential()
    _, _, scale = mref.reference(p, p.phi_m_prev, degree=1)
    assert np.array_equal(hard["tag"], F.tags)
    _check(got, hard["mean"] * hard["area"], scale[:, 0], "phi_m against mean x area of knp_diag_membrane_potential")


def _op_names(spec):
    from cgx_hip._lib import OPS
    inv = {v: k for k, v in OPS.items()}
    return [inv[op] for op, _, _, _ in spec.code.tolist()]


# ------------------------------------------------------------------------------------------ the NumPy reference
@pytest.mark.parametrize("case", CASES)
def test_the_channel_currents_of_the_three_ions(problems, case):
    from cgx_hip.functionals import MembraneFunctional
    p, be, _ = problems(case)
    tag = p.gamma_tags[0]
    outs = [p.ion_list[j]["I_ch"][tag] for j in range(3)]
    F = MembraneFunctional(p, outs)
    got = F.value()
    _, want, scale = mref.reference(p, outs)
    assert got.shape == (len(p.gamma_tags), 3) and np.abs(want).min() > 0
    _check(got, want, scale, "I_ch of Na, K, Cl")


@pytest.mark.parametrize("case", CASES)
def test_nonlinear_integrands_constants_and_rebound_functions(problems, case):
    from cgx_hip import fem
    from cgx_hip.functionals import MembraneFunctional
    p, be, user = problems(case)
    dim = p.local_mesh.coords.shape[1]
    x = fem.SpatialCoordinate(p.mesh)
    xc = float(p.local_mesh.coords[p._fv[:, 0], 0].mean())
    amp = fem.Constant(p.mesh, 0.25)
    n = _normal(p)
    phi_i, phi_e, ci, ce = p.wh[0][3], p.wh[1][3], p.wh[0][1], p.wh[1][2]
    h = float(p._fmeas.mean()) ** (1.0 / (dim - 1))      # a facet's length: derivatives times h are of the fields' order
    mix = (fem.exp(8.0 * phi_i) * fem.grad(user)[0]("-") * h + ce * fem.grad(ci)[dim - 1] * h * n[0]
           + fem.sqrt(abs(fem.grad(phi_e)[1]) * h + 1.0) * fem.grad(user)[dim - 1]("+") * h + user * p.phi_m_prev * ci / ce + n[dim - 1] ** 2)
    cond = amp * fem.conditional(fem.lt(x[0], xc), ci, -2.0 * ce) * phi_i ** 2
    F = MembraneFunctional(p, [mix, cond, amp * user], degree=6)
    modes = sorted(F.spec.spec.aux_derivs)
    assert len(modes) == 8 and modes[0] == -1 and {dim - 1, 3, 4, 8, 8 + dim - 1} <= set(modes)
    for value in (0.25, -1.75):
        amp.value = value
        _, want, scale = mref.reference(p, [mix, cond, amp * user], degree=6)
        got = F.value()
        assert np.abs(want).min() > 0
        _check(got, want, scale, f"nonlinear mix, conditional on x, amplitude {value}")
    assert abs(F.value()[0, 2] / want[0, 2] - 1.0) < 1e-9      # the second constant reached the device
    before = F.value()
    kept = user.x.array
    try:
        user.x.array = kept * 2.0                 # a new tensor; doubling is exact
        assert user.x.array.data_ptr() != kept.data_ptr()
        assert np.array_equal(F.value()[:, 2], 2.0 * before[:, 2])
        _, want, scale = mref.reference(p, [mix, cond, amp * user], degree=6)
        _check(F.value(), want, scale, "a Function bound to another tensor")
    finally:
        user.x.array = kept
    assert np.array_equal(F.value(), before)
    out = torch.full((len(F.tags), 3), 7.0, dtype=torch.float64, device=be.device)
    assert F(out=out).data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), before)
    F.close()
    with pytest.raises(Exception, match="closed"):
        F()


@pytest.fixture(scope="module")
def long_row():
    """tissue_config(3, 30, 5): 125 cells, a membrane tag each"""
    p = make_problem(tissue_config(3, 30, 5, steps=1), "ci")
    be = p.create_backend()
    return p, be, _randomize(p, 53)


def test_a_pooled_row_of_more_than_64_chunks(long_row):
    from cgx_hip import fem
    from cgx_hip.functionals import MembraneFunctional
    p, be, user = long_row
    tags = tuple(int(t) for t in p.gamma_tags)
    outs = [p.wh[0][0] * fem.ln(p.wh[1][1]) + fem.NormalDerivative(p.wh[0][3]) * float(p._fmeas.mean()) ** 0.5,
            fem.grad(user)[2]("-") * _normal(p)[1] + user]
    F = MembraneFunctional(p, outs, tags=[tags], degree=2)
    n = int(F.spec.seg_ptr[1])
    chunks = (n - 1) // 128 + 1
    print("pooled row:", n, "facets in", chunks, "chunks of 128")
    assert len(tags) == 125 and len(F.tags) == 1 and chunks > 64
    got = F.value()
    _, want, scale = mref.reference(p, outs, tags=[tags], degree=2)
    _check(got, want, scale, "long pooled row")
    assert F.value().tobytes() == got.tobytes()
    # every tag on its own stays with the wave combine and sums to the pooled row
    each = MembraneFunctional(p, outs, degree=2)
    assert np.all(np.diff(each.spec.seg_ptr) // 128 + 2 <= 64)
    _check(each.value().sum(axis=0), want[0], scale[0], "sum of the 125 rows")


# ------------------------------------------------------------------------------------------ the raw ABI
def test_every_error_of_the_raw_abi(problems):
    from cgx_hip import _lib
    from cgx_hip._lib import OPS
    p, be, user = problems("square")
    lib, ctx = be.lib, be.ctx
    ng, dim = len(p._fv), 2
    raw = _Raw(be, ng, dim)
    E_ARG = -1
    code = raw.args["code"]

    def prog(*rows):
        return dict(code=np.array(rows, dtype=np.int32), n_instr=len(rows))
    mode = lambda m: dict(aux_mode=np.array([m], dtype=np.int32))
    bad = {
        "null id": dict(id=False), "null q_pts": dict(q_pts=None), "null q_w": dict(q_w=None), "null code": dict(code=None),
        "null consts": dict(n_consts=1, consts=None), "null aux_mode": dict(aux_mode=None), "null seg_ptr": dict(seg_ptr=None),
        "null facets": dict(facets=None),
        "n_q 0": dict(n_q=0), "n_q 126": dict(n_q=_lib.KNP_FUNCTIONAL_MAX_Q + 1, q_pts=np.zeros((126, 2)), q_w=np.full(126, 1 / 126)),
        "n_out 0": dict(n_out=0), "n_out 4": dict(n_out=4),
        "n_aux -1": dict(n_aux=-1), "n_aux 9": dict(n_aux=_lib.KNP_MAX_AUX + 1, aux_mode=np.full(9, -1, dtype=np.int32)),
        "mode -2": mode(-2), "mode 11": mode(11), "d/dz on the + cell in 2D": mode(2), "d/dz on the - cell in 2D": mode(5),
        "n_z in 2D": mode(10),
        "empty program": dict(n_instr=0),
        "unknown opcode": prog([99, 0, 0, 0], code[2]), "register 48": prog([OPS["AUX"], _lib.KNP_MAX_PROG_REGS, 0, 0], code[2]),
        "constant out of range": prog([OPS["CONST"], 0, 0, 0], [OPS["OUT"], 0, 0, 0]),
        "coordinate axis = dim": prog([OPS["X"], 0, dim, 0], [OPS["OUT"], 0, 0, 0]),
        "OUT index = n_out": prog(code[0], [OPS["OUT"], 0, 1, 0]), "aux slot = n_aux": prog([OPS["AUX"], 0, 1, 0], [OPS["OUT"], 0, 0, 0]),
        "65 constants": dict(n_consts=_lib.KNP_DIAG_MAX_CONSTS + 1, consts=np.zeros(65)), "negative constants": dict(n_consts=-1),
        "facet out of range": dict(facets=np.r_[np.arange(ng - 1), ng].astype(np.int32)),
        "negative facet": dict(facets=np.r_[np.arange(ng - 1), -1].astype(np.int32)),
        "facet listed twice": dict(facets=np.r_[np.arange(ng - 1), 0].astype(np.int32)),
        "seg_ptr[0] != 0": dict(seg_ptr=np.array([1, ng], dtype=np.int32)),
        "seg_ptr decreases": dict(n_tags=2, seg_ptr=np.array([0, 5, 3], dtype=np.int32)),
        "seg_ptr past the facets": dict(seg_ptr=np.array([0, ng + 1], dtype=np.int32), facets=np.arange(ng + 1, dtype=np.int32)),
        "negative n_tags": dict(n_tags=-1),
    }
    seen = set()
    for what, kw in bad.items():
        rc, fid = raw.create(**kw)
        msg = raw.error()
        assert rc == E_ARG and fid == -1 and msg, (what, rc, fid, msg)
        seen.add(msg)
    assert len(seen) >= 12      # the messages tell the causes apart
    # no plan was half-made: the first valid create takes slot 0; the ids are apart from the volume functionals'
    rc, fid = raw.create()
    assert rc == 0 and fid == 0, raw.error()
    # slot 0 the value, slot 1 d/dn on the extracellular cell, slot 2 a normal component: OUT = aux0 * aux1 * aux2
    rc, second = raw.create(n_aux=3, aux_mode=np.array([-1, 7, 9], dtype=np.int32),
                            **prog(code[0], [OPS["AUX"], 1, 1, 0], [OPS["AUX"], 2, 2, 0], [OPS["MUL"], 3, 0, 1], [OPS["MUL"], 3, 3, 2],
                                   [OPS["OUT"], 0, 0, 3]))
    assert rc == 0 and second == 1, raw.error()
    sentinel = -123.25
    out = torch.full((1,), sentinel, dtype=torch.float64, device=be.device)
    optr = C.c_void_p(out.data_ptr())
    f = _lib.Fields()
    one = np.ones(1)

    def refused(rc, what):
        assert rc == E_ARG and raw.error(), (what, rc)
        torch.cuda.synchronize()
        assert float(out[0]) == sentinel, what      # nothing was launched
    refused(lib.knp_membrane_functional_eval(ctx, fid, C.byref(f), optr), "the aux field the code reads is null")
    refused(lib.knp_membrane_functional_eval(ctx, fid, None, optr), "null fields")
    refused(lib.knp_membrane_functional_eval(ctx, 7, C.byref(f), optr), "unknown id")
    refused(lib.knp_membrane_functional_eval(ctx, -1, C.byref(f), optr), "negative id")
    phi = p.wh[0][3]
    f.aux[0] = phi.data_ptr()
    refused(lib.knp_membrane_functional_eval(ctx, fid, C.byref(f), None), "null out")
    refused(lib.knp_membrane_functional_eval(ctx, second, C.byref(f), optr), "the second aux field is null")
    refused(lib.knp_membrane_functional_set_constants(ctx, fid, 1, _f64(one)), "constant count mismatch")
    refused(lib.knp_membrane_functional_set_constants(ctx, 7, 0, None), "unknown id")
    refused(lib.knp_membrane_functional_destroy(ctx, 7), "unknown id")
    assert lib.knp_membrane_functional_eval(ctx, fid, C.byref(f), optr) == 0, raw.error()      # concentrations and phi_m null: not read
    lm = p.local_mesh
    fv = np.asarray(p._fv)
    opp = mref.opposite_vertices(np.asarray(lm.cells), np.asarray(lm.gamma), fv)
    qp, qw = raw.args["q_pts"], raw.args["q_w"]
    (want, scale), = mref.integrate_facets(lm.coords, fv, opp, p._fmeas, [phi * phi], qp, qw)
    assert abs(float(out[0]) - want) <= TOL * scale
    f.aux[1] = user.data_ptr()      # the normal's slot 2 needs no pointer
    assert lib.knp_membrane_functional_eval(ctx, second, C.byref(f), optr) == 0, raw.error()
    from cgx_hip import fem
    e = phi * fem.NormalDerivative(user, "-") * fem.FacetNormal(p.mesh)[1]("+")
    (want, scale), = mref.integrate_facets(lm.coords, fv, opp, p._fmeas, [e], qp, qw)
    assert abs(want) > 0 and abs(float(out[0]) - want) <= TOL * scale
    assert lib.knp_membrane_functional_destroy(ctx, fid) == 0
    out.fill_(sentinel)
    refused(lib.knp_membrane_functional_eval(ctx, fid, C.byref(f), optr), "destroyed id")
    rc, again = raw.create()
    assert rc == 0 and again == fid      # the slot is reused
    rc, empty = raw.create(n_tags=0, seg_ptr=None, facets=None)      # n_tags == 0 is a successful no-op
    assert rc == 0 and empty == 2, raw.error()
    assert lib.knp_membrane_functional_eval(ctx, empty, C.byref(f), optr) == 0
    torch.cuda.synchronize()
    assert float(out[0]) == sentinel
    for k in (again, second, empty):
        assert lib.knp_membrane_functional_destroy(ctx, k) == 0


def test_a_flat_adjacent_cell_with_a_bound_derivative_is_a_mesh_error():
    """A hand-made mesh of two triangles on the edge (1, 2): the extracellular one is 1e-310 high, so its determinant is not zero and
    the context builds, but the gradients of its barycentric coordinates overflow.  A functional that binds a derivative on that
    cell refuses the facet; one that reads values, the intracellular cell's derivatives or the normal takes it."""
    from cgx_hip import _lib
    lib = _lib.load()
    torch.cuda.current_device()
    coords = np.array([[0.5, 1.0], [0.0, 0.0], [1.0, 0.0], [0.5, -1e-310]])
    cells = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)
    side = np.array([0, 1], dtype=np.uint8)
    gamma = np.array([[0, 0, 1, 1]], dtype=np.int32)
    gprog = np.zeros(1, dtype=np.int32)
    qp, qw = np.array([[0.5, 0.5]]), np.array([1.0])
    assert 0.0 < -coords[3, 1] < 1.0 / np.finfo(np.float64).max      # its reciprocal overflows
    d = _lib.MeshDesc()
    d.dim, d.n_vertices, d.n_vertices_owned, d.n_cells, d.n_cells_owned = 2, 4, 4, 2, 2
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
        raw = _Raw(be, 1, 2)
        mode = lambda m: dict(aux_mode=np.array([m], dtype=np.int32))
        for m in (3, 4, 7):      # d/dx, d/dy, d/dn on the extracellular cell
            rc, fid = raw.create(**mode(m))
            assert rc == -5 and fid == -1 and "flat" in raw.error(), (m, rc, raw.error())
        for k, m in enumerate((-1, 0, 1, 6, 8, 9)):      # the value, the intracellular cell, the normal
            rc, fid = raw.create(**mode(m))
            assert rc == 0 and fid == k, (m, raw.error())
        # a slot of the flat cell that the code does not read binds nothing
        rc, fid = raw.create(n_aux=2, aux_mode=np.array([-1, 3], dtype=np.int32))
        assert rc == 0 and fid == 6, raw.error()
    finally:
        lib.knp_destroy(ctx)      # frees the plans that are left


def test_an_extracellular_cell_that_does_not_hold_the_facet_is_a_mesh_error():
    """A hand-made mesh whose membrane entry names an extracellular cell away from the facet: the context builds (the graph finds
    no opposite vertex there), a functional that reads that cell refuses the facet, one that reads the intracellular cell takes it"""
    from cgx_hip import _lib
    lib = _lib.load()
    torch.cuda.current_device()
    coords = np.array([[0.5, 1.0], [0.0, 0.0], [1.0, 0.0], [0.5, -1.0], [2.0, -1.0], [2.0, 0.0]])
    cells = np.array([[0, 1, 2], [1, 3, 2], [3, 4, 5]], dtype=np.int32)
    side = np.array([0, 1, 1], dtype=np.uint8)
    gamma = np.array([[0, 0, 2, 0]], dtype=np.int32)
    gprog = np.zeros(1, dtype=np.int32)
    qp, qw = np.array([[0.5, 0.5]]), np.array([1.0])
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
        raw = _Raw(be, 1, 2)
        mode = lambda m: dict(aux_mode=np.array([m], dtype=np.int32))
        for m in (3, 4, 7):
            rc, fid = raw.create(**mode(m))
            assert rc == -5 and fid == -1 and "does not hold" in raw.error(), (m, rc, raw.error())
        for k, m in enumerate((-1, 0, 1, 6, 8, 9)):
            rc, fid = raw.create(**mode(m))
            assert rc == 0 and fid == k, (m, raw.error())
    finally:
        lib.knp_destroy(ctx)


# ------------------------------------------------------------------------------------------ both kinds, every kernel
def _facet_length(p):
    return float(p._fmeas.mean()) ** (1.0 / (p.local_mesh.coords.shape[1] - 1))


def _mixed_volume_forms(p, user, n_out):
    """per side ``n_out`` outputs, each a concentration (KI / KE), a nonlinear term of the potential (an aux value) and a derivative
    slot, the axis moving with the output"""
    from cgx_hip import fem
    dim, h = p.local_mesh.coords.shape[1], _facet_length(p)
    return [[p.wh[s][j] + fem.exp(8.0 * p.wh[s][p.N_ions]) * fem.grad(user)[(j + 1) % dim] * h for j in range(n_out)] for s in range(2)]


def _mixed_membrane_outs(p, user, n_out):
    """``n_out`` outputs, each a concentration, a nonlinear term of the potential times a '+' gradient of the user's field, and a
    '-' normal derivative"""
    from cgx_hip import fem
    dim, h = p.local_mesh.coords.shape[1], _facet_length(p)
    return [p.wh[0][j] + fem.exp(8.0 * p.wh[0][p.N_ions]) * fem.grad(user)[(j + 1) % dim]("+") * h
            + fem.sqrt(p.wh[1][j]) * fem.NormalDerivative(user, "-") * h for j in range(n_out)]


@pytest.mark.parametrize("n_out", [1, 2, 3])
@pytest.mark.parametrize("case", ["square", "cube"])
def test_every_instantiation_of_both_kernels(problems, case, n_out):
    """k_functional and k_membrane_functional over <2 | 3, 1 | 2 | 3>, each named here and not reached by the way"""
    from cgx_hip.functionals import MembraneFunctional, VolumeFunctional
    p, be, user = problems(case)
    forms = _mixed_volume_forms(p, user, n_out)
    V = VolumeFunctional(p, forms[0], forms[1], degree=2)
    assert V.n_out == n_out and all(-1 in sp.spec.aux_derivs and max(sp.spec.aux_derivs) >= 0 for sp in V.spec.sides)
    _, _, want, scale = functional_ref.reference(p, forms[0], forms[1], degree=2)
    assert want.shape == (len(V.tags), n_out) and np.all(scale > 0)
    _check(V.value(), want, scale, f"volume kernel <{p.local_mesh.coords.shape[1]}, {n_out}>")
    outs = _mixed_membrane_outs(p, user, n_out)
    M = MembraneFunctional(p, outs, degree=2)
    modes = set(M.spec.spec.aux_derivs)
    assert M.n_out == n_out and -1 in modes and 7 in modes and modes & {0, 1, 2}
    _, want, scale = mref.reference(p, outs, degree=2)
    assert want.shape == (len(M.tags), n_out) and np.all(scale > 0)
    _check(M.value(), want, scale, f"membrane kernel <{p.local_mesh.coords.shape[1]}, {n_out}>")


def test_two_plan_tables_one_lifecycle():
    """The two kinds keep their plans apart: each kind's first plan has id 0, destroying one kind's plan leaves the other kind's plan
    of the same id as it was, the destroyed id is unknown to its own kind only, and its slot is taken again."""
    from cgx_hip import _lib
    p = make_problem(ci_config(N=8, steps=1), "ci")
    be = p.create_backend()
    _randomize(p, 67)
    lib, ctx = be.lib, be.ctx
    kinds = {"volume": (_RawVolume(be, int(p.local_mesh.n_cells_owned), 2), lib.knp_functional_eval, lib.knp_functional_destroy,
                        "unknown functional 0"),
             "membrane": (_Raw(be, len(p._fv), 2), lib.knp_membrane_functional_eval, lib.knp_membrane_functional_destroy,
                          "unknown membrane functional 0")}
    f = _lib.Fields()
    f.aux[0] = p.wh[0][3].data_ptr()
    sentinel = -123.25

    def evaluate(kind):
        out = torch.full((1,), sentinel, dtype=torch.float64, device=be.device)
        rc = kinds[kind][1](ctx, 0, C.byref(f), C.c_void_p(out.data_ptr()))
        torch.cuda.synchronize()
        return rc, out.cpu().numpy()

    for gone, stays in (("volume", "membrane"), ("membrane", "volume")):
        for kind in (gone, stays):
            rc, fid = kinds[kind][0].create()
            assert rc == 0 and fid == 0, (kind, kinds[kind][0].error())
        before = {}
        for kind in (gone, stays):
            rc, before[kind] = evaluate(kind)
            assert rc == 0 and before[kind][0] != sentinel and np.isfinite(before[kind][0]), (kind, kinds[kind][0].error())
        assert before["volume"][0] != before["membrane"][0]
        raw, _, destroy, unknown = kinds[gone]
        assert destroy(ctx, 0) == 0, raw.error()
        rc, after = evaluate(stays)
        assert rc == 0 and after.tobytes() == before[stays].tobytes(), (stays, kinds[stays][0].error())
        rc, untouched = evaluate(gone)
        assert rc == -1 and raw.error() == unknown and untouched[0] == sentinel      # nothing was launched
        rc, fid = raw.create()
        assert rc == 0 and fid == 0, raw.error()
        rc, again = evaluate(gone)
        assert rc == 0 and again.tobytes() == before[gone].tobytes()
        for kind in (gone, stays):
            assert kinds[kind][2](ctx, 0) == 0, kinds[kind][0].error()


# ------------------------------------------------------------------------------------------ EMI and whole runs
def test_emi_transmembrane_current():
    """int -sigma_i d phi_i / dn dS on square8 after two steps, every Function an aux field"""
    from cgx_hip import fem
    from cgx_hip.emi_models import g_syn
    from cgx_hip.emi_problem import ProblemEMI
    from cgx_hip.emi_solver import SolverEMI
    from cgx_hip.functionals import MembraneFunctional
    cfg = {"problem_type": "EMI", "dt": 5e-5, "time_steps": 2, "C_M": 0.02, "sigma_i": 0.7, "sigma_e": 1.3, "quiet": True,
           "cell_tag_file": "square8.xdmf", "facet_tag_file": "square8.xdmf", "mesh_conversion_factor": 1e-6,
           "ics_tags": [1], "ecs_tags": [2], "membrane_tags": [4]}
    p = ProblemEMI(cfg)
    p.add_ionic_model("HH", stim_fun=g_syn)
    p.init_ionic_model()
    s = SolverEMI(p)
    s.solve()
    n = _normal(p)
    outs = [-p.sigma_i * fem.dot(_grad(p.wh[0], "+"), n), -p.sigma_e * fem.NormalDerivative(p.wh[1]), p.phi_M * p.n + (p.wh[0] - p.wh[1])]
    F = MembraneFunctional(p, outs)
    assert all(op not in ("KI", "KE", "PHIM") for op in _op_names(F.spec.spec))
    assert sorted(F.spec.spec.aux_derivs) == [-1, -1, -1, -1, 6, 7]
    got = F.value()
    _, want, scale = mref.reference(p, outs)
    assert got.shape == (1, 3) and np.abs(want).min() > 0
    _check(got, want, scale, "EMI trans-membrane current")
    tot = p.assemble_scalar_membrane(outs[0])
    assert isinstance(tot, float) and abs(tot - want[0, 0]) <= TOL * scale[0, 0]
    with pytest.raises(ValueError, match="intracellular side"):
        p.assemble_scalar_membrane(fem.NormalDerivative(p.wh[0], "-"))


def test_a_run_records_a_volume_and_a_membrane_functional(tmp_path):
    from cgx_hip import fem
    from cgx_hip.functionals import MembraneFunctional, VolumeFunctional
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    cfg = ci_config(N=8, steps=3, rtol=1e-11)
    cfg["output_dir"] = str(tmp_path / "out") + "/"
    p = make_problem(cfg, "ci")
    p.solver_config["view_ksp"] = False
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    phi = [p.wh[k][p.N_ions] for k in range(2)]
    V = VolumeFunctional(p, phi[0] * phi[0], phi[1] * phi[1])
    outs = [p.ion_list[0]["I_ch"][p.gamma_tags[0]], -p.ion_list[1]["Di"] * fem.NormalDerivative(p.wh[0][1])]
    M = MembraneFunctional(p, outs)
    s.add_functional("norms", V)
    s.add_functional("membrane", M, interval=2)
    with pytest.raises(ValueError):
        s.add_functional("membrane", M)
    with pytest.raises(ValueError):
        s.add_functional("other", object())
    s.prepare()
    first = M.value()
    for i in range(1, 4):
        s.step(i)
    s.finish()
    last = M.value()
    out = tmp_path / "out"
    rec, tags = np.load(out / "functional_membrane.npy"), np.load(out / "functional_membrane_tags.npy")
    assert rec.shape == (2, len(M.tags), 2) and tags.shape == (len(M.tags), 3)      # steps 0 and 2
    assert np.array_equal(tags[:, 0], M.tags) and np.all(tags[:, 1] == 2) and np.array_equal(tags[:, 2], M.area)
    assert rec[0].tobytes() == first.tobytes() and np.all(np.isfinite(rec)) and not np.array_equal(rec[1], rec[0])
    _, want, scale = mref.reference(p, outs)
    _check(last, want, scale, "after the last step")
    rv, tv = np.load(out / "functional_norms.npy"), np.load(out / "functional_norms_tags.npy")
    assert rv.shape == (4, len(V.tags), 1) and np.array_equal(tv[:, 1], V.side) and np.array_equal(tv[:, 2], V.volume)
