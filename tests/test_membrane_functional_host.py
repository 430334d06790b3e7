"""Host side of the membrane functionals (cgx_hip/functionals.py, cgx_hip/fem.py): how integrands compile -- roles, slot modes,
default sides, ``dot`` --, every ``ValueError`` of ``compile_membrane_functional``, what stays as it was for the other programs, and
the NumPy reference (tests/membrane_functional_ref.py) on single hand-made facets.  No device."""
import math

import numpy as np
import pytest

import membrane_functional_ref as mref
from parity_utils import ci_config, make_problem, tissue_config


@pytest.fixture(scope="module")
def problem():
    return make_problem(ci_config(N=8, steps=1), "ci")


@pytest.fixture(scope="module")
def tissue():
    """nine cells, a membrane tag each"""
    return make_problem(tissue_config(2, 18, 3, steps=1), "ci")


def _ops(spec):
    from cgx_hip._lib import OPS
    inv = {v: k for k, v in OPS.items()}
    return [(inv[op], a) for op, _, a, _ in spec.code.tolist() if inv[op] in ("KI", "KE", "PHIM", "AUX", "X", "OUT")]


def _bound(prog):
    return [(None if f is None else f.name, m) for f, m in zip(prog.aux_functions, prog.aux_derivs)]


def test_roles_and_slot_modes(problem, tissue):
    from cgx_hip import fem
    from cgx_hip.functionals import compile_membrane_functional
    p = problem
    user = fem.Function(p.V, "user")
    n = fem.FacetNormal(p.mesh)
    phi_i, phi_e = p.wh[0][3], p.wh[1][3]
    spec = compile_membrane_functional(p, [p.wh[0][0] * p.wh[1][1] * p.phi_m_prev,
                                           fem.grad(phi_i)[1] + fem.grad(phi_e)[0] + fem.grad(user)[0]("-") + fem.grad(user)[0]("+") + user,
                                           fem.NormalDerivative(phi_i) + fem.NormalDerivative(user, "-") + n[1]("-") * n[1]("+")])
    prog = spec.spec
    assert spec.n_out == 3 and not spec.single and spec.degree == 10
    ops = _ops(prog)
    assert ("KI", 0) in ops and ("KE", 1) in ops and ("PHIM", 0) in ops and [o for o in ops if o[0] == "OUT"] == [("OUT", 0), ("OUT", 1), ("OUT", 2)]
    # default sides: phi_i on '+' (axis 1 -> 1), phi_e on '-' (axis 0 -> 3); the user function as restricted; one normal slot for both signs
    assert _bound(prog) == [(phi_i.name, 1), (phi_e.name, 3), ("user", 3), ("user", 0), ("user", -1), (phi_i.name, 6), ("user", 7), (None, 9)]
    assert prog.aux_functions[0] is phi_i and prog.aux_functions[-1] is None
    assert sum(1 for o in ops if o[0] == "AUX") == 8
    # the rule is the problem's own at the default degree; rows: every membrane tag on its own
    assert np.array_equal(spec.q_pts, p.q_pts) and np.array_equal(spec.q_w, p.q_w)
    assert list(spec.tags) == [int(t) for t in p.gamma_tags] and spec.groups == tuple((int(t),) for t in p.gamma_tags)
    assert np.array_equal(np.sort(spec.facets), np.arange(len(p._fv))) and spec.area.sum() == pytest.approx(p._fmeas.sum(), rel=1e-14)
    # pooled tags, in the caller's order
    t = [int(x) for x in tissue.gamma_tags]
    each = compile_membrane_functional(tissue, 1.0)
    assert len(t) == 9 and list(each.tags) == t and np.all(each.area > 0)
    pooled = compile_membrane_functional(tissue, 1.0, tags=[(t[2], t[0]), t[1]], degree=3)
    assert pooled.single and pooled.groups == ((t[2], t[0]), (t[1],)) and list(pooled.tags) == [t[2], t[1]]
    assert pooled.q_w.shape == (2,) and pooled.area[0] == pytest.approx(each.area[0] + each.area[2], rel=1e-14)
    assert np.all(np.isin(np.asarray(tissue.gamma_facet_tags)[pooled.facets[:pooled.seg_ptr[1]]], [t[0], t[2]]))
    # a restriction the function's side agrees with changes nothing
    same = compile_membrane_functional(p, fem.grad(phi_i)[1]("+") + fem.NormalDerivative(phi_e, "-"))
    assert _bound(same.spec) == [(phi_i.name, 1), (phi_e.name, 7)]
    # a Function's value needs no restriction, whichever side it lives on; phi_i and phi_e take aux slots, concentrations none
    val = compile_membrane_functional(p, phi_i * phi_e * p.wh[0][1] * p.wh[1][2] * user)
    assert _bound(val.spec) == [(phi_i.name, -1), (phi_e.name, -1), ("user", -1)]


def test_value_errors(problem, tissue):
    from cgx_hip import fem
    from cgx_hip._lib import KNP_MAX_AUX
    from cgx_hip.functionals import compile_membrane_functional as cmf
    p = problem
    user = fem.Function(p.V, "user")
    n = fem.FacetNormal(p.mesh)
    t = [int(x) for x in tissue.gamma_tags]
    with pytest.raises(ValueError, match="'user'.*must be restricted"):
        cmf(p, fem.grad(user)[0])
    with pytest.raises(ValueError, match="'user'.*must be restricted"):
        cmf(p, fem.NormalDerivative(user))
    with pytest.raises(ValueError, match="'phi_m'.*must be restricted"):
        cmf(p, fem.grad(p.phi_m_prev)[1])
    with pytest.raises(ValueError, match="normal must be restricted"):
        cmf(p, n[0])
    with pytest.raises(ValueError, match="intracellular side"):
        cmf(p, fem.grad(p.wh[0][3])[0]("-"))
    with pytest.raises(ValueError, match="extracellular side"):
        cmf(p, fem.NormalDerivative(p.wh[1][0], "+"))
    with pytest.raises(ValueError, match="restriction is"):
        fem.grad(user)[0]("i")
    with pytest.raises(ValueError, match="restriction is"):
        fem.NormalDerivative(user, 0)
    with pytest.raises(ValueError, match="up to 3"):
        cmf(p, [user] * 4)
    with pytest.raises(ValueError, match="up to 3"):
        cmf(p, [])
    with pytest.raises(ValueError, match="listed twice"):
        cmf(tissue, 1.0, tags=[t[0], t[0]])
    with pytest.raises(ValueError, match="listed twice"):
        cmf(tissue, 1.0, tags=[(t[0], t[1]), t[1]])
    with pytest.raises(ValueError, match="unknown membrane tag"):
        cmf(tissue, 1.0, tags=[t[0], 987654])
    with pytest.raises(ValueError, match="empty group"):
        cmf(p, user, tags=[()])
    users = [fem.Function(p.V, f"u{k}") for k in range(KNP_MAX_AUX + 1)]
    total = users[0]
    for u in users[1:]:
        total = total + u
    with pytest.raises(ValueError, match="aux slots"):
        cmf(p, total)
    # dim components of a gradient and dim of the normal fill slots that dot() saves
    five = fem.inner([g("+") for g in fem.grad(user)], [c("+") for c in n])
    for u in users[:5]:
        five = five + fem.inner([g("-") for g in fem.grad(u)], [c("+") for c in n])
    with pytest.raises(ValueError, match="aux slots"):
        cmf(p, five)
    # 2D facets: degree // 2 + 1 points; 3D: its square
    assert cmf(p, user, degree=248).q_w.shape == (125,)
    with pytest.raises(ValueError, match="quadrature points"):
        cmf(p, user, degree=250)
    with pytest.raises(ValueError, match="degree"):
        cmf(p, user, degree=-1)
    p3 = make_problem(ci_config(N=4, steps=1, kind="cube"), "ci")
    assert cmf(p3, p3.wh[0][0], degree=21).q_w.shape == (121,) and cmf(p3, p3.wh[0][0]).q_pts.shape == (36, 3)
    with pytest.raises(ValueError, match="quadrature points"):
        cmf(p3, p3.wh[0][0], degree=22)


def test_dot_folds_a_restricted_gradient_and_normal_into_one_slot(problem):
    from cgx_hip import fem
    from cgx_hip.functionals import compile_membrane_functional as cmf
    p = problem
    user = fem.Function(p.V, "user")
    n = fem.FacetNormal(p.mesh)
    N = lambda r: [c(r) for c in n]
    gr = lambda f, r: [g(r) for g in fem.grad(f)]
    d = fem.dot(gr(user, "+"), N("+"))
    assert isinstance(d, fem.NormalDerivative) and d.function is user and d.side == "+"
    d = fem.dot(N("-"), gr(user, "-"))
    assert isinstance(d, fem.NormalDerivative) and d.side == "-"
    for r, rn in (("+", "-"), ("-", "+")):
        d = fem.dot(gr(user, r), N(rn))
        assert isinstance(d, fem.Op) and d.op == "NEG" and isinstance(d.args[0], fem.NormalDerivative) and d.args[0].side == r
    # no fold: unrestricted parts, axes out of order, two functions, one component short
    other = fem.Function(p.V, "other")
    g = gr(user, "+")
    for a, b in ((fem.grad(user), N("+")), (g, n), (g[::-1], N("+")), ([g[0], gr(other, "+")[1]], N("+")), ([g[0], g[1]("-")], N("+")),
                 (g, [n[0]("+"), n[1]("-")]), (g[:1], N("+")[:1])):
        assert not isinstance(fem.dot(a, b), fem.NormalDerivative) and fem.dot(a, b).op in ("ADD", "MUL")
    assert fem.dot(2.0, user).op == "MUL"
    # the flux of utils/calc_fluxes.py binds two slots per side, not nine
    flux = []
    for s, r in enumerate("+-"):
        c, phi = p.wh[s][0], p.wh[s][3]
        flux.append(-1.3e-9 * (fem.dot(gr(c, r), N(r)) + 37.0 * c * fem.dot(gr(phi, r), N(r))))
    spec = cmf(p, flux)
    assert _bound(spec.spec) == [(p.wh[0][0].name, 6), (p.wh[0][3].name, 6), (p.wh[1][0].name, 7), (p.wh[1][3].name, 7)]
    wide = cmf(p, -1.3e-9 * (fem.inner(gr(p.wh[0][0], "+"), N("+")) + 37.0 * p.wh[0][0] * fem.inner(gr(p.wh[0][3], "+"), N("+"))))
    assert len(wide.spec.aux_functions) == 6


def test_the_other_programs_are_as_before(problem):
    from cgx_hip import fem
    from cgx_hip.functionals import compile_functional
    p = problem
    u, v = p.wh[0][0], p.wh[0][3]
    n = fem.FacetNormal(p.mesh)
    # inner on its old inputs
    e = fem.inner(fem.grad(u), fem.grad(v))
    assert e.op == "ADD" and all(a.op == "MUL" for a in e.args) and isinstance(e.args[0].args[0], fem.Derivative)
    assert e.args[0].args[0].side is None and fem.inner(2.0, v).op == "MUL"
    with pytest.raises(ValueError):
        fem.inner(fem.grad(u), [fem.grad(u)[0]])
    # every other node still ignores a restriction
    assert v("+") is v and (u * v)("-").op == "MUL" and fem.Constant(p.mesh, 1.0)("+").value == 1.0
    # compile_program without aux_derivs refuses all three new nodes as it refuses a Derivative, and membrane programs with them
    for node in (fem.grad(v)[0], fem.grad(v)[0]("+"), n[0]("+"), fem.NormalDerivative(v, "+")):
        with pytest.raises(TypeError):
            fem.compile_program([node], {})
        with pytest.raises(TypeError):
            fem.compile_program([node * 2.0], {}, [])
    aux, der = [], []
    spec = fem.compile_program([fem.grad(v)[1], fem.grad(v)[1]("-")], {}, aux, der)
    assert aux == [v] and der == [1] and spec.aux_derivs is der      # the restriction is ignored: one slot
    # a volume functional ignores a restricted Derivative and refuses a normal and a normal derivative
    plain = compile_functional(p, integrand_i=fem.inner(fem.grad(u), fem.grad(v)))
    restricted = compile_functional(p, integrand_i=fem.inner([g("-") for g in fem.grad(u)], [g("+") for g in fem.grad(v)]))
    assert np.array_equal(plain.sides[0].spec.code, restricted.sides[0].spec.code)
    assert plain.sides[0].spec.aux_derivs == restricted.sides[0].spec.aux_derivs
    with pytest.raises(ValueError, match="membrane facets only"):
        compile_functional(p, integrand_i=n[0]("+") * u)
    with pytest.raises(ValueError, match="membrane facets only"):
        compile_functional(p, integrand_i=fem.NormalDerivative(v, "+"))
    with pytest.raises(ValueError, match="other side"):
        compile_functional(p, integrand_e=fem.NormalDerivative(v, "+"))


class _Nodal:
    """a Function of a hand-made mesh: nodal values on the host only"""

    def __new__(cls, values, name="nodal"):
        from cgx_hip import fem

        class Nodal(fem.Function):
            def __init__(self, v, nm):
                self._v = np.asarray(v, dtype=np.float64)
                self.name = nm

            def numpy(self):
                return self._v
        return Nodal(values, name)


@pytest.mark.parametrize("dim", [2, 3])
def test_the_reference_on_one_hand_made_facet(dim):
    """One facet between two skewed simplices.  int_F prod lambda_a^{k_a} = (d-1)! |F| prod k_a! / (d - 1 + sum k_a)! at the degree
    of the monomial; the gradients of a linear function are its coefficients on both sides, the normal is the unit vector
    orthogonal to the facet that points away from the intracellular cell's opposite vertex."""
    from cgx_hip import fem
    from cgx_hip.mesh import facet_quadrature
    rng = np.random.default_rng(7 + dim)
    # facet vertices 0..d-1 near the plane x_last = 0, the intracellular opposite vertex above it, the extracellular one below
    coords = np.zeros((dim + 2, dim))
    coords[:dim, :dim - 1] = rng.uniform(-1.0, 1.0, (dim, dim - 1)) + 2.0 * np.eye(dim)[:, :dim - 1]
    coords[:dim, dim - 1] = rng.uniform(-0.2, 0.2, dim)
    coords[dim] = np.r_[rng.uniform(-0.5, 0.5, dim - 1), 1.3]
    coords[dim + 1] = np.r_[rng.uniform(-0.5, 0.5, dim - 1), -0.9]
    fv = np.arange(dim)[None, :]
    opp = np.array([[dim, dim + 1]])
    cells = np.array([list(range(dim)) + [dim], list(range(dim)) + [dim + 1]])
    assert np.array_equal(mref.opposite_vertices(cells, np.array([[0, dim, 1, 0]]), fv), opp)
    e = coords[1:dim] - coords[0]
    nrm = np.array([e[0, 1], -e[0, 0]]) if dim == 2 else np.cross(e[0], e[1])
    meas = np.array([np.linalg.norm(nrm) / math.factorial(dim - 1)])
    nrm = nrm / np.linalg.norm(nrm)
    nrm = -nrm if nrm @ (coords[dim] - coords[0]) > 0 else nrm
    lam = [_Nodal(np.r_[np.eye(dim)[a], 0.0, 0.0]) for a in range(dim)]
    for powers in [[1, 0, 0], [1, 1, 0], [2, 1, 0], [3, 2, 0], [4, 6, 0]] + ([[1, 1, 1], [2, 1, 3], [4, 3, 3]] if dim == 3 else []):
        powers = powers[:dim]
        ex = fem.as_expr(1.0)
        for a, k in enumerate(powers):
            if k:
                ex = ex * lam[a] ** k
        exact = math.factorial(dim - 1) * meas[0] * np.prod([math.factorial(k) for k in powers]) / math.factorial(dim - 1 + sum(powers))
        qp, qw = facet_quadrature(dim, sum(powers))
        (got, scale), = mref.integrate_facets(coords, fv, opp, meas, [ex], qp, qw)
        assert abs(got - exact) <= 1e-13 * scale, (powers, got, exact)
        if sum(powers) >= 4:      # and a rule four degrees short is not exact
            qp, qw = facet_quadrature(dim, sum(powers) - 4)
            (low, _), = mref.integrate_facets(coords, fv, opp, meas, [ex], qp, qw)
            assert abs(low - exact) > 1e-6 * abs(exact)
    # a linear function with a large offset: its coefficients on both sides, whatever the offset
    a = rng.uniform(-2.0, 2.0, dim)
    lin = _Nodal(coords @ a - 70.0, "lin")
    n = fem.FacetNormal(type("M", (), {"geometry": type("G", (), {"dim": dim})})())
    qp, qw = facet_quadrature(dim, 2)
    exprs = [fem.Derivative(lin, k, r) for r in "+-" for k in range(dim)] + [c("+") for c in n] + [c("-") for c in n] + \
            [fem.NormalDerivative(lin, "+"), fem.NormalDerivative(lin, "-"), fem.Derivative(lin, 0), fem.NormalDerivative(lin)]
    res = mref.integrate_facets(coords, fv, opp, meas, exprs, qp, qw, sides={id(lin): 1})
    got = np.array([r[0] for r in res]) / meas[0]
    want = np.r_[a, a, nrm, -nrm, a @ nrm, -(a @ nrm), a[0], -(a @ nrm)]
    assert np.allclose(got, want, rtol=0, atol=5e-13), (got, want)
    # a kink across the facet: each side sees its own cell
    kink = lin.numpy().copy()
    kink[dim + 1] += 0.5
    K = _Nodal(kink, "kink")
    (dp, _), (dm, _) = mref.integrate_facets(coords, fv, opp, meas, [fem.NormalDerivative(K, "+"), fem.NormalDerivative(K, "-")], qp, qw)
    assert abs(dp / meas[0] - a @ nrm) < 5e-13 and abs(dm / meas[0] + a @ nrm) > 0.1
