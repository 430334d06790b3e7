"""Host side of the volume functionals (cgx_hip/functionals.py, cgx_hip/fem.py): how integrands compile -- roles, aux slots,
derivative bindings --, the errors of ``compile_functional``, and the NumPy reference on single cells.  No device."""
import math

import numpy as np
import pytest

import functional_ref
from parity_utils import ci_config, make_problem, tissue_config


@pytest.fixture(scope="module")
def problem():
    return make_problem(ci_config(N=8, steps=1), "ci")


def _ops(spec):
    from cgx_hip._lib import OPS
    inv = {v: k for k, v in OPS.items()}
    return [(inv[op], a) for op, _, a, _ in spec.code.tolist() if inv[op] in ("KI", "KE", "PHIM", "AUX", "X", "OUT")]


def test_roles_and_aux_slots(problem):
    from cgx_hip import fem
    from cgx_hip.functionals import compile_functional
    p = problem
    user = fem.Function(p.V, "user")
    x = fem.SpatialCoordinate(p.mesh)
    spec = compile_functional(p, integrand_i=[p.wh[0][0] * p.wh[0][2], p.wh[0][3] * p.phi_m_prev + user * x[1]],
                              integrand_e=[p.wh[1][1], p.wh[1][3] * p.wh[1][3]])
    assert spec.n_out == 2 and not spec.single and [sp.side for sp in spec.sides] == [0, 1]
    si, se = spec.sides
    assert _ops(si.spec) == [("KI", 0), ("KI", 2), ("AUX", 0), ("AUX", 1), ("AUX", 2), ("X", 1), ("OUT", 0), ("OUT", 1)]
    assert [f.name for f in si.spec.aux_functions] == [p.wh[0][3].name, p.phi_m_prev.name, "user"]
    assert si.spec.aux_functions[0] is p.wh[0][3] and si.spec.aux_functions[1] is p.phi_m_prev and si.spec.aux_derivs == [-1, -1, -1]
    assert _ops(se.spec) == [("KE", 1), ("AUX", 0), ("OUT", 0), ("OUT", 1)]
    assert se.spec.aux_functions == [p.wh[1][3]] and se.spec.aux_derivs == [-1]
    # rows: the intracellular tags, then the extracellular ones; the cell lists cover each side's owned cells once
    assert list(spec.tags) == [int(t) for t in p.intra_tags] + [int(t) for t in np.ravel(p.extra_tag)]
    assert list(spec.side) == [0] * len(p.intra_tags) + [1] * len(np.ravel(p.extra_tag))
    for sp in spec.sides:
        assert np.array_equal(np.sort(sp.cells), np.nonzero(p.cell_side == sp.side)[0])
    assert spec.volume.sum() == pytest.approx(functional_ref.cell_volumes(p.local_mesh.coords[p.local_mesh.cells]).sum(), rel=1e-13)


def test_a_derivative_of_the_same_function_and_axis_shares_a_slot(problem):
    from cgx_hip import fem
    from cgx_hip.functionals import compile_functional
    p = problem
    u, v = p.wh[0][0], p.wh[0][3]
    spec = compile_functional(p, integrand_i=fem.inner(fem.grad(u), fem.grad(u)) + fem.inner(fem.grad(u), fem.grad(v)) + u * v)
    assert spec.single and spec.n_out == 1
    prog = spec.sides[0].spec
    # u itself is KI 0; du/dx, du/dy, dv/dx, dv/dy and v's value take one slot each, however often they are read
    bound = [(f.name, a) for f, a in zip(prog.aux_functions, prog.aux_derivs)]
    assert len(bound) == 5 and sorted(bound) == sorted([(u.name, 0), (u.name, 1), (v.name, 0), (v.name, 1), (v.name, -1)])
    assert sum(1 for op, _ in _ops(prog) if op == "AUX") == 5 and ("KI", 0) in _ops(prog)


def test_compile_program_called_the_old_way_refuses_a_derivative(problem):
    from cgx_hip import fem
    p = problem
    g = fem.grad(p.wh[0][3])
    assert len(g) == 2 and all(isinstance(c, fem.Derivative) and c.axis == k for k, c in enumerate(g))
    with pytest.raises(TypeError):
        fem.compile_program([g[0] * 2.0], {})
    with pytest.raises(TypeError):
        fem.compile_program([g[0]], {}, [])
    aux, der = [], []
    spec = fem.compile_program([g[1]], {}, aux, der)
    assert aux == [p.wh[0][3]] and der == [1] and spec.aux_derivs is der
    with pytest.raises(TypeError):
        fem.grad(p.wh[0][3] * 2.0)
    with pytest.raises(ValueError):
        fem.inner(g, [g[0]])
    assert isinstance(fem.inner(2.0, p.wh[0][3]), fem.Op)


def test_value_errors(problem):
    from cgx_hip import fem
    from cgx_hip._lib import KNP_MAX_AUX
    from cgx_hip.functionals import compile_functional
    p = problem
    ti, te = int(p.intra_tags[0]), int(np.ravel(p.extra_tag)[0])
    with pytest.raises(ValueError, match="other side"):
        compile_functional(p, integrand_i=p.wh[1][0])
    with pytest.raises(ValueError, match="other side"):
        compile_functional(p, integrand_e=fem.grad(p.wh[0][3])[0])
    with pytest.raises(ValueError, match="not given"):
        compile_functional(p, integrand_i=p.wh[0][0], tags=[ti, te])
    with pytest.raises(ValueError, match="unknown cell tag"):
        compile_functional(p, integrand_i=p.wh[0][0], tags=[ti, 987654])
    with pytest.raises(ValueError, match="up to 3"):
        compile_functional(p, integrand_i=[p.wh[0][0]] * 4)
    with pytest.raises(ValueError):
        compile_functional(p)
    users = [fem.Function(p.V, f"u{k}") for k in range(KNP_MAX_AUX + 1)]
    total = users[0]
    for u in users[1:]:
        total = total + u
    with pytest.raises(ValueError, match="aux slots"):
        compile_functional(p, integrand_i=total)
    eight = p.wh[0][0]
    for u in users[:KNP_MAX_AUX]:
        eight = eight + u
    assert len(compile_functional(p, integrand_i=eight).sides[0].spec.aux_functions) == KNP_MAX_AUX      # a concentration takes no slot
    # 2D: m^2 points, m = ceil((degree + 1) / 2): degree 21 is the last that fits in 125; 3D: degree 9
    compile_functional(p, integrand_i=p.wh[0][0], degree=21)
    with pytest.raises(ValueError, match="quadrature points"):
        compile_functional(p, integrand_i=p.wh[0][0], degree=22)
    p3 = make_problem(ci_config(N=4, steps=1, kind="cube"), "ci")
    assert compile_functional(p3, integrand_i=p3.wh[0][0], degree=9).q_w.shape == (125,)
    with pytest.raises(ValueError, match="quadrature points"):
        compile_functional(p3, integrand_i=p3.wh[0][0], degree=10)
    assert compile_functional(p3, integrand_i=p3.wh[0][0]).q_bary.shape == (8, 4)


def test_tags_keep_their_order_within_a_side():
    from cgx_hip.functionals import compile_functional
    p = make_problem(tissue_config(2, 18, 3, steps=1), "ci")
    ics = [int(t) for t in p.intra_tags]
    e = int(np.ravel(p.extra_tag)[0])
    spec = compile_functional(p, integrand_i=1.0, integrand_e=1.0, tags=[ics[4], e, ics[1]])
    assert list(spec.tags) == [ics[4], ics[1], e] and list(spec.side) == [0, 0, 1]
    lm = p.local_mesh
    for sp in spec.sides:
        for k, t in enumerate(sp.tags):
            assert np.all(lm.cell_tags[sp.cells[sp.seg_ptr[k]:sp.seg_ptr[k + 1]]] == t)
    one = compile_functional(p, integrand_e=1.0)
    assert list(one.tags) == [e] and len(one.sides) == 1


@pytest.mark.parametrize("dim", [2, 3])
def test_the_reference_integrates_barycentric_polynomials_exactly(dim):
    """int_T prod lambda_a^{k_a} = d! |T| prod k_a! / (d + sum k_a)! on one skewed simplex, at the degree of the monomial"""
    from cgx_hip import fem
    from cgx_hip.functionals import quadrature

    class Nodal(fem.Function):
        def __init__(self, values):
            self._v = np.asarray(values, dtype=np.float64)
            self.name = "nodal"

        def numpy(self):
            return self._v
    rng = np.random.default_rng(5)
    coords = rng.uniform(-1.0, 1.0, (dim + 1, dim)) + 2.0 * np.eye(dim + 1)[:, :dim]
    cells = np.arange(dim + 1)[None, :]
    vol = functional_ref.cell_volumes(coords[cells])[0]
    lam = [Nodal(np.eye(dim + 1)[a]) for a in range(dim + 1)]
    for powers in [[1, 0, 0, 0], [1, 1, 0, 0], [2, 1, 0, 0], [1, 1, 1, 0], [2, 2, 1, 0], [3, 0, 2, 0]] + ([[1, 1, 1, 1], [2, 1, 1, 1]] if dim == 3 else []):
        powers = powers[:dim + 1]
        e = fem.as_expr(1.0)
        for a, k in enumerate(powers):
            if k:
                e = e * lam[a] ** k
        exact = math.factorial(dim) * vol * np.prod([math.factorial(k) for k in powers]) / math.factorial(dim + sum(powers))
        qb, qw = quadrature(dim, sum(powers))
        (got, scale), = functional_ref.integrate_cells(coords, cells, [e], qb, qw)
        assert abs(got - exact) <= 1e-14 * scale, (powers, got, exact)
        if sum(powers) >= 3:      # and a rule two degrees short is not exact
            qb, qw = quadrature(dim, sum(powers) - 2)
            (low, _), = functional_ref.integrate_cells(coords, cells, [e], qb, qw)
            assert abs(low - exact) > 1e-6 * abs(exact)
    # a derivative: grad(lambda_a) . grad(lambda_b) |T| is the P1 stiffness entry; the closed forms agree with the quadrature
    u, v = rng.uniform(-1, 1, dim + 1), rng.uniform(-1, 1, dim + 1)
    U, V = Nodal(u), Nodal(v)
    qb, qw = quadrature(dim, 2)
    (k_q, ks), (m_q, ms) = functional_ref.integrate_cells(coords, cells, [fem.inner(fem_grad(U, dim), fem_grad(V, dim)), U * V], qb, qw)
    assert abs(k_q - functional_ref.stiffness_form(coords, cells, u, v)[0]) <= 1e-13 * functional_ref.stiffness_form(coords, cells, u, v)[1]
    assert abs(m_q - functional_ref.mass_form(coords, cells, u, v)[0]) <= 1e-13 * functional_ref.mass_form(coords, cells, u, v)[1]
    G = functional_ref.simplex_gradients(coords[cells])[0]      # grad(lambda_a) . (x_b - x_0) = delta_ab - delta_a0
    assert np.allclose(G.sum(axis=0), 0.0, atol=1e-13) and np.allclose(G @ (coords[1:] - coords[0]).T, np.eye(dim + 1)[:, 1:] - np.eye(dim + 1)[:, :1], atol=1e-12)


def fem_grad(f, dim):
    from cgx_hip import fem
    return [fem.Derivative(f, a) for a in range(dim)]
