"""The inputs of tests/test_gpu_functionals_irregular.py, pinned without a GPU: the meshes have the properties the GPU tests rest on,
the NumPy references (tests/functional_ref.py, tests/membrane_functional_ref.py) meet closed forms on them, and every case that reads
a derivative or the normal has a tolerance max(TOL, 8 * floor) <= 1e-10, the floor being the distance between the fp64 reference and
its long-double-geometry twin (tests/functionals_irregular.py).  A failure of the GPU file is then the kernels', not the fixtures'.

All derivative cases keep all their meshes: the worst floor is 9.1e-16 (the nonlinear volume mix on the two-tag delaunay3d_5), and
hub2d_12_300 (edge matrices of condition 234) stays at 3.2e-16, so every tolerance is TOL itself.  The table is printed by
``test_tolerance_floors`` and kept in DESIGN.md section 4."""
import itertools
import math

import numpy as np
import pytest

import functional_ref
import functionals_irregular as FI
import irregular_meshes as IM
import membrane_functional_ref as mref
from functional_ref import TOL

GEOMETRY = ["delaunay2d_12_cw", "hub2d_12_48m_cw", "hub2d_12_300", "delaunay3d_5", "delaunay3d_7", "hub3d_5_60", "hub3d_5_60m", "delaunay2d_92"]
MEMBRANE_GEOMETRY = ["delaunay2d_12_cw", "hub2d_12_48m_cw", "delaunay3d_5", "delaunay3d_7", "hub3d_5_60m", "delaunay2d_92"]


@pytest.fixture(scope="module")
def stats():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = FI.mesh_stats(*IM.mesh(name))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def probs(tmp_path_factory):
    cache = {}
    tmp = tmp_path_factory.mktemp("functionals_irregular_host")

    def get(name):
        if name not in cache:
            cache[name] = FI.Prob(tmp, name)
        return cache[name]
    return get


# ---------------------------------------------------------------------------------------------- the meshes
@pytest.mark.parametrize("name", FI.CW)
def test_reoriented_meshes_keep_everything_but_the_orientation(name, stats):
    coords, cells, tags = IM.mesh(name)
    c0, cells0, t0 = IM.mesh(IM.PARENT[name])
    assert coords is c0 and tags is t0 and cells.dtype == np.int32 and not cells.flags.writeable
    assert np.array_equal(np.sort(cells, axis=1), np.sort(cells0, axis=1)) and not np.array_equal(cells, cells0)
    assert all(np.array_equal(a, b) for a, b in zip(IM.mesh(name), IM.ORIENTED[name]()))      # seeded
    s, s0 = stats(name), stats(IM.PARENT[name])
    print(name, "det < 0:", s["neg"], "parent:", s0["neg"])
    assert s0["neg"] == 0.0 and 0.3 <= s["neg"] <= 0.7
    # the same membrane facets between the same cells (a cell's facets are listed by local index, so their order may differ)
    rows = lambda t: sorted(map(tuple, np.column_stack([t["gamma"][:, [0, 2]], np.sort(t["fv"], axis=1)]).tolist()))
    assert rows(s) == rows(s0)


@pytest.mark.parametrize("name", MEMBRANE_GEOMETRY)
def test_membrane_facets_take_every_local_index_and_many_sizes(name, stats):
    s = stats(name)
    dim = IM.mesh(name)[0].shape[1]
    spread = s["meas"].max() / s["meas"].min()
    print(f"{name}: {s['n_cells']} cells, {s['n_facets']} membrane facets, det < 0 {100 * s['neg']:.0f} %, max cond(E) {s['cond']:.0f}, "
          f"facet-measure spread {spread:.1f}")
    assert np.all(s["opp"] >= 0)
    for side in range(2):
        assert set(s["local"][:, side].tolist()) == set(range(dim + 1)), (name, side)
    assert spread > 3.0


def test_the_two_tag_split_takes_every_local_index_too():
    coords, cells, tags = IM.mesh("delaunay3d_5")
    s = FI.mesh_stats(coords, cells, IM.two_tag(coords, cells, tags), (2, 3), (1,), "intra")
    assert all(set(s["local"][:, side].tolist()) == {0, 1, 2, 3} for side in range(2)) and s["meas"].max() > 3.0 * s["meas"].min()


def test_three_dimensional_meshes_hold_both_orientations(stats):
    for name in ("delaunay3d_5", "delaunay3d_7", "hub3d_5_60", "hub3d_5_60m"):
        assert 0.3 <= stats(name)["neg"] <= 0.7, name


def test_the_membrane_hubs_carry_facets(stats):
    for name, centre in (("hub3d_5_60m", IM.MEMBRANE_HUB_3D), ("hub2d_12_48m_cw", IM.MEMBRANE_HUB)):
        v = IM.hub_vertex(IM.mesh(name)[0], centre)
        at = np.any(stats(name)["fv"] == v, axis=1).sum()
        print(name, "membrane facets at the hub:", at)
        assert at >= 2
    s = stats("hub3d_5_60m")
    assert s["meas"].max() / s["meas"].min() > 50.0


def test_the_block_edge_meshes_are_large_enough(stats):
    for name in ("delaunay3d_7", "delaunay2d_92"):
        assert stats(name)["n_facets"] >= FI.FN_BT + 1, name
    for name in ("delaunay2d_12_cw", "delaunay3d_5"):
        assert IM.mesh(name)[1].shape[0] >= 2 * FI.FN_BT + 1, name
    for name, sp in FI.SEG_PTRS.items():
        assert sp[0] == 0 and np.all(np.diff(sp) >= 0), name
        capped = FI.seg_ptr_for(name, 184)
        assert capped[-1] == min(sp[-1], 184) and np.all(np.diff(capped) >= 0)


# ---------------------------------------------------------------------------------------------- the references against closed forms
@pytest.mark.parametrize("longdouble", [False, True])
@pytest.mark.parametrize("name", GEOMETRY)
def test_volumes_tile_the_box_and_gradients_are_exact_on_affine_fields(name, longdouble):
    coords, cells, _ = IM.mesh(name)
    X = coords[cells]
    vol = functional_ref.cell_volumes(X, longdouble)
    assert vol.min() > 0 and abs(math.fsum(vol) - 1.0) <= 1e-13
    a = np.random.default_rng(2).uniform(0.5, 1.5, coords.shape[1])
    f = coords @ a + 0.25
    G = functional_ref.simplex_gradients(X, longdouble)
    g = np.einsum("nak,na->nk", G, f[cells])
    scale = np.abs(G).sum(axis=(1, 2)) * np.abs(f).max()
    print(name, "longdouble" if longdouble else "fp64", "max |grad - a| / (|G|_1 |f|):", np.max(np.abs(g - a) / scale[:, None]))
    assert np.all(np.abs(g - a) <= 4e-16 * scale[:, None] * (coords.shape[1] + 1))
    assert np.max(np.abs(G.sum(axis=1))) <= 1e-9 * np.abs(G).max()


def test_the_two_geometry_paths_agree_to_rounding():
    for name in GEOMETRY:
        X = IM.mesh(name)[0][IM.mesh(name)[1]]
        G, Gl = functional_ref.simplex_gradients(X), functional_ref.simplex_gradients(X, True)
        cond = np.linalg.cond(X[:, 1:, :] - X[:, :1, :])
        rel = np.abs(G - Gl).max(axis=(1, 2)) / np.abs(Gl).max(axis=(1, 2))
        print(f"{name}: max |G - G_ld| / |G| = {rel.max():.2e}, against eps cond: {(rel / (2.2e-16 * cond)).max():.2f}")
        assert np.all(rel <= 16 * 2.2e-16 * cond)
        assert np.allclose(functional_ref.cell_volumes(X), functional_ref.cell_volumes(X, True), rtol=1e-13, atol=0)


@pytest.mark.parametrize("longdouble", [False, True])
@pytest.mark.parametrize("name", MEMBRANE_GEOMETRY)
def test_divergence_theorem_and_one_sided_gradients(name, longdouble, stats):
    """x . n('+') over the closed membrane is dim x the intracellular volume, every normal component integrates to zero, and the
    gradient of a nodally affine field is its coefficient vector on both sides of every facet: through integrate_facets"""
    from cgx_hip import fem
    from cgx_hip.mesh import facet_quadrature
    coords, cells, tags = IM.mesh(name)
    dim = coords.shape[1]
    s = stats(name)
    mesh = type("M", (), {"geometry": type("G", (), {"dim": dim})()})()
    x, n = list(fem.SpatialCoordinate(mesh)), [c("+") for c in fem.FacetNormal(mesh)]
    qp, qw = facet_quadrature(dim, 1)
    r = mref.integrate_facets(coords, s["fv"], s["opp"], s["meas"], [fem.inner(x, n)] + n, qp, qw, longdouble=longdouble)
    want = dim * math.fsum(functional_ref.cell_volumes(coords[cells[tags == 1]]))
    print(name, "x.n:", abs(r[0][0] - want) / r[0][1], "normal components:", [abs(v) / sc for v, sc in r[1:]])
    assert abs(r[0][0] - want) <= TOL * r[0][1]
    for v, sc in r[1:]:
        assert abs(v) <= TOL * sc
    assert np.allclose(mref.facet_measures_longdouble(coords, s["fv"]), s["meas"], rtol=1e-14, atol=0)
    a = np.random.default_rng(4).uniform(0.5, 1.5, dim)
    f = coords @ a + 0.25
    for side in range(2):
        cv = np.concatenate([s["fv"], s["opp"][:, side:side + 1]], axis=1)
        G = functional_ref.simplex_gradients(coords[cv], longdouble)
        g = np.einsum("nbk,nb->nk", G[:, 1:, :], f[cv][:, 1:] - f[cv][:, :1])
        assert np.all(np.abs(g - a) <= 8e-16 * np.abs(G).sum(axis=(1, 2))[:, None] * np.abs(f).max())


@pytest.mark.parametrize("name,degree,n_q", [("delaunay3d_5", 9, 125), ("hub3d_5_60", 9, 125), ("delaunay2d_12_cw", 21, 121), ("hub2d_12_300", 21, 121)])
def test_the_largest_rules_integrate_every_monomial_of_their_degree(name, degree, n_q):
    from cgx_hip.functionals import quadrature
    coords, cells, _ = IM.mesh(name)
    dim = coords.shape[1]
    qb, qw = quadrature(dim, degree)
    assert len(qw) == n_q and abs(qw.sum() - 1.0) <= 1e-14
    X = coords[cells]
    w = (functional_ref.cell_volumes(X)[:, None] * qw[None, :]).ravel()
    xq = np.einsum("qa,nak->nqk", qb, X).reshape(-1, dim)
    P = np.stack([xq ** k for k in range(degree + 1)])      # P[k, point, axis]
    worst = 0.0
    for e in itertools.product(range(degree + 1), repeat=dim):
        if sum(e) > degree:
            continue
        got = math.fsum(w * np.prod([P[e[k], :, k] for k in range(dim)], axis=0))
        want = 1.0 / np.prod([k + 1.0 for k in e])
        worst = max(worst, abs(got / want - 1.0))
    print(f"{name}: degree {degree}, {n_q} points: worst relative error over all monomials {worst:.2e}")
    assert worst <= 1e-12      # positive integrands: sum |w f| is the integral


# ---------------------------------------------------------------------------------------------- the tolerance of every derivative case
def test_tolerance_floors(probs, tmp_path):
    for name in FI.VOLUME_MESHES:
        for case in FI.VOLUME_CASES:
            FI.volume_floor(probs(name), case)
    for name in FI.MEMBRANE_MESHES:
        for case in FI.MEMBRANE_CASES:
            FI.membrane_floor(probs(name), case)
    FI.emi_floor(FI.emi_problem(tmp_path))
    table = FI.floor_table()
    print("\n".join(table))
    assert len(table) == len(FI.VOLUME_MESHES) * len(FI.VOLUME_CASES) + len(FI.MEMBRANE_MESHES) * len(FI.MEMBRANE_CASES) + 1
    for f in FI._FLOORS.values():
        assert np.isfinite(f) and FI.tolerance(f) <= FI.BOUND


def test_problems_on_the_reoriented_meshes_hold_the_parents_fields(probs):
    for name in FI.CW:
        a, b = probs(name), probs(IM.PARENT[name])
        assert np.array_equal(a.user.numpy(), b.user.numpy()) and np.array_equal(a.p.wh[0][3].numpy(), b.p.wh[0][3].numpy())
        assert np.array_equal(a.p.local_mesh.coords, b.p.local_mesh.coords) and not np.array_equal(a.p.local_mesh.cells, b.p.local_mesh.cells)
        # The references of the two orientations agree where the rule is exact (the polynomial case).  The rule is a collapsed
        # Gauss-Jacobi rule, not symmetric under a permutation of the vertices: a non-polynomial integrand is sampled at other
        # points and the two orientations differ by the quadrature error, in the reference as on the device.
        (v, s), (v0, _) = FI.volume_reference(a, "mass_stiffness"), FI.volume_reference(b, "mass_stiffness")
        print(name, "mass_stiffness: reference cw against ccw:", np.max(np.abs(v - v0) / s))
        assert np.all(np.abs(v - v0) <= TOL * s)
        (v, s), (v0, _) = FI.volume_reference(a, "nonlinear"), FI.volume_reference(b, "nonlinear")
        print(name, "nonlinear: reference cw against ccw (quadrature error):", np.max(np.abs(v - v0) / s))
        assert np.all(np.abs(v - v0) <= 0.05 * s) and np.any(np.abs(v - v0) > TOL * s)


# ---------------------------------------------------------------------------------------------- the oracle on clockwise cells
@pytest.mark.parametrize("name", FI.CW)
def test_the_oracle_does_not_see_the_orientation(name):
    o, o0 = IM.oracle(name), IM.oracle(IM.PARENT[name])
    IM.perturb(o)
    IM.perturb(o0)
    assert np.array_equal(o.lay.node_i, o0.lay.node_i) and np.array_equal(o.lay.node_e, o0.lay.node_e)
    for what in ("assemble_A", "assemble_P"):
        A, A0 = getattr(o, what)().tocsr(), getattr(o0, what)().tocsr()
        d = abs(A - A0).max() / abs(A0).max()
        print(name, what, "cw against ccw:", d)
        assert A.shape == A0.shape and d <= 1e-13
    b, b0 = o.assemble_b(), o0.assemble_b()
    assert np.max(np.abs(b - b0)) <= 1e-13 * np.max(np.abs(b0))
    IM.check_launch(IM.predicted_launch(o), IM.PARENT[name])
