"""What tests/test_gpu_emi_irregular.py rests on, without a GPU: the launch constants it restates are those of the sources, every
mesh is on the intended side of the grid caps of csrc/knp_emi.inc, and the k-step reference ``EmiRef.pcg`` is good for a 1e-12
comparison (its own fp64 / long double spread is far below) and converges to the LU solution."""
import os
import re

import numpy as np
import pytest

import emi_ref
import irregular_meshes as IM
import emi_irregular as GI
from emi_irregular import CM, DT, SE, SI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "knp-emi-cgx_amd", "csrc")


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name, two=False):
        if (name, two) not in cache:
            coords, cells, tags, intra, extra, gamma, gtags, _ = IM.emi_arrays(name, two)
            ref = emi_ref.from_tags(coords, cells, tags, intra, gamma, dt=DT, C_M=CM, sigma_i=SI, sigma_e=SE)
            ref.nullspace = True
            cache[(name, two)] = (ref, gtags)
        return cache[(name, two)]
    return get


# ------------------------------------------------------------------------------------------ launch constants
def _body(text, head):
    """the text of the function whose definition starts with ``head``, up to the brace that closes it"""
    i = text.index(head)
    j = text.index("{", i)
    depth, k = 1, j + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(text[k], 0)
        k += 1
    return text[j:k]


def test_restated_launch_constants_are_those_of_the_sources():
    emi = open(os.path.join(CSRC, "knp_emi.inc")).read()
    kernels = open(os.path.join(CSRC, "knp_kernels.hip")).read()

    def const(text, name):
        found = re.findall(r"\bconstexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
        assert len(found) == 1, (name, found)
        return int(found[0])
    assert const(kernels, "NT") == GI.NT
    assert const(emi, "EMI_SPMV_BLOCKS") == GI.EMI_SPMV_BLOCKS
    assert const(emi, "EMI_VEC_BLOCKS") == GI.EMI_VEC_BLOCKS
    assert const(emi, "EMI_BT") == GI.EMI_BT
    assert const(_body(emi, "static void emi_launch_spmv("), "G") == GI.G
    assert const(_body(emi, "int knp_emi_assemble_rhs("), "G") == GI.G


# ------------------------------------------------------------------------------------------ what each mesh is for
def _shape(refs, name):
    ref, _ = refs(name)
    L = GI.launch_shape(ref.n, len(ref.fv))
    L.update(n=ref.n, n_facets=len(ref.fv), facets_per_vertex=int(np.bincount(ref.fv.ravel()).max()),
             spread=float(ref.fmeas.max() / ref.fmeas.min()), longest_row=int(np.diff(ref.A.indptr).max()))
    print(name, L)
    return L


def test_launch_shape_at_the_caps():
    NT, G = GI.NT, GI.G
    per_block = NT // G
    n = GI.EMI_SPMV_BLOCKS * per_block
    assert GI.launch_shape(n, 1)["spmv_trips"] == 1 and GI.launch_shape(n + 1, 1)["spmv_trips"] == 2
    assert GI.launch_shape(n + 1, 1)["spmv_last_trip"] == 1
    assert GI.launch_shape(NT * per_block, 1)["sum_trips_pq"] == 1 and GI.launch_shape(NT * per_block + 1, 1)["sum_trips_pq"] == 2
    assert GI.launch_shape(NT * NT, 1)["sum_trips_rows"] == 1 and GI.launch_shape(NT * NT + 1, 1)["sum_trips_rows"] == 2
    m = GI.EMI_VEC_BLOCKS * NT
    assert GI.launch_shape(m, 1)["vec_strides"] == 1 and GI.launch_shape(m + 1, 1)["vec_strides"] == 2
    assert GI.launch_shape(1, GI.EMI_BT)["facet_blocks"] == 1 and GI.launch_shape(1, GI.EMI_BT)["facet_tail"] == 0
    assert GI.launch_shape(1, GI.EMI_BT + 1)["facet_blocks"] == 2 and GI.launch_shape(1, GI.EMI_BT + 1)["facet_tail"] == 1


def test_hub3d_5_60m_has_many_uneven_facets_at_one_vertex(refs):
    L = _shape(refs, "hub3d_5_60m")
    ref, _ = refs("hub3d_5_60m")
    assert L["facets_per_vertex"] >= 17 and L["facets_per_vertex"] > 2 * GI.G      # three trips of the ``c += G`` gather of k_emi_rhs
    assert L["spread"] >= 50.0 and L["longest_row"] > 6 * GI.G
    assert L["facet_blocks"] == 2 and L["facet_tail"] > 0
    # the vertex with the most facets is the hub, and it has a node on each side
    v = IM.hub_vertex(ref.coords, np.array(IM.MEMBRANE_HUB_3D) * 1e-6)
    assert np.bincount(ref.fv.ravel())[v] == L["facets_per_vertex"] and ref.node_i[v] >= 0 and ref.node_e[v] >= 0
    assert L["spmv_trips"] == 1 and L["sum_trips_pq"] == 1 and L["vec_strides"] == 1


def test_delaunay2d_92_sums_a_ragged_second_trip_of_partials(refs):
    L = _shape(refs, "delaunay2d_92")
    assert L["n"] > GI.NT * GI.NT // GI.G == 8192 and L["n"] <= GI.EMI_SPMV_BLOCKS * GI.NT // GI.G
    assert L["spmv_trips"] == 1 and GI.NT < L["spmv_blocks"] < 2 * GI.NT            # 277 partial sums of p . q: 256 + a ragged rest
    assert L["sum_trips_pq"] == 2 and L["sum_trips_rows"] == 1 and L["vec_strides"] == 1
    assert L["facet_blocks"] == 2 and L["facet_tail"] > 0


def test_delaunay2d_365_is_past_every_cap(refs):
    L = _shape(refs, "delaunay2d_365")
    assert L["n"] > GI.EMI_SPMV_BLOCKS * GI.NT // GI.G == 32768 and L["n"] > GI.EMI_VEC_BLOCKS * GI.NT == 131072
    assert L["spmv_blocks"] == GI.EMI_SPMV_BLOCKS and L["vec_blocks"] == GI.EMI_VEC_BLOCKS
    assert L["spmv_trips"] >= 5 and 0 < L["spmv_last_trip"] < L["spmv_groups"]       # the last trip is ragged: whole blocks of dead groups
    assert L["spmv_last_trip"] % (GI.NT // GI.G) != 0                                 # ... and one block with live and dead groups
    assert L["sum_trips_pq"] == 4 and L["sum_trips_rows"] == 2 and L["vec_strides"] == 2
    assert L["n"] % GI.NT != 0                                                        # the second stride ends inside a block
    assert L["facet_blocks"] >= 7 and L["facet_tail"] > 0 and L["facet_tail"] % 64 != 0
    assert L["spread"] >= 3.5


@pytest.mark.parametrize("name,least_facets,least_spread", [("delaunay3d_7", 12, 5.5), ("hub2d_12_48m", 2, 3.0)])
def test_reused_rhs_meshes(refs, name, least_facets, least_spread):
    L = _shape(refs, name)
    assert L["facets_per_vertex"] >= least_facets and L["spread"] >= least_spread
    assert (L["facets_per_vertex"] > GI.G) == (name == "delaunay3d_7")               # a second trip of the gather there


def test_hub2d_12_300_has_a_row_of_301_same_side_pairs(refs):
    assert _shape(refs, "hub2d_12_300")["longest_row"] >= 301


@pytest.mark.parametrize("name", GI.RHS_MESHES)
def test_two_tag_split_mixes_both_programs_in_a_wave(refs, name):
    """the facets come in the order of their intracellular cells, which the generator shuffled: tags 2 and 3 interleave"""
    ref, gtags = refs(name, True)
    ref1, _ = refs(name)
    assert np.array_equal(ref.fv, ref1.fv) and set(gtags.tolist()) == {2, 3}      # the same facets in the same order as with one tag
    mixed = [len(set(gtags[i:i + 64].tolist())) == 2 for i in range(0, len(gtags), 64)]
    print(name, "facets", len(gtags), "of tag 2:", int((gtags == 2).sum()), "waves holding both programs:", sum(mixed), "of", len(mixed))
    assert sum(mixed) >= 1
    if name == "delaunay2d_365":
        assert all(mixed)


def _residual_floor(ref):
    """eps | |A| |x| |_2 / |b| with x the LU solution of the right-hand side of the solve tests: the rounding of b - A x itself"""
    rng = np.random.default_rng(21)                 # the state of test_gpu_emi_irregular.test_solve_reaches_the_true_residual
    nv = ref.coords.shape[0]
    phi = rng.uniform(-0.1, 0.1, nv)
    gates = [rng.uniform(0.01, 0.99, nv) for _ in range(3)]
    ref.models = [emi_ref.hh_current]
    b = ref.rhs(phi, *gates, t=0.003)
    x = ref.solve(b)
    return np.finfo(float).eps * np.linalg.norm(abs(ref.A) @ np.abs(x)) / np.linalg.norm(b), np.linalg.norm(b - ref.A @ x) / np.linalg.norm(b)


def test_solve_meshes_can_reach_the_true_residual_bound(refs):
    """The solve tests ask for a true residual <= 2 rtol |b| at rtol 1e-10.  x is nearly constant per side and b is small against
    |A| |x|, so b - A x is itself only known to eps |A| |x|: that floor has to sit below rtol |b| / 2.  hub2d_12_300 misses it whatever
    the seed (the 2 pi / 300 angles at its hub give cotangents of 48: entries 200 times the typical one), which is why the solve tests
    with that bound take hub3d_5_140 for the long row.  What sparse LU leaves is printed, not asserted (it follows its pivoting)."""
    rtol = 1e-10
    for name in GI.SOLVE_MESHES:
        floor, lu = _residual_floor(refs(name)[0])
        print(f"{name}: eps | |A||x| | / |b| = {floor:.3e}, LU leaves {lu:.3e}")
        assert floor <= 0.5 * rtol
    floor, lu = _residual_floor(refs("hub2d_12_300")[0])
    print(f"hub2d_12_300: eps | |A||x| | / |b| = {floor:.3e}, LU leaves {lu:.3e}")
    assert floor > 2.0 * rtol
    assert int(np.diff(refs("hub3d_5_140")[0].A.indptr).max()) >= 141


def _device_pcg(A, b, B, rtol, max_it):
    """PCG as knp_emi_cg_solve writes it: z is not projected, mu = mean(z), beta = r . z - mu sum(r), p = (z - mu) + ..."""
    n = len(b)
    x = np.zeros(n)
    r = b - A @ x
    r -= r.mean()

    def reduce(r):
        z = B(r)
        mu = z.sum() / n
        return z, mu, r @ z - mu * r.sum()
    z, mu, beta = reduce(r)
    p = z - mu
    for it in range(max_it + 1):
        if np.linalg.norm(r) <= rtol * np.linalg.norm(b) or it == max_it:
            return it, np.linalg.norm(r) / np.linalg.norm(b)
        q = A @ p
        alpha = beta / (p @ q)
        x += alpha * p
        r -= alpha * q
        z, mu, beta_new = reduce(r)
        p = (z - mu) + (beta_new / beta) * p
        beta = beta_new


def test_hierarchy_on_hub2d_12_300_survives_rounding_of_the_matrix(refs):
    """The hierarchy is built from the matrix the device wrote, which differs from ``ref.A`` in the last bits.  On hub2d_12_300 that
    is enough to flip a decision of the set-up: on several of the perturbed copies below the coarsest operator (24 rows) is not
    singular any more, the image of the constant has eigenvalue 5.9e-12 against 1.3e-3 (the smallest physical one is 1.4e-8), a plain
    pseudo-inverse keeps it, and PCG with the device's formulas stalls near 1e-8 |b|.  ``build_emi_hierarchy`` leaves that mode out
    of the coarse inverse for a pure Neumann problem: PCG with the NumPy cycle then reaches 1e-10 |b| in about 30 iterations on
    every copy.  (Random relative perturbations of 2e-16 per entry, symmetric; seeds fixed.)"""
    import scipy.sparse as sp
    import knpemi_oracle as K
    from cgx_hip import amg
    from cgx_hip.emi_solver import build_emi_hierarchy
    ref, _ = refs("hub2d_12_300")
    rng = np.random.default_rng(21)
    nv = ref.coords.shape[0]
    ref.models = [emi_ref.hh_current]
    b = ref.rhs(rng.uniform(-0.1, 0.1, nv), *[rng.uniform(0.01, 0.99, nv) for _ in range(3)], t=0.003)
    lost = []
    for seed in (None, 1, 2, 3, 4, 5, 6, 7):
        A = ref.A
        if seed is not None:
            U = sp.triu(ref.A).tocsr()
            U.data = U.data * (1.0 + 2e-16 * np.random.default_rng(seed).standard_normal(U.nnz))
            A = (U + sp.triu(U, 1).T).tocsr()
        plain = amg.build_hierarchy(A, theta=0.08, coarse_size=40, smoother_degree=1)
        w = np.linalg.eigvalsh(plain.levels[-1].A.toarray())
        lost.append(bool(np.abs(w).min() > 1e-13 * np.abs(w).max()))
        h = build_emi_hierarchy(A, True, 0.08, 40, 1)
        assert np.abs(h.coarse_inv).max() <= 10.0 / np.sort(np.abs(w))[1]            # nothing near 1 / 5.9e-12 is left in it
        its, rel = _device_pcg(ref.A, b, K.pc_amg_vcycle(h.levels, h.coarse_inv, 1, 1, 1), 1e-10, 100)
        its0, rel0 = _device_pcg(ref.A, b, K.pc_amg_vcycle(plain.levels, plain.coarse_inv, 1, 1, 1), 1e-10, 100)
        print(f"seed {seed}: coarse eigenvalues {np.sort(np.abs(w))[:2]} of {np.abs(w).max():.2e}; PCG {its} iterations to {rel:.2e} |b| "
              f"(plain pseudo-inverse: {its0} to {rel0:.2e})")
        assert its < 100 and rel <= 1e-10
    assert any(lost) and not all(lost)            # the copies do reach both outcomes of the set-up


def test_dense_pseudo_inverse_leaves_out_the_known_null_modes():
    from cgx_hip import amg
    import scipy.sparse as sp
    rng = np.random.default_rng(0)
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    w = np.array([3e-12, 1e-8, 1e-3, 0.5, 1.0, 2.0])
    D = (Q * w) @ Q.T
    D = 0.5 * (D + D.T)
    plain = amg.dense_pseudo_inverse(sp.csr_matrix(D))
    one = amg.dense_pseudo_inverse(sp.csr_matrix(D), null_dim=1)
    assert np.abs(plain @ D - np.eye(6)).max() <= 1e-3                        # every mode is above the relative cut-off: an inverse
    want = (Q[:, 1:] / w[1:]) @ Q[:, 1:].T
    assert np.abs(one - want).max() <= 1e-6 * np.abs(want).max() and np.abs(one @ Q[:, 0]).max() <= 1e-6 * np.abs(one).max()
    # an exactly singular operator: the same result with and without the hint
    D0 = (Q[:, 1:] * w[1:]) @ Q[:, 1:].T
    D0 = 0.5 * (D0 + D0.T)
    a, b = amg.dense_pseudo_inverse(sp.csr_matrix(D0)), amg.dense_pseudo_inverse(sp.csr_matrix(D0), null_dim=1)
    assert np.abs(a - b).max() <= 1e-6 * np.abs(a).max()


def test_delaunay2d_24_gives_three_levels():
    from cgx_hip import amg
    coords, cells, tags, intra, extra, gamma, _, _ = IM.emi_arrays("delaunay2d_24")
    ref = emi_ref.from_tags(coords, cells, tags, intra, gamma, dt=DT, C_M=CM, sigma_i=SI, sigma_e=SE)
    h = amg.build_hierarchy(ref.A, theta=0.08, coarse_size=40, smoother_degree=1)
    print("delaunay2d_24 hierarchy rows:", h.describe()["rows"])
    assert len(h.levels) >= 3


# ------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("name", GI.ALL)
def test_reference_matrix_is_symmetric_and_annihilates_the_constant(refs, name):
    ref, _ = refs(name)
    A = ref.A
    assert abs(A - A.T).max() <= 1e-15 * abs(A).max()
    assert np.abs(A @ np.ones(ref.n)).max() <= 1e-14 * abs(A).max()


def test_pcg_spread_between_fp64_and_long_double(refs):
    """The precondition of the 1e-12 comparisons on the GPU: ten Jacobi-preconditioned steps on delaunay2d_365 in fp64 and in long
    double differ by max|dx| / max|x| <= 1e-14 (measured: see the printed figure), two orders below the tolerance."""
    assert np.finfo(np.longdouble).eps < 1e-18
    ref, _ = refs("delaunay2d_365")
    b = np.random.default_rng(41).standard_normal(ref.n)
    b -= b.mean()
    for norm_type in ("preconditioned", "natural"):
        x, r, norms = ref.pcg(b, 10, "jacobi", norm_type)
        xl, rl, norms_l = ref.pcg(b, 10, "jacobi", norm_type, dtype=np.longdouble)
        assert x.dtype == np.float64 and xl.dtype == np.longdouble and len(norms) == 11
        dx = float(np.abs(x - xl).max() / np.abs(xl).max())
        dn = float(np.abs(norms - norms_l).max() / norms_l.max())
        print(f"delaunay2d_365 jacobi {norm_type} k = 10: fp64 against long double max|dx| / max|x| = {dx:.3e}, norms {dn:.3e}")
        assert dx <= 1e-14 and np.all(np.abs(norms - norms_l) <= 1e-13 * norms_l)


def test_pcg_norm_types_and_residual(refs):
    """the returned r is the recurrence's residual of the returned x, and the three norms are norms of that pair"""
    ref, _ = refs("delaunay2d_92")
    b = np.random.default_rng(5).standard_normal(ref.n)
    b -= b.mean()
    d = ref.A.diagonal()
    for pc in ("none", "jacobi"):
        x, r, n_un = ref.pcg(b, 7, pc, "unpreconditioned")
        assert np.abs(r - (b - ref.A @ x)).max() <= 1e-12 * np.abs(b).max() and n_un[-1] == pytest.approx(np.linalg.norm(r), rel=1e-14)
        z = r / d if pc == "jacobi" else r
        z = z - z.mean()
        assert ref.pcg(b, 7, pc, "preconditioned")[2][-1] == pytest.approx(np.linalg.norm(z), rel=1e-12)
        assert ref.pcg(b, 7, pc, "natural")[2][-1] == pytest.approx(np.sqrt(r @ z), rel=1e-12)
        assert abs(x.mean()) <= 1e-12 * np.abs(x).max()             # the gauge of the zero guess is kept


def _converged(ref, b, pc, rtol=1e-10):
    """``pcg`` with the number of steps doubled until the recurrence's residual is below rtol |b|, b over the free nodes (the
    Dirichlet values are orders above the membrane terms and carry no residual)"""
    k = 50
    while True:
        x, r, norms = ref.pcg(b, k, pc, "unpreconditioned")
        if norms[-1] <= rtol * np.linalg.norm(np.delete(b, ref.bc_nodes)):
            return x, norms, k
        k *= 2
        assert k <= 51200, (pc, norms[-1])


def test_pcg_converges_to_the_lu_solution(refs):
    ref, _ = refs("hub3d_5_60m")
    rng = np.random.default_rng(6)
    nv = ref.coords.shape[0]
    b = ref.rhs(rng.uniform(-0.1, 0.1, nv), *[rng.uniform(0.01, 0.99, nv) for _ in range(3)], t=0.003)
    x_lu = ref.solve(b)
    for pc in ("none", "jacobi"):
        x, norms, k = _converged(ref, b, pc)
        print(f"hub3d_5_60m {pc}: |r| / |b| after {k} steps = {norms[-1] / np.linalg.norm(b):.3e}, max|x - x_lu| / max|x_lu| = {np.abs(x - x_lu).max() / np.abs(x_lu).max():.3e}")
        assert np.allclose(x, x_lu, rtol=1e-6, atol=1e-9 * np.abs(x_lu).max())
    # Dirichlet nodes: x = b there, the rest converges to the LU solution of the eliminated operator
    coords, cells, tags, intra, extra, gamma, _, _ = IM.emi_arrays("hub3d_5_60m")
    ref2 = emi_ref.from_tags(coords, cells, tags, intra, gamma, dt=DT, C_M=CM, sigma_i=SI, sigma_e=SE)
    nodes = np.unique(rng.choice(ref2.n, size=20, replace=False))
    ref2.set_dirichlet(nodes)
    g = np.zeros(ref2.n)
    g[nodes] = rng.uniform(-0.01, 0.01, len(nodes))
    b2 = ref2.rhs(rng.uniform(-0.1, 0.1, nv), g=g)
    x2, n2, _ = _converged(ref2, b2, "jacobi")
    assert np.array_equal(x2[nodes], g[nodes])
    assert np.allclose(x2, ref2.solve(b2), rtol=1e-6, atol=1e-9 * np.abs(x2).max())
