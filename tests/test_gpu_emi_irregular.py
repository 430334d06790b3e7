"""The EMI kernels (csrc/knp_emi.inc) on irregular meshes and past their grid caps, against tests/emi_ref.py.  tests/test_gpu_emi.py
runs them on generated grids of a few thousand unknowns: no grid-stride loop takes a second trip there, ``emi_sum_all`` adds at most
256 partial sums, a membrane vertex has a handful of facets of one measure, and no Dirichlet node touches the membrane.  The meshes
(tests/irregular_meshes.py) and what each is for are pinned without a GPU by tests/test_emi_irregular_host.py, which also reads the
launch constants restated in tests/emi_irregular.py out of the sources.

Tolerances are those of tests/test_gpu_emi.py.  The k-step comparisons use its operator tolerance 1e-12: the reference's own fp64 /
long double spread over the same ten iterations is two orders below it (host test).  No iteration counts are asserted."""
import numpy as np
import pytest
import torch

import emi_ref
import irregular_meshes as IM
import test_gpu_emi
from emi_irregular import ALL, CM, CONVERGED_RTOL, DIVERGED_ITS, DT, NORMS, RHS_MESHES, SE, SI, SOLVE_MESHES, launch_shape
from test_gpu_emi import T_STIM, _dev, _problem, _random_state, _rhs, _setup_pc

pytestmark = pytest.mark.gpu

assert (DT, CM, SI, SE) == (test_gpu_emi.DT, test_gpu_emi.CM, test_gpu_emi.SI, test_gpu_emi.SE)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """one problem per (mesh, models), built at first use and shared: "hh" / "passive" on one membrane tag, "mixed" on the two-tag
    split (HH on tag 2, passive on tag 3).  Tests that change the Dirichlet set build their own."""
    cache = {}
    tmp = tmp_path_factory.mktemp("emi_irregular")

    def get(mesh, models="hh"):
        if (mesh, models) not in cache:
            cache[(mesh, models)] = _problem(mesh, models, **IM.emi_config(tmp, mesh, two=(models == "mixed")))
        return cache[(mesh, models)]
    get.tmp = tmp
    return get


def _spmv(be, x):
    y = torch.empty(be.n_nodes, dtype=torch.float64, device=be.device)
    be.spmv(_dev(x, be), y)
    return y.cpu().numpy()


def _worst(err, bound):
    """max err / bound over the rows with a bound (0 when there is none); rows without one must be exact, the caller asserts it"""
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


# ------------------------------------------------------------------------------------------ a. matrix
@pytest.mark.parametrize("mesh", ALL)
def test_matrix_against_the_reference(cases, mesh):
    """k_emi_pairs / k_emi_gamma: up to 17 facets of a 55-fold measure spread under one membrane vertex pair (hub3d_5_60m)"""
    p, be, ref = cases(mesh)
    A = be.csr()
    amax = abs(ref.A).max()
    d, asym = abs(A - ref.A).max(), abs(A - A.T).max()
    print(f"{mesh}: n = {ref.n}, nnz = {A.nnz}, max|A| = {amax:.3e}, max|dA| / max|A| = {d / amax:.3e}, max|A - A^T| / max|A| = {asym / amax:.3e}")
    assert A.shape == ref.A.shape and d <= 1e-12 * amax and asym <= 1e-12 * amax
    lm = p.local_mesh
    ref2 = emi_ref.EmiRef(lm.coords, lm.cells, p.cell_side, lm.gamma, 3.0 * DT, p.C_M, p.sigma_i, p.sigma_e)
    be.setup(3.0 * DT, p.C_M, p.sigma_i, p.sigma_e)
    A2 = be.csr()
    be.setup(DT, p.C_M, p.sigma_i, p.sigma_e)
    a2 = abs(ref2.A).max()
    d2, asym2 = abs(A2 - ref2.A).max(), abs(A2 - A2.T).max()
    print(f"{mesh}: dt x 3: max|dA| / max|A| = {d2 / a2:.3e}, max|A - A^T| / max|A| = {asym2 / a2:.3e}")
    assert d2 <= 1e-12 * a2 and asym2 <= 1e-12 * a2
    assert abs(be.csr() - A).max() == 0.0


# ------------------------------------------------------------------------------------------ b. SpMV
@pytest.mark.parametrize("mesh", ALL)
def test_spmv_against_the_reference(cases, mesh):
    p, be, ref = cases(mesh)
    x = np.random.default_rng(1).standard_normal(ref.n)
    err = np.abs(_spmv(be, x) - ref.A @ x)
    bound = abs(ref.A) @ np.abs(x)
    print(f"{mesh}: SpMV max err / bound = {_worst(err, bound):.3e}")
    assert np.all(err <= 1e-12 * bound)


def test_spmv_trips_do_not_bleed(cases):
    """delaunay2d_365: five grid-stride trips of k_emi_spmv, the last with whole lane groups dead.  x = 1 on the nodes of the last trip
    and 0 elsewhere, and the reverse: a row whose neighbours are all zero has bound 0 and must come out as exactly 0 (with the random
    numbering most rows of the first four trips have no neighbour in the last one; every row has one outside it).

    The magnitude on the right is that of the terms behind each entry (``ref.absA_terms``: dt |sigma K_cell| summed over the cells,
    plus C_M |M_Gamma|), not |A|: a 0 / 1 vector picks single entries out of a row, and the mesh has edges whose two cotangents
    cancel to 6e-6 of a typical entry (1.9e-10 against 3.3e-5), which any assembly knows to eps of its terms only (the two here
    differ by 4e-11 of the entry).  With a random x the row's other entries cover that in |A| |x|; here nothing does."""
    p, be, ref = cases("delaunay2d_365")
    L = launch_shape(ref.n, len(ref.fv))
    assert L["spmv_trips"] >= 2 and 0 < L["spmv_last_trip"] < L["spmv_groups"]
    first_of_last = (L["spmv_trips"] - 1) * L["spmv_groups"]
    for name, x in (("last trip", (np.arange(ref.n) >= first_of_last).astype(np.float64)), ("all but the last trip", (np.arange(ref.n) < first_of_last).astype(np.float64))):
        y = _spmv(be, x)
        err, bound = np.abs(y - ref.A @ x), ref.absA_terms @ x
        print(f"delaunay2d_365, x = 1 on {name}: max err / (|terms| x) = {_worst(err, bound):.3e}, rows with bound 0: {(bound == 0).sum()}; "
              f"against |A| x: {_worst(err, abs(ref.A) @ x):.3e}")
        assert ((bound == 0).sum() > ref.n // 2 or name != "last trip") and np.all(err <= 1e-12 * bound)


# ------------------------------------------------------------------------------------------ c. right-hand side
@pytest.mark.parametrize("models", ["passive", "hh", "mixed"])
@pytest.mark.parametrize("mesh", RHS_MESHES)
def test_rhs_against_the_reference(cases, mesh, models):
    """k_emi_facets (blocks of 128 with a ragged tail, waves that hold both programs on the two-tag split) and the ``c += G`` gather of
    k_emi_rhs over up to 17 facets of differing measure"""
    p, be, ref = cases(mesh, models)
    phi, gates = _random_state(p, 7)
    n, m, h = gates if hasattr(p, "n") else (None, None, None)
    rng = np.random.default_rng(8)
    fi, fe = rng.standard_normal(p.mesh.num_vertices), rng.standard_normal(p.mesh.num_vertices)
    if models == "mixed":
        assert sorted(set(ref.facet_model.tolist())) == [0, 1]
    for with_src in (False, True):
        be.f_i, be.f_e = (_dev(fi, be), _dev(fe, be)) if with_src else (None, None)
        for scale in (1.0, DT):
            b = _rhs(p, be, T_STIM, scale)
            b_ref, S = ref.rhs(phi, n, m, h, T_STIM, f_i=fi if with_src else None, f_e=fe if with_src else None, scale=scale, with_magnitude=True)
            worst = (np.abs(b - b_ref) / np.maximum(S, 1e-300)).max()
            print(f"{mesh} {models} sources={with_src} s={scale:g}: max |db| / S = {worst:.3e} (|b|max {np.abs(b_ref).max():.3e})")
            assert np.abs(b_ref).max() > 0 and np.all(np.abs(b - b_ref) <= 1e-12 * S)
    be.f_i = be.f_e = None
    if models == "mixed":           # the second program matters: all-HH on the same facets and the same state gives another b
        b = _rhs(p, be)
        p2, be2, _ = cases(mesh, "hh")
        _random_state(p2, 7)
        be2.f_i = be2.f_e = None
        b_hh = _rhs(p2, be2)
        print(f"{mesh}: max|b_mixed - b_hh| / max|b_hh| = {np.abs(b - b_hh).max() / np.abs(b_hh).max():.3e}")
        assert np.abs(b - b_hh).max() > 1e-6 * np.abs(b_hh).max()


# ------------------------------------------------------------------------------------------ d. Dirichlet nodes on the membrane
def _dirichlet_nodes(ref, mesh, seed):
    """a random 5 % of all nodes, both nodes of ten membrane vertices and, where the mesh has one, of the hub on the membrane"""
    rng = np.random.default_rng(seed)
    nodes = list(rng.choice(ref.n, size=max(ref.n // 20, 1), replace=False))
    mv = np.unique(ref.fv)
    verts = list(rng.choice(mv, size=10, replace=False))
    if mesh == "hub3d_5_60m":
        verts.append(IM.hub_vertex(ref.coords, np.array(IM.MEMBRANE_HUB_3D) * 1e-6))
    for v in verts:
        assert ref.node_i[v] >= 0 and ref.node_e[v] >= 0
        nodes += [ref.node_i[v], ref.node_e[v]]
    return np.unique(np.array(nodes, dtype=np.int64))


@pytest.mark.parametrize("mesh", ["hub3d_5_60m", "delaunay2d_92"])
def test_dirichlet_nodes_on_the_membrane(cases, mesh):
    """masked columns in the ``gx`` loop of k_emi_spmv and the lifting ``s -= xval[q] * g[j]`` of k_emi_rhs"""
    p, be, ref = _problem(mesh, "hh", **IM.emi_config(cases.tmp, mesh))
    nodes = _dirichlet_nodes(ref, mesh, 31)
    g = np.zeros(ref.n)
    g[nodes] = np.random.default_rng(32).uniform(-0.01, 0.01, len(nodes))
    be.set_dirichlet(nodes, g[nodes])
    ref.set_dirichlet(nodes)
    Ae = ref.operator()
    # some other-side entry of a free membrane row points at a constrained node: the masked ``gx`` column is really there
    free = np.ones(ref.n, bool)
    free[nodes] = False
    cross = ref.absA_gamma.tocoo()
    cross_masked = free[cross.row] & ~free[cross.col] & (ref.node_side[cross.row] != ref.node_side[cross.col])
    assert cross_masked.sum() > 0
    phi, (n, m, h) = _random_state(p, 33)
    be.f_i = be.f_e = None
    b = _rhs(p, be)
    b_ref, S = ref.rhs(phi, n, m, h, T_STIM, g=g, with_magnitude=True)
    print(f"{mesh}: {len(nodes)} Dirichlet nodes, {cross_masked.sum()} masked cross entries, rhs max |db| / S = {(np.abs(b - b_ref) / np.maximum(S, 1e-300)).max():.3e}")
    assert np.all(np.abs(b - b_ref) <= 1e-12 * S) and np.array_equal(b[nodes], g[nodes])
    x = np.random.default_rng(34).standard_normal(ref.n)
    err, bound = np.abs(_spmv(be, x) - Ae @ x), abs(Ae) @ np.abs(x)
    print(f"{mesh}: eliminated SpMV max err / bound = {_worst(err, bound):.3e}")
    assert np.all(err <= 1e-12 * bound)
    assert abs(be.csr(eliminated=True) - Ae).max() <= 1e-12 * abs(Ae).max()
    if mesh == "hub3d_5_60m":
        _setup_pc(p, be, "hypre")
        be.x.zero_()
        its, rn, reason = be.cg(1e-12, max_it=2000, norm_type="preconditioned")
        xs = be.x.cpu().numpy()
        x_ref = ref.solve(b_ref)
        print(f"{mesh} dirichlet solve: {its} iterations, reason {reason}, max|dx| = {np.abs(xs - x_ref).max():.3e} of {np.abs(x_ref).max():.3e}")
        assert reason == CONVERGED_RTOL and np.array_equal(xs[nodes], g[nodes])
        assert np.allclose(xs, x_ref, rtol=1e-6, atol=1e-9)


# ------------------------------------------------------------------------------------------ e. k steps of PCG past every cap
def _k_steps(p, be, ref, pc, norm_type, x0=None, k=10, seed=41):
    """b random and mean-free, ``k`` iterations on the device and in the reference; the two ratios of the comparison"""
    b = np.random.default_rng(seed).standard_normal(ref.n)
    b -= b.mean()
    _setup_pc(p, be, pc)
    be.b.copy_(_dev(b, be))
    if x0 is None:
        be.x.zero_()
    else:
        be.x.copy_(_dev(x0, be))
    its, rn, reason = be.cg(0.0, atol=1e-300, max_it=k, norm_type=norm_type)
    x = be.x.cpu().numpy()
    x_ref, _, norms = ref.pcg(b, k, pc, norm_type, x0=x0)
    return its, rn, reason, x, np.abs(x - x_ref).max() / np.abs(x_ref).max(), abs(rn - norms[-1]) / norms[-1], norms


@pytest.mark.parametrize("norm_type", NORMS)
@pytest.mark.parametrize("pc", ["none", "jacobi"])
@pytest.mark.parametrize("mesh", ["delaunay2d_365", "delaunay2d_92"])
def test_ten_pcg_steps_against_the_reference(cases, mesh, pc, norm_type):
    """delaunay2d_365: five SpMV trips accumulate p . q, emi_sum_all adds 1024 and 512 partial sums in four and two trips, every
    vector kernel strides; delaunay2d_92: 277 partial sums of p . q (a ragged second trip of emi_sum_all) while the SpMV takes one"""
    p, be, ref = cases(mesh)
    its, rn, reason, x, dx, dn, norms = _k_steps(p, be, ref, pc, norm_type)
    print(f"{mesh} {pc} {norm_type}: max|dx| / max|x| = {dx:.3e}, norm {rn:.6e} (relative difference {dn:.3e}), first norm {norms[0]:.3e}")
    assert reason == DIVERGED_ITS and its == 10
    assert dx <= 1e-12 and dn <= 1e-10


@pytest.mark.parametrize("mesh", ["delaunay2d_365", "delaunay2d_92"])
def test_ten_pcg_steps_from_a_nearly_constant_guess(cases, mesh):
    """x0 constant per side up to 1e-6: A x0 is all rounding away from the membrane, its mean is taken out of the first residual"""
    p, be, ref = cases(mesh)
    x0 = np.where(ref.node_side == 0, 0.3, -0.2) + 1e-6 * np.random.default_rng(42).standard_normal(ref.n)
    its, rn, reason, x, dx, dn, norms = _k_steps(p, be, ref, "jacobi", "unpreconditioned", x0=x0)
    print(f"{mesh} from x0: max|dx| / max|x| = {dx:.3e}, norm {rn:.6e} (relative difference {dn:.3e})")
    assert reason == DIVERGED_ITS and its == 10
    assert dx <= 1e-12 and dn <= 1e-10
    assert np.abs(x - x0).max() > 1e-3 * np.abs(x0).max()         # the ten steps did move x


# ------------------------------------------------------------------------------------------ f. converged solves
@pytest.mark.parametrize("pc_type", ["hypre", "jacobi", "none"])
@pytest.mark.parametrize("mesh", SOLVE_MESHES)
def test_solve_reaches_the_true_residual(cases, mesh, pc_type):
    """test_gpu_emi.test_solve_reaches_the_true_residual on irregular matrices; ``hypre`` is the generic level-by-level V-cycle"""
    p, be, ref = cases(mesh)
    phi, (n, m, h) = _random_state(p, 21)
    be.f_i = be.f_e = None
    s = _setup_pc(p, be, pc_type, coarse_size=40)
    if pc_type == "hypre":
        rows = s.hierarchy.describe()["rows"]
        print(f"{mesh}: hierarchy rows {rows}")
        assert rows[0] == ref.n and (mesh != "delaunay2d_24" or len(rows) >= 3)
    b = _rhs(p, be)
    be.x.zero_()
    rtol = 1e-10
    its, rn, reason = be.cg(rtol, max_it=20000, norm_type="unpreconditioned")
    x = be.x.cpu().numpy()
    b_ref = ref.rhs(phi, n, m, h, T_STIM)
    res = np.linalg.norm(b_ref - ref.A @ x)
    print(f"{mesh} {pc_type}: {its} iterations, reason {reason}, reported {rn:.3e}, true {res:.3e}, rtol |b| = {rtol * np.linalg.norm(b_ref):.3e}")
    assert reason == CONVERGED_RTOL and its > 0
    assert res <= 2.0 * rtol * np.linalg.norm(b_ref)
    assert abs(x.mean()) <= 2e4 * 4 * np.finfo(float).eps * np.abs(x).max()


def test_hierarchy_solve_on_the_301_pair_row(cases):
    """hub2d_12_300 with the hierarchy, rtol 1e-10.  The solve must end with CONVERGED_RTOL.  b - A x is itself known to
    eps | |A| |x| | only, 3.1e-10 |b| on this mesh (host test), so that floor is added to the 2 rtol |b| of the other meshes.
    Before the coarse inverse left out the image of the constant this solve stagnated at 5.6e-8 |b| for 20000 iterations: the coarse
    operator built from the device's matrix kept that mode with an eigenvalue of 5.9e-12 against 1.3e-3."""
    mesh = "hub2d_12_300"
    p, be, ref = cases(mesh)
    phi, (n, m, h) = _random_state(p, 21)
    be.f_i = be.f_e = None
    s = _setup_pc(p, be, "hypre", coarse_size=40)
    b = _rhs(p, be)
    be.x.zero_()
    rtol = 1e-10
    its, rn, reason = be.cg(rtol, max_it=2000, norm_type="unpreconditioned")
    x = be.x.cpu().numpy()
    b_ref = ref.rhs(phi, n, m, h, T_STIM)
    nb = np.linalg.norm(b_ref)
    res = np.linalg.norm(b_ref - ref.A @ x)
    floor = np.finfo(float).eps * np.linalg.norm(abs(ref.A) @ np.abs(x))
    print(f"{mesh} hypre: rows {s.hierarchy.describe()['rows']}, {its} iterations, reason {reason}, reported {rn / nb:.3e} |b|, true {res / nb:.3e} |b|, floor {floor / nb:.3e} |b|")
    assert reason == CONVERGED_RTOL and its > 0 and rn <= rtol * nb * (1 + 1e-12)
    assert res <= 2.0 * rtol * nb + floor
    assert abs(x.mean()) <= 2e4 * 4 * np.finfo(float).eps * np.abs(x).max()


@pytest.mark.parametrize("mesh", SOLVE_MESHES + ["hub2d_12_300"])
def test_pc_apply_against_the_numpy_cycle(cases, mesh):
    """the generic level-by-level V-cycle (the only one the EMI path runs) against knpemi_oracle.pc_amg_vcycle on the hierarchy that
    was uploaded, with and without the projection of its output: 1e-10, the fp64 tolerance of
    test_gpu_irregular.test_pc_apply_against_the_numpy_cycle.  hub2d_12_300: a level-0 row of 301 entries."""
    import knpemi_oracle as K
    p, be, ref = cases(mesh)
    s = _setup_pc(p, be, "hypre", coarse_size=40)
    h = s.hierarchy
    assert len(h.levels) >= 2 and h.levels[0].A.shape[0] == ref.n
    cycle = K.pc_amg_vcycle(h.levels, h.coarse_inv, s.amg_sweeps, s.amg_sweeps, s.amg_cheby_degree)
    r = np.random.default_rng(3).standard_normal(ref.n)
    r -= r.mean()
    zo = cycle(r.copy())
    try:
        for ns, want in ((True, zo - zo.mean()), (False, zo)):
            be.set_nullspace(ns)
            z = torch.zeros(ref.n, dtype=torch.float64, device=be.device)
            be.pc_apply(_dev(r, be), z)
            d = np.abs(z.cpu().numpy() - want).max() / np.abs(want).max()
            print(f"{mesh}: rows {h.describe()['rows']}, null space {ns}: max|dz| / max|z| = {d:.3e}")
            assert d <= 1e-10
    finally:
        be.set_nullspace(True)


# ------------------------------------------------------------------------------------------ g. repeatability
def test_ten_steps_repeat_bitwise(cases):
    """the fixed grids are there for this: the same partial sums in the same order on every run"""
    p, be, ref = cases("delaunay2d_365")
    out = [_k_steps(p, be, ref, "jacobi", "preconditioned")[:4] for _ in range(2)]
    assert out[0][:3] == out[1][:3] and np.array_equal(out[0][3], out[1][3])


def test_converged_solve_repeats(cases):
    p, be, ref = cases("delaunay3d_7")
    _random_state(p, 23)
    be.f_i = be.f_e = None
    _setup_pc(p, be, "hypre")
    _rhs(p, be)
    out = []
    for _ in range(2):
        be.x.zero_()
        its, rn, reason = be.cg(1e-9, max_it=500, norm_type="unpreconditioned")
        out.append((its, rn, reason, be.x.clone()))
    assert out[0][2] == CONVERGED_RTOL and out[0][:3] == out[1][:3] and torch.equal(out[0][3], out[1][3])


# ------------------------------------------------------------------------------------------ h. knp_emi_update
@pytest.mark.parametrize("mesh", ["delaunay2d_365", "hub3d_5_60m"])
def test_update_splits_the_solution(cases, mesh):
    p, be, ref = cases(mesh)
    x = np.random.default_rng(51).standard_normal(ref.n)
    be.x.copy_(_dev(x, be))
    nv = p.mesh.num_vertices
    out = [torch.full((nv,), float("nan"), dtype=torch.float64, device=be.device) for _ in range(3)]
    be.update(*out)
    for got, want in zip(out, ref.split(x)):
        assert np.array_equal(got.cpu().numpy(), want)
