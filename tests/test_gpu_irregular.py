"""The node-graph kernels on irregular meshes (tests/irregular_meshes.py; preconditions in tests/test_irregular_meshes_host.py):
Delaunay meshes of a jittered grid, randomly renumbered, with and without a vertex of 26 to 301 pairs.  Every other GPU test runs on
generated grids, where no lane-group loop takes a second trip, only two lane widths are ever launched, the automatic choice of the
assembly kernel always lands on one branch, and all cells / membrane facets have one measure.

Operators are compared with the oracle on the same arrays, the preconditioner with the NumPy cycle on the hierarchy that was uploaded,
time steps with direct solves.  Tolerances are those of the structured-mesh tests named at each test.  No iteration counts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import irregular_meshes as IM
from parity_utils import fp32_stored, make_problem, run_native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [4, 8, 16, 32]


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _maxdiff(A, B):
    D = (A - B).tocoo()
    return np.abs(D.data).max() if D.nnz else 0.0


def _context(tmp_path, name, models="ci", dirichlet=False):
    """the native problem with its backend and the oracle on the same mesh, both in the perturbed state of test_gpu_parity._setup"""
    import knpemi_oracle as K
    cfg = IM.config(tmp_path, name)
    params = None
    if dirichlet:
        cfg["dirichlet_bcs"] = True
        cfg["initial_conditions"].update({"Na_i": 10, "Na_e": 145, "K_i": 130, "K_e": 3, "Cl_i": 5, "Cl_e": 134})
        params = K.Params(ki_init=K.OracleKNPEMI.REF_DEFAULT_KI, ke_init=K.OracleKNPEMI.REF_DEFAULT_KE)
    p = make_problem(cfg, models=models)
    be = p.create_backend()
    o = IM.oracle(name, models, params=params)
    IM.perturb(o, p)
    return p, be, o


def _set_time(p, o):
    o.t = o.p.dt
    o.update_t_mod()
    p.t.value = o.p.dt
    for m in p.ionic_models:
        if hasattr(m, "update_t_mod"):
            m.update_t_mod()


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """One context per mesh with the library's own launch choices (no environment switch), the matrix assembled, and the oracle's
    matrix next to it.  Shared by the tests that only read: none of them assembles again or writes a field."""
    cache = {}
    tmp = tmp_path_factory.mktemp("irregular")

    def get(name):
        if name not in cache:
            assert not [k for k in os.environ if k.startswith(("KNP_SPMV", "KNP_ASM", "KNP_PC_GROUP"))], "a shared context is built without switches"
            p, be, o = _context(tmp, name)
            be.assemble_matrix()
            cache[name] = (p, be, o, o.assemble_A().tocsr())
        return cache[name]
    return get


# ---- a. layout, operators, and the kernel the library chose ---------------------------------------------------------------------
@pytest.mark.parametrize("name", IM.EIGHT)
def test_layout_operators_and_launch_path(name, tmp_path):
    """test_gpu_parity.test_matrix_rhs_precond_match_oracle and test_gpu_fullsize.test_second_assembly_matches_oracle_entrywise on
    the irregular meshes; ``launch_info`` says which assembly kernel ran and how many trips its lane loop took."""
    p, be, o = _context(tmp_path, name)
    info = be.launch_info()
    print(name, info)
    IM.check_launch(info, name)
    assert info["spmv_unroll"] == 2 and info["spmv_mk"] == 1
    g = IM.graph_stats(o)
    assert info["max_node_pairs"] == g["pairs"].max() and info["max_node_cells"] == g["cells_per_node"].max()
    assert be.n_dof_owned == o.n_dof
    assert np.array_equal(be.node_i, o.lay.node_i.astype(np.int32))
    assert np.array_equal(be.node_e, o.lay.node_e.astype(np.int32))
    _set_time(p, o)
    be.assemble_matrix()
    A, Ao = be.csr(), o.assemble_A()
    assert A.shape == Ao.shape
    print("A", _maxdiff(A, Ao) / np.abs(Ao.data).max())
    assert _maxdiff(A, Ao) <= 1e-12 * np.abs(Ao.data).max()
    be.assemble_rhs()
    b, bo = be.b.cpu().numpy(), o.assemble_b()
    print("b", _rel(b, bo), [_rel(b[f::4], bo[f::4]) for f in range(4)])
    assert _rel(b, bo) <= 1e-12
    for f in range(4):
        assert _rel(b[f::4], bo[f::4]) <= 1e-10, f
    be.assemble_precond()
    P, Po = be.precond_csr(), o.assemble_P()
    print("P", _maxdiff(P, Po) / np.abs(Po.data).max())
    assert _maxdiff(P, Po) <= 1e-12 * np.abs(Po.data).max()
    # second assembly, other fields: only the entries that depend on the previous solution are rewritten
    X = o.coords / o.coords.max()
    s2 = 1.0 + 0.08 * np.cos(2.0 * X[:, 0] - 0.3) * np.sin(3.0 * X[:, 1] + 0.2)
    for side in range(2):
        for j in range(3):
            o.k[side][j] = o.k[side][j] * (s2 if (side + j) % 2 else 2.0 - s2)
            p.wh[side][j].x.array[:] = torch.as_tensor(o.k[side][j], device=p.mesh.device)
    be.assemble_matrix()
    A2, Ao2 = be.csr(), o.assemble_A()
    print("A second", _maxdiff(A2, Ao2) / np.abs(Ao2.data).max())
    assert _maxdiff(A2, Ao2) <= 1e-12 * np.abs(Ao2.data).max()
    assert _maxdiff(Ao2, Ao) > 1e-6 * np.abs(Ao.data).max()           # the fields did move the matrix


# ---- b. forced assembly variants and lane widths ----------------------------------------------------------------------------------
def _assembled(tmp_path, name):
    p, be, o = _context(tmp_path, name)
    be.assemble_matrix()
    be.assemble_precond()
    return be.csr(), be.precond_csr(), be.launch_info(), o


@pytest.mark.parametrize("name", ["hub2d_12_40", "delaunay3d_5"])
def test_assembly_variants_write_the_same_bits(name, tmp_path, monkeypatch):
    """test_gpu_fullsize.test_assembly_variants_write_the_same_bits where the lane loops take several trips and the self pair sits in
    a later one; and the fused cell means (sums in the cell's vertex order, like k_cell_means) write the bits of the unfused form."""
    A1, P1, i1, _ = _assembled(tmp_path, name)
    IM.check_launch(i1, name)
    monkeypatch.setenv("KNP_ASM_FUSED_MEANS", "0")
    Af, Pf, inf, _ = _assembled(tmp_path, name)
    monkeypatch.delenv("KNP_ASM_FUSED_MEANS")
    assert i1["asm_dmax"] > 0 and inf["asm_dmax"] == 0 and inf["asm_variant"] == i1["asm_variant"]
    monkeypatch.setenv("KNP_ASM_TRANSPOSED", "0")
    A2, P2, i2, _ = _assembled(tmp_path, name)
    monkeypatch.setenv("KNP_ASM_STAGE", "0")
    A3, P3, i3, _ = _assembled(tmp_path, name)
    assert i2["asm_variant"] == 1 and i3["asm_variant"] == 0 and i3["asm_stage"] == 0
    print(name, "plain vs staged: A", np.abs(A3.data - A1.data).max() / np.abs(A1.data).max(),
          "P", np.abs(P3.data - P1.data).max() / np.abs(P1.data).max())
    assert np.array_equal(Af.indices, A1.indices) and np.array_equal(Af.data, A1.data)
    assert np.array_equal(Pf.indices, P1.indices) and np.array_equal(Pf.data, P1.data)
    assert np.array_equal(A2.indices, A1.indices) and np.array_equal(A2.data, A1.data)
    assert np.array_equal(P2.indices, P1.indices) and np.array_equal(P2.data, P1.data)
    assert np.array_equal(A3.indices, A1.indices) and np.abs(A3.data - A1.data).max() <= 1e-15 * np.abs(A1.data).max()
    assert np.array_equal(P3.indices, P1.indices) and np.abs(P3.data - P1.data).max() <= 1e-15 * np.abs(P1.data).max()


@pytest.mark.parametrize("G", WIDTHS)
@pytest.mark.parametrize("name", ["hub2d_12_40", "delaunay3d_5"])
def test_plain_assembly_at_every_lane_width(name, G, tmp_path, monkeypatch):
    """k_assemble_nodes<G> for G = 4, 8, 16, 32 (KNP_ASM_GROUP applies to the unstaged kernel): 11 to 2 trips at the hub"""
    monkeypatch.setenv("KNP_ASM_STAGE", "0")
    monkeypatch.setenv("KNP_ASM_GROUP", str(G))
    A, P, info, o = _assembled(tmp_path, name)
    assert info["asm_variant"] == 0 and info["asm_group"] == G
    Ao, Po = o.assemble_A(), o.assemble_P()
    print(name, G, "A", _maxdiff(A, Ao) / np.abs(Ao.data).max(), "P", _maxdiff(P, Po) / np.abs(Po.data).max())
    assert _maxdiff(A, Ao) <= 1e-12 * np.abs(Ao.data).max()
    assert _maxdiff(P, Po) <= 1e-12 * np.abs(Po.data).max()


# ---- c. SpMV ------------------------------------------------------------------------------------------------------------------------
def _check_spmv(be, o, Ao, what):
    """row by row, |y - Ao x|_i <= 1e-12 (|Ao| |x|)_i (the bound of test_gpu_emi.test_spmv_against_the_reference: a 301-term row
    next to 4-term rows); null-space test and projection as in test_gpu_parity.test_spmv_and_nullspace"""
    x = np.random.default_rng(0).standard_normal(o.n_dof)
    xt = torch.as_tensor(x, device=be.device)
    yt = torch.empty_like(xt)
    be.spmv(xt, yt)
    err = np.abs(yt.cpu().numpy() - Ao @ x)
    bound = abs(Ao) @ np.abs(x)
    print(f"{what}: SpMV max err / bound = {(err / bound).max():.3e}, worst row {int(np.argmax(err / bound))}")
    assert np.all(err <= 1e-12 * bound)
    return x


@pytest.mark.parametrize("G", [None] + WIDTHS)
@pytest.mark.parametrize("name", IM.EIGHT)
def test_spmv_rowwise_at_every_lane_width(name, G, cases, tmp_path, monkeypatch):
    if G is None:
        p, be, o, Ao = cases(name)
        assert be.launch_info()["spmv_group"] == IM.EXPECT[name]["asm_group"] // 2
    else:
        monkeypatch.setenv("KNP_SPMV", str(G))
        p, be, o = _context(tmp_path, name)
        be.assemble_matrix()
        Ao = o.assemble_A().tocsr()
    info = be.launch_info()
    assert info["spmv_group"] == (G or info["spmv_group"]) and info["spmv_mk"] == 1 and info["spmv_unroll"] == 2
    x = _check_spmv(be, o, Ao, f"{name} G={info['spmv_group']} trips={-(-info['max_node_pairs'] // (2 * info['spmv_group']))}")
    assert be.nullspace_test() <= 1e-10 * np.abs(Ao.data).max()
    v = torch.as_tensor(x.copy(), device=be.device)
    be.project_nullspace(v)
    ns = o.nullspace()
    assert _rel(v.cpu().numpy(), x - ns * (ns @ x)) <= 1e-13


def test_spmv_with_dirichlet_rows_reads_the_stored_entries(tmp_path):
    """The configuration of test_gpu_parity.test_dirichlet_bcs_without_mms: identity rows on the exterior boundary, so the SpMV reads
    the stored time-invariant entries instead of {M, K} per pair (``spmv_mk`` 0)."""
    import scipy.sparse as sp
    name = "delaunay2d_12"
    p, be, o = _context(tmp_path, name, dirichlet=True)
    be.assemble_matrix()
    info = be.launch_info()
    assert info["spmv_mk"] == 0 and -(-info["max_node_pairs"] // (2 * info["spmv_group"])) == 2
    x = o.coords / o.coords.max()
    bv = np.nonzero(np.any((np.abs(x) < 1e-12) | (np.abs(x - 1.0) < 1e-12), axis=1))[0]
    dofs, _ = o.dirichlet_initial_values(bv)
    assert len(dofs) == 4 * len(bv) and set(dofs.tolist()) == set(be.bc_dofs.cpu().numpy().tolist())
    Ao = o.assemble_A().tocsr()
    keep = np.ones(o.n_dof)
    keep[dofs] = 0.0
    Ar = (sp.diags(keep) @ Ao + sp.diags(1.0 - keep)).tocsr()
    _check_spmv(be, o, Ar, name + " Dirichlet")


def test_spmv_with_one_pair_in_flight(tmp_path):
    """KNP_SPMV_UNROLL is read once per process: a fresh child runs k_spmv_node<G, ., ., 1> on the 41-pair hub (11 trips of 4 lanes)
    and hands back y (the _run_in_subprocess pattern of test_gpu_parity)."""
    name = "hub2d_12_40"
    code = ("import sys; sys.path[:0]=['tests','oracle','knp-emi-cgx_amd']; import conftest, json, numpy as np, torch\n"
            "import irregular_meshes as IM\n"
            "from parity_utils import make_problem\n"
            f"p = make_problem(IM.config(sys.argv[1], '{name}'))\n"
            "be = p.create_backend()\n"
            f"o = IM.oracle('{name}'); IM.perturb(o, p)\n"
            "be.assemble_matrix()\n"
            "x = torch.as_tensor(np.random.default_rng(0).standard_normal(o.n_dof), device=be.device)\n"
            "y = torch.empty_like(x); be.spmv(x, y)\n"
            "print('RESULT' + json.dumps({'y': y.cpu().numpy().tolist(), 'info': be.launch_info()}))\n")
    out = subprocess.run([sys.executable, "-c", code, str(tmp_path)], cwd=ROOT, env=dict(os.environ, KNP_SPMV_UNROLL="1"),
                         capture_output=True, text=True, timeout=300)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
    assert line, out.stdout[-2000:] + out.stderr[-2000:]
    res = json.loads(line[0][6:])
    assert res["info"]["spmv_unroll"] == 1 and res["info"]["spmv_group"] == 4 and res["info"]["max_node_pairs"] == 41
    o = IM.oracle(name)
    IM.perturb(o)
    Ao = o.assemble_A().tocsr()
    x = np.random.default_rng(0).standard_normal(o.n_dof)
    err = np.abs(np.array(res["y"]) - Ao @ x)
    bound = abs(Ao) @ np.abs(x)
    print(f"unroll 1: SpMV max err / bound = {(err / bound).max():.3e}")
    assert np.all(err <= 1e-12 * bound)


# ---- d. preconditioner application against the NumPy cycle on the uploaded hierarchy ----------------------------------------------
COARSE = {"delaunay2d_24": 12, "delaunay3d_7": 12}


def _pc_solver(tmp_path, name, pc, fp32):
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    cfg = IM.config(tmp_path, name, pc=pc)
    ks = cfg["solver"]["ksp_settings"]
    ks["amg_coarse_size"], ks["amg_fp32"], ks["amg_setup"] = COARSE[name], fp32, "host"
    p = make_problem(cfg)
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    s.setup_solver()
    be = s.backend
    o = IM.oracle(name)
    IM.perturb(o, p)
    p.setup_preconditioner(s.use_block_Jacobi)
    s.assemble_preconditioner()
    _set_time(p, o)
    be.assemble_rhs()
    be.assemble_matrix()
    be.pc_setup(s._pc_kind)
    return s, be, o


def _numpy_cycle(s, o, pc, fp32, fused):
    import knpemi_oracle as K
    if pc == "btcc":
        hk, hp = s.hierarchies
        if fp32:
            hk, hp = fp32_stored(hk, coarse=fused), fp32_stored(hp, level0_uploaded=s._coupled_phi)
        return K.pc_btcc(o, hk, hp, s.amg_pre, s.amg_post, s.amg_cheby_degree, fused=fused)
    h = fp32_stored(s.hierarchy) if fp32 else s.hierarchy
    return K.pc_amg_vcycle(h.levels, h.coarse_inv, s.amg_pre, s.amg_post, s.amg_cheby_degree, fused=fused)


@pytest.mark.parametrize("G", [None] + WIDTHS)
@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("pc", ["hypre", "btcc"])
@pytest.mark.parametrize("name", ["delaunay2d_24", "delaunay3d_7"])
def test_pc_apply_against_the_numpy_cycle(name, pc, fp32, G, tmp_path, monkeypatch):
    """``pc_apply`` on a random residual against knpemi_oracle.pc_amg_vcycle / pc_btcc on the host hierarchy that was uploaded
    (fp32 storage: rounded by ``fp32_stored`` as oracle_gmres_same_algorithm does), per field block: 1e-10 with fp64 storage, 2e-6
    with fp32 (the tolerances of test_fused_cycle_is_the_same_operator_as_the_unfused_cycle, here against the oracle).  The fused
    cycle, the level-by-level cycle (KNP_FUSED=0: k_pnode) and the scalar-row form (KNP_BLOCKED=0), at every lane width of the
    level-0 kernels; the right-hand side (k_rhs<G>, the same switch) with the assertion of test_matrix_rhs_precond_match_oracle."""
    if G is not None:
        monkeypatch.setenv("KNP_PC_GROUP", str(G))
    s, be, o = _pc_solver(tmp_path, name, pc, fp32)
    info = be.launch_info()
    assert info["pc_group"] == (G or IM.EXPECT[name]["asm_group"] // 2)
    assert all(len(h.levels) >= 3 for h in s.hierarchies), [len(h.levels) for h in s.hierarchies]
    # the right-hand side kernel k_rhs<G> takes its lanes per node from the same switch
    b, bo = be.b.cpu().numpy(), o.assemble_b()
    assert _rel(b, bo) <= 1e-12 and all(_rel(b[f::4], bo[f::4]) <= 1e-10 for f in range(4))
    r = np.random.default_rng(3).standard_normal(be.n_dof_owned)
    rt = torch.as_tensor(r, device=be.device)
    tol = 2e-6 if fp32 else 1e-10
    seen = []
    for switch in (None, "KNP_BLOCKED", "KNP_FUSED"):
        if switch:
            monkeypatch.setenv(switch, "0")
            be.pc_setup(s._pc_kind)
        st = be.stats()
        seen.append((st["fused"], st["blocked"]))
        z = torch.zeros_like(rt)
        be.pc_apply(rt, z)
        z = z.cpu().numpy()
        zo = _numpy_cycle(s, o, pc, fp32, bool(st["fused"]))(r.copy())
        d = [np.max(np.abs(z[f::4] - zo[f::4])) / np.max(np.abs(zo[f::4])) for f in range(4)]
        print(f"{name} {pc} fp32={fp32} G={info['pc_group']} fused={st['fused']} blocked={st['blocked']}: {d}")
        for f in range(4):
            assert d[f] <= tol, (switch, f, d)
    # node-blocked operators exist with fp32 storage only; the fused cycle runs either way
    assert seen[0][0] > 0 and (seen[0][1] > 0) == fp32 and seen[1] == (seen[0][0], 0) and seen[2][0] == 0, seen


def test_pc_apply_vbjacobi_inverts_vertex_blocks_at_the_hub(tmp_path):
    """test_gpu_parity.test_pc_apply_vbjacobi_inverts_vertex_blocks where one vertex block gathers 41 pairs (k_vbj_extract)"""
    p, be, o = _context(tmp_path, "hub2d_12_40")
    be.assemble_matrix()
    be.pc_setup(1)
    A = be.csr().tocsr()
    r = np.random.default_rng(1).standard_normal(o.n_dof)
    rt = torch.as_tensor(r, device=be.device)
    zt = torch.zeros_like(rt)
    be.pc_apply(rt, zt)
    z = zt.cpu().numpy()
    grp = o.lay.node_vertex
    starts = np.nonzero(np.r_[True, grp[1:] != grp[:-1]])[0]
    sizes = np.diff(np.r_[starts, o.lay.n_nodes])
    assert sizes.max() == 2
    for s, sz in zip(starts, sizes):
        idx = np.arange(4 * s, 4 * (s + sz))
        blk = A[idx][:, idx].toarray()
        assert np.allclose(blk @ z[idx], r[idx], rtol=1e-9, atol=1e-12 * np.abs(r).max())


# ---- e. two steps against direct solves ---------------------------------------------------------------------------------------------
def _step_config(tmp_path, name, pc, rtol=1e-13):
    cfg = IM.config(tmp_path, name, steps=2, rtol=rtol, pc=pc)
    cfg["solver"]["ksp_settings"]["ksp_max_it"] = 5000
    cfg["solver"]["ksp_settings"]["amg_coarse_size"] = 100
    return cfg


@pytest.fixture(scope="module")
def stepped():
    """the oracle after two lu_gauge steps, once per mesh"""
    cache = {}

    def get(name):
        if name not in cache:
            o = IM.oracle(name)
            o.run(2, solver="lu_gauge")
            cache[name] = o
        return cache[name]
    return get


@pytest.mark.parametrize("pc", ["hypre", "btcc"])
@pytest.mark.parametrize("name", ["delaunay2d_12", "hub2d_12_48m", "delaunay3d_5"])
def test_two_steps_match_direct_solves(name, pc, stepped, tmp_path):
    """the assertions of test_gpu_xdmf.test_run_from_xdmf_files_matches_oracle_on_the_same_arrays"""
    s = run_native(_step_config(tmp_path, name, pc))
    assert all(r > 0 for r in s.reasons), s.reasons
    o = stepped(name)
    ni, ne = s.potential_norms()
    oi, oe = o.potential_norms()
    gam = (o.lay.node_i >= 0) & (o.lay.node_e >= 0)
    phim = s.problem.phi_m_prev.numpy()
    print(name, pc, "its", list(s.iterations), "phi_i", abs(ni - oi) / oi, "phi_e", abs(ne - oe) / oe,
          "phi_m", np.max(np.abs(phim[gam] / o.phi_m[gam] - 1.0)))
    assert abs(ni - oi) <= 1e-6 * oi and abs(ne - oe) <= 1e-5 * oe
    assert np.allclose(phim[gam], o.phi_m[gam], rtol=1e-6)
    vi, ve = o.lay.node_i >= 0, o.lay.node_e >= 0
    for j in range(3):
        assert np.allclose(s.problem.wh[0][j].numpy()[vi], o.k[0][j][vi], rtol=1e-7)
        assert np.allclose(s.problem.wh[1][j].numpy()[ve], o.k[1][j][ve], rtol=1e-7)


@pytest.mark.parametrize("name,pc", [("hub2d_12_48m", "hypre"), ("delaunay3d_5", "btcc")])
def test_flexible_gmres_reaches_the_true_residual(name, pc, tmp_path):
    """k_spmv_node_dots (the SpMV with the first reduction stage of flexible GMRES in its epilogue) over several trips: the true
    residual, recomputed through knp_spmv, meets the tolerance the solver reports -- the assertion of
    test_gpu_fgmres.test_true_residual_at_benchmarked_sizes."""
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    from test_gpu_fgmres import FLEX, MARGIN, _true_res, _wrap
    rtol = 1e-9
    cfg = _step_config(tmp_path, name, pc, rtol=rtol)
    cfg["solver"]["ksp_settings"].update(FLEX)
    p = make_problem(cfg)
    p.solver_config["view_ksp"] = False
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    rec = _wrap(s, _true_res)
    s.solve()
    print(name, pc, rec, s.backend.stats())
    assert s._flexible and len(rec) == 2 and s.backend.stats()["spmv_dots"] > 0
    for r in rec:
        assert r["reason"] == 2 and r["true"] <= MARGIN * rtol, r


def test_morton_vertex_order_gives_the_same_solution(tmp_path):
    """test_gpu_parity.test_morton_vertex_order_gives_the_same_solution from a random numbering, with the hub on the membrane"""
    name, pc = "hub2d_12_48m", "btcc"
    s0 = run_native(_step_config(tmp_path, name, pc, rtol=1e-12))
    cfg1 = _step_config(tmp_path, name, pc, rtol=1e-12)
    cfg1["vertex_order"] = "morton"
    s1 = run_native(cfg1)
    p0, p1 = s0.problem, s1.problem
    assert "Morton" in p1.mesh_description and not np.array_equal(p0.local_mesh.l2g, p1.local_mesh.l2g)
    assert all(r > 0 for r in s0.reasons) and all(r > 0 for r in s1.reasons)
    o0, o1 = np.argsort(p0.local_mesh.l2g), np.argsort(p1.local_mesh.l2g)
    assert np.allclose(p0.local_mesh.coords[o0], p1.local_mesh.coords[o1])
    pot_scale = np.abs(p0.wh[0][3].numpy()).max()
    for side in (0, 1):
        for f in range(4):
            a, b = p0.wh[side][f].numpy()[o0], p1.wh[side][f].numpy()[o1]
            tol = 1e-6 * pot_scale if f == 3 else 1e-7 * max(np.abs(a).max(), 1e-300)
            assert np.abs(a - b).max() <= tol, (side, f, np.abs(a - b).max(), tol)
    pm0, pm1 = p0.phi_m_prev.numpy()[o0], p1.phi_m_prev.numpy()[o1]
    assert np.abs(pm0 - pm1).max() <= 1e-6 * np.abs(pm0).max()
    n0, n1 = s0.potential_norms(), s1.potential_norms()
    assert abs(n0[0] - n1[0]) <= 1e-6 * n0[0] and abs(n0[1] - n1[1]) <= 1e-6 * n0[0]


# ---- f. the EMI model ------------------------------------------------------------------------------------------------------------------
EMI_MESHES = ["delaunay2d_12", "hub2d_12_40", "delaunay3d_5"]


def _emi_problem(tmp_path, name, models):
    from test_gpu_emi import _problem
    path = IM.write_npz(tmp_path, name, *IM.mesh(name))
    return _problem(name, models, cell_tag_file=path, facet_tag_file=path, input_dir="")


@pytest.mark.parametrize("name", EMI_MESHES)
def test_emi_matrix_and_spmv_against_the_reference(name, tmp_path):
    """test_gpu_emi.test_matrix_against_the_reference (with its symmetry) and test_spmv_against_the_reference"""
    from test_gpu_emi import _dev
    p, be, ref = _emi_problem(tmp_path, name, "hh")
    info = be.launch_info()
    assert info["max_node_pairs"] > info["emi_group"]                 # a second trip of k_emi_spmv's pair loop
    A = be.csr()
    amax = abs(ref.A).max()
    d, asym = abs(A - ref.A).max(), abs(A - A.T).max()
    print(f"{name}: n = {ref.n}, max|dA| / max|A| = {d / amax:.3e}, max|A - A^T| / max|A| = {asym / amax:.3e}, {info}")
    assert A.shape == ref.A.shape and d <= 1e-12 * amax and asym <= 1e-12 * amax
    x = np.random.default_rng(1).standard_normal(ref.n)
    y = torch.empty(ref.n, dtype=torch.float64, device=be.device)
    be.spmv(_dev(x, be), y)
    err = np.abs(y.cpu().numpy() - ref.A @ x)
    bound = abs(ref.A) @ np.abs(x)
    print(f"{name}: SpMV max err / bound = {(err / bound).max():.3e}")
    assert np.all(err <= 1e-12 * bound)


@pytest.mark.parametrize("models", ["passive", "hh"])
@pytest.mark.parametrize("name", EMI_MESHES)
def test_emi_rhs_against_the_reference(name, models, tmp_path):
    """test_gpu_emi.test_rhs_against_the_reference: facet measures enter the membrane term, lumped pair masses the sources"""
    from test_gpu_emi import DT, T_STIM, _dev, _random_state, _rhs
    p, be, ref = _emi_problem(tmp_path, name, models)
    phi, gates = _random_state(p, 7)
    n, m, h = gates if hasattr(p, "n") else (None, None, None)
    rng = np.random.default_rng(8)
    fi, fe = rng.standard_normal(p.mesh.num_vertices), rng.standard_normal(p.mesh.num_vertices)
    for with_src in (False, True):
        be.f_i, be.f_e = (_dev(fi, be), _dev(fe, be)) if with_src else (None, None)
        for scale in (1.0, DT):
            b = _rhs(p, be, T_STIM, scale)
            b_ref, S = ref.rhs(phi, n, m, h, T_STIM, f_i=fi if with_src else None, f_e=fe if with_src else None, scale=scale, with_magnitude=True)
            worst = (np.abs(b - b_ref) / np.maximum(S, 1e-300)).max()
            print(f"{name} {models} sources={with_src} s={scale:g}: max |db| / S = {worst:.3e}")
            assert np.abs(b_ref).max() > 0 and np.all(np.abs(b - b_ref) <= 1e-12 * S)


# ---- g. per-tag diagnostics on non-uniform geometry ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_tag(tmp_path_factory):
    """delaunay3d(5) with two cells (tags 2, 3) and random nodal fields, no time step"""
    from test_gpu_fluxes import _random_fields
    p = make_problem(IM.two_tag_config(tmp_path_factory.mktemp("two_tag")), "ci")
    be = p.create_backend()
    _random_fields(p, 11)
    assert [int(t) for t in p.gamma_tags] == [2, 3]
    return p, be


@pytest.mark.parametrize("what", ["ion_amounts", "fluxes", "membrane_potential"])
def test_per_tag_diagnostics_on_cells_and_facets_of_many_sizes(what, two_tag):
    """k_diag_cells / k_diag_fluxes / k_diag_phim where cell volumes span a factor of 85 and facet areas a factor of 4: against
    the host integrals of test_gpu_ion_budget, flux_ref and phim_ref, with the tolerances of those files"""
    p, be = two_tag
    tags = [int(t) for t in p.gamma_tags]
    if what == "ion_amounts":
        from test_gpu_ion_budget import _host_budget
        ctags, host = _host_budget(p)
        assert np.array_equal(be.budget_layout().tags, ctags) and list(ctags) == [2, 3, 1]
        got = be.ion_amounts().cpu().numpy()
        print("ion amounts: max rel. difference", np.abs(got / host - 1.0).max())
        assert np.allclose(got, host, rtol=1e-12, atol=0)
    elif what == "fluxes":
        from test_gpu_fluxes import _close, _reference
        out = p.membrane_fluxes()
        ref, S, cover = _reference(p, [[t] for t in tags], False)
        assert list(out["tag"]) == tags and min(len(c) for c in cover) >= 20
        assert np.all(S > 0) and np.all(np.abs(ref) > 0)
        assert _close(out["flux_i"], ref[:, 0], S[:, 0]) and _close(out["flux_e"], ref[:, 1], S[:, 1])
        lm = p.local_mesh
        for t, tag in enumerate(tags):
            assert out["area"][t] == pytest.approx(p._fmeas[np.asarray(lm.gamma_tags) == tag].sum(), rel=1e-13)
    else:
        from phim_ref import phim_ref
        from test_gpu_membrane_potential import _check_device
        phi = p.phi_m_prev.numpy().copy()
        out = p.membrane_potential()
        ref = phim_ref(p, phi, [[t] for t in tags])
        I, A, lo, hi, S, cover = ref
        assert list(out["tag"]) == tags and np.all(S > 0) and np.all(lo < hi)
        got = be.membrane_potential().cpu().numpy()
        _check_device(got, ref, "two-tag delaunay3d(5)")
        assert np.allclose(out["area"], A, rtol=1e-13, atol=0)
        assert np.array_equal(out["min"], lo) and np.array_equal(out["max"], hi)
