"""The EMI model on the GPU (knp_emi_* in csrc/knp_emi.inc, ProblemEMI / SolverEMI) against tests/emi_ref.py, the independent
NumPy / SciPy restatement pinned by tests/test_emi_host.py.  Meshes: square8, square16, cube4 and the 2D tissue lattice
tissue2d_18_3 (nine cells, nine membrane tags, two membrane models)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import emi_ref

pytestmark = pytest.mark.gpu

MESHES = ["square8", "square16", "cube4", "tissue2d_18_3"]
DT, CM, SI, SE = 5e-5, 0.02, 0.7, 1.3
T_STIM = 0.003          # g_syn(0.003) = 40 exp(-1.5): the stimulus constant of the HH program is non-zero


def _config(mesh, **kw):
    cfg = {"problem_type": "EMI", "dt": DT, "time_steps": 1, "C_M": CM, "sigma_i": SI, "sigma_e": SE, "quiet": True,
           "cell_tag_file": mesh + ".xdmf", "facet_tag_file": mesh + ".xdmf", "mesh_conversion_factor": 1e-6}
    if mesh.startswith("tissue"):
        cfg.update(ics_tags=list(range(2, 11)), ecs_tags=[1], membrane_tags=list(range(2, 11)))
    else:
        cfg.update(ics_tags=[1], ecs_tags=[2], membrane_tags=[4])
    cfg.update(kw)
    return cfg


def _problem(mesh, models="hh", **kw):
    """ProblemEMI with its context and programs on the device, and the reference built from the same mesh arrays"""
    from cgx_hip.emi_models import g_syn
    from cgx_hip.emi_problem import ProblemEMI
    p = ProblemEMI(_config(mesh, **kw))
    tags = p.gamma_tags
    if models == "hh":
        p.add_ionic_model("HH", stim_fun=g_syn)
    elif models == "passive":
        p.add_ionic_model("Passive")
    else:                                   # two programs on one membrane: HH on the even tags, passive on the odd ones
        p.add_ionic_model("HH", tags=tuple(t for t in tags if t % 2 == 0), stim_fun=g_syn)
        p.add_ionic_model("Passive", tags=tuple(t for t in tags if t % 2 == 1))
    p.init_ionic_model()
    p.setup_bilinear_form()
    p.setup_linear_form()
    lm = p.local_mesh
    model_of_tag = {int(t): k for k, m in enumerate(p.ionic_models) for t in m.tags}
    ref = emi_ref.EmiRef(lm.coords, lm.cells, p.cell_side, lm.gamma, float(p.dt.value), p.C_M, p.sigma_i, p.sigma_e,
                         facet_model=[model_of_tag[int(t)] for t in lm.gamma_tags])
    ref.models = [emi_ref.hh_current if str(m) == "Hodgkin-Huxley" else emi_ref.passive_current for m in p.ionic_models]
    ref.nullspace = not p.dirichlet_bcs
    if p.dirichlet_bcs:
        ref.set_dirichlet(ref.exterior_extra_nodes())
    be = p.backend
    assert be.n_nodes == ref.n and np.array_equal(be.node_i, ref.node_i) and np.array_equal(be.node_e, ref.node_e)
    return p, be, ref


def _random_state(p, seed):
    """phi_M in +-0.1 V, gates in (0, 1)"""
    rng = np.random.default_rng(seed)
    nv = p.mesh.num_vertices
    phi = rng.uniform(-0.1, 0.1, nv)
    gates = [rng.uniform(0.01, 0.99, nv) for _ in range(3)]
    dev = p.mesh.device
    p.phi_M.x.array[:] = torch.as_tensor(phi, device=dev)
    if hasattr(p, "n"):
        for f, g in zip((p.n, p.m, p.h), gates):
            f.x.array[:] = torch.as_tensor(g, device=dev)
    return phi, gates


def _rhs(p, be, t=T_STIM, scale=1.0):
    for m in p.ionic_models:
        m.refresh(t)
    be.refresh_program_constants()
    be.assemble_rhs(scale)
    return be.b.cpu().numpy()


def _dev(a, be):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=be.device)


@pytest.fixture(scope="module")
def cases():
    """one problem per mesh (HH; both models on the tissue lattice), shared by the matrix / SpMV / solve tests"""
    cache = {}

    def get(mesh):
        if mesh not in cache:
            cache[mesh] = _problem(mesh, "mixed" if mesh.startswith("tissue") else "hh")
        return cache[mesh]
    return get


# ------------------------------------------------------------------------------------------ matrix
@pytest.mark.parametrize("mesh", MESHES)
def test_matrix_against_the_reference(cases, mesh):
    p, be, ref = cases(mesh)
    A = be.csr()
    amax = abs(ref.A).max()
    d, asym = abs(A - ref.A).max(), abs(A - A.T).max()
    print(f"{mesh}: n = {ref.n}, nnz = {A.nnz}, max|A| = {amax:.3e}, max|dA| = {d:.3e}, max|A - A^T| = {asym:.3e}")
    assert A.shape == ref.A.shape and d <= 1e-12 * amax and asym <= 1e-12 * amax
    # another dt rewrites the values; back again for the tests that share the context
    lm = p.local_mesh
    ref2 = emi_ref.EmiRef(lm.coords, lm.cells, p.cell_side, lm.gamma, 3.0 * DT, p.C_M, p.sigma_i, p.sigma_e)
    be.setup(3.0 * DT, p.C_M, p.sigma_i, p.sigma_e)
    A2 = be.csr()
    be.setup(DT, p.C_M, p.sigma_i, p.sigma_e)
    d2, asym2 = abs(A2 - ref2.A).max(), abs(A2 - A2.T).max()
    print(f"{mesh}: dt x 3: max|dA| = {d2:.3e}, max|A - A^T| = {asym2:.3e}")
    assert d2 <= 1e-12 * abs(ref2.A).max() and asym2 <= 1e-12 * abs(ref2.A).max()
    assert abs(be.csr() - A).max() == 0.0


@pytest.mark.parametrize("mesh", MESHES)
def test_spmv_against_the_reference(cases, mesh):
    p, be, ref = cases(mesh)
    x = np.random.default_rng(1).standard_normal(ref.n)
    y = torch.empty(ref.n, dtype=torch.float64, device=be.device)
    be.spmv(_dev(x, be), y)
    err = np.abs(y.cpu().numpy() - ref.A @ x)
    bound = abs(ref.A) @ np.abs(x)
    print(f"{mesh}: SpMV max err / bound = {(err / bound).max():.3e}")
    assert np.all(err <= 1e-12 * bound)


# ------------------------------------------------------------------------------------------ right-hand side
@pytest.mark.parametrize("mesh,models", [(m, k) for m in MESHES for k in ("passive", "hh")] + [("tissue2d_18_3", "mixed")])
def test_rhs_against_the_reference(mesh, models):
    p, be, ref = _problem(mesh, models)
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
            print(f"{mesh} {models} sources={with_src} s={scale:g}: max |db| / S = {worst:.3e} (|b|max {np.abs(b_ref).max():.3e})")
            assert np.abs(b_ref).max() > 0 and np.all(np.abs(b - b_ref) <= 1e-12 * S)


def test_rhs_with_dirichlet_lifting():
    p, be, ref = _problem("square16", "hh", dirichlet_bcs=True)
    phi, (n, m, h) = _random_state(p, 9)
    g = np.zeros(ref.n)
    g[ref.bc_nodes] = np.random.default_rng(10).uniform(-0.01, 0.01, len(ref.bc_nodes))
    be.set_dirichlet_values(g[be.bc_nodes.cpu().numpy()])
    b = _rhs(p, be)
    b_ref, S = ref.rhs(phi, n, m, h, T_STIM, g=g, with_magnitude=True)
    assert np.array_equal(np.sort(be.bc_nodes.cpu().numpy()), np.sort(ref.bc_nodes))
    assert np.all(np.abs(b - b_ref) <= 1e-12 * S) and np.array_equal(b[ref.bc_nodes], g[ref.bc_nodes])
    # the operator: identity on the constrained nodes, rows and columns
    x = np.random.default_rng(11).standard_normal(ref.n)
    y = torch.empty(ref.n, dtype=torch.float64, device=be.device)
    be.spmv(_dev(x, be), y)
    Ae = ref.operator()
    assert np.all(np.abs(y.cpu().numpy() - Ae @ x) <= 1e-12 * (abs(Ae) @ np.abs(x)))
    assert abs(be.csr(eliminated=True) - Ae).max() <= 1e-12 * abs(Ae).max()


# ------------------------------------------------------------------------------------------ solve
def _setup_pc(p, be, pc_type, coarse_size=40):
    from cgx_hip.emi_solver import SolverEMI

    class S(SolverEMI):
        pass
    S.pc_type = pc_type
    S.amg_coarse_size = coarse_size          # 40: several levels on every test mesh (cube4 has 151 unknowns)
    s = S.__new__(S)
    s.problem, s.backend, s.comm, s.direct_solver = p, be, p.comm, False
    p.P = None
    s.setup_solver()
    return s


@pytest.mark.parametrize("pc_type", ["hypre", "jacobi", "none"])
@pytest.mark.parametrize("mesh", ["square16", "cube4", "tissue2d_18_3"])
def test_solve_reaches_the_true_residual(cases, mesh, pc_type):
    p, be, ref = cases(mesh)
    phi, (n, m, h) = _random_state(p, 21)
    be.f_i = be.f_e = None
    _setup_pc(p, be, pc_type)
    b = _rhs(p, be)
    be.x.zero_()
    rtol = 1e-10
    its, rn, reason = be.cg(rtol, max_it=20000, norm_type="unpreconditioned")
    x = be.x.cpu().numpy()
    b_ref = ref.rhs(phi, n, m, h, T_STIM)
    res = np.linalg.norm(b_ref - ref.A @ x)
    print(f"{mesh} {pc_type}: {its} iterations, reason {reason}, reported {rn:.3e}, true {res:.3e}, rtol |b| = {rtol * np.linalg.norm(b_ref):.3e}")
    from cgx_hip import _lib
    assert _lib.REASONS[reason] == "CONVERGED_RTOL" and its > 0
    assert res <= 2.0 * rtol * np.linalg.norm(b_ref)
    # the gauge of the (zero) initial guess: every search direction has mean zero up to a few roundings, at most 2e4 of them add up
    assert abs(x.mean()) <= 2e4 * 4 * np.finfo(float).eps * np.abs(x).max()


@pytest.mark.parametrize("norm_type", ["preconditioned", "natural"])
def test_other_norms_and_dirichlet_solve(norm_type):
    p, be, ref = _problem("square16", "hh", dirichlet_bcs=True)
    phi, (n, m, h) = _random_state(p, 22)
    g = np.zeros(ref.n)
    g[ref.bc_nodes] = 0.005
    be.set_dirichlet_values(g[be.bc_nodes.cpu().numpy()])
    _setup_pc(p, be, "hypre")
    _rhs(p, be)
    its, rn, reason = be.cg(1e-12, max_it=2000, norm_type=norm_type)
    x = be.x.cpu().numpy()
    x_ref = ref.solve(ref.rhs(phi, n, m, h, T_STIM, g=g))
    print(f"dirichlet {norm_type}: {its} iterations, reason {reason}, max|dx| = {np.abs(x - x_ref).max():.3e} of {np.abs(x_ref).max():.3e}")
    assert reason == 2 and np.array_equal(x[ref.bc_nodes], g[ref.bc_nodes])
    assert np.allclose(x, x_ref, rtol=1e-6, atol=1e-9)


def test_repeatability(cases):
    p, be, ref = cases("tissue2d_18_3")
    _random_state(p, 23)
    _setup_pc(p, be, "hypre")
    _rhs(p, be)
    out = []
    for _ in range(2):
        be.x.zero_()
        its, rn, reason = be.cg(1e-9, max_it=500, norm_type="unpreconditioned")
        out.append((its, rn, be.x.clone()))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and torch.equal(out[0][2], out[1][2])


# ------------------------------------------------------------------------------------------ whole runs
def _run(mesh, steps, models="hh", **attrs):
    from cgx_hip.emi_models import g_syn
    from cgx_hip.emi_problem import ProblemEMI
    from cgx_hip.emi_solver import SolverEMI
    cfg = attrs.pop("config", None) or _config(mesh, time_steps=steps)
    p = ProblemEMI(cfg)
    p.add_ionic_model("HH" if models == "hh" else "Passive", stim_fun=g_syn)
    p.init_ionic_model()
    kw = {k: attrs.pop(k) for k in ("use_direct_solver", "save_xdmfs", "save_pngs") if k in attrs}

    class S(SolverEMI):
        pass
    for k, v in attrs.items():
        setattr(S, k, v)
    s = S(p, **kw)
    s.solve()
    return s


@pytest.mark.parametrize("mesh", ["square16", "cube4"])
def test_hh_trajectory_against_lu_stepping(mesh):
    s = _run(mesh, 5, use_direct_solver=True)            # PCG at rtol 1e-12
    p = s.problem
    lm = p.local_mesh
    ref = emi_ref.EmiRef(lm.coords, lm.cells, p.cell_side, lm.gamma, DT, p.C_M, p.sigma_i, p.sigma_e)
    phi, n, m, h = emi_ref.hh_trajectory(ref, 5)
    print(f"{mesh}: iterations {s.iterations}; phi_M range [{phi.min():.6f}, {phi.max():.6f}], max|dphi_M| = {np.abs(p.phi_M.numpy() - phi).max():.3e}")
    assert np.allclose(p.phi_M.numpy(), phi, rtol=1e-6, atol=1e-9)
    for f, g in ((p.n, n), (p.m, m), (p.h, h)):
        assert np.allclose(f.numpy(), g, rtol=1e-6, atol=1e-9)
    assert len(s.iterations) == 5 and s.tot_its == sum(s.iterations) and len(s.solve_time) == 5 and len(s.assembly_time) == 5
    # outputs of the problem: the solution functions and their copies of the previous step
    assert torch.equal(p.u_p[0].x.array, p.wh[0].x.array) and torch.equal(p.wh[0].x.array - p.wh[1].x.array, p.phi_M.x.array)


def test_mms_through_the_product():
    errs = {}
    for N in (16, 32):
        cfg = {"problem_type": "EMI", "dt": 0.01, "time_steps": 2, "C_M": 1.0, "sigma_i": 1.0, "sigma_e": 1.0, "quiet": True,
               "cell_tag_file": "mms.xdmf", "facet_tag_file": "mms.xdmf", "ics_tags": [1], "ecs_tags": [2],
               "MMS_test": {"N_mesh": N, "dim": 2}}
        s = _run(None, 2, models="passive", config=cfg, use_direct_solver=True)
        errs[N] = s.problem.errors
        want, _ = emi_ref.mms_run(N, dt=0.01, steps=2)
        print(f"N = {N}: native errors {errs[N][0]:.6e} {errs[N][1]:.6e}, reference {want[0]:.6e} {want[1]:.6e}, iterations {s.iterations}")
        assert errs[N][0] == pytest.approx(want[0], rel=1e-6) and errs[N][1] == pytest.approx(want[1], rel=1e-6)
    assert errs[16][0] / errs[32][0] >= 3.0 and errs[16][1] / errs[32][1] >= 3.0


def test_preconditioner_does_its_job():
    """square64, dt 5e-5, C_M 0.02, micrometre mesh, rtol 1e-8: the hierarchy on the EMI matrix against Jacobi"""
    from cgx_hip.emi_solver import SolverEMI
    its = {}
    for pc in ("hypre", "jacobi"):
        p, be, ref = _problem("square64", "hh", sigma_i=1.0, sigma_e=1.0)
        _random_state(p, 0)
        _setup_pc(p, be, pc, coarse_size=SolverEMI.amg_coarse_size)
        _rhs(p, be, DT)
        be.x.zero_()
        its[pc], rn, reason = be.cg(1e-8, max_it=5000, norm_type="unpreconditioned")
        assert reason == 2
    print(f"square64 PCG iterations at rtol 1e-8: hypre {its['hypre']}, jacobi {its['jacobi']}")
    assert 4 * its["hypre"] <= its["jacobi"]


def test_solution_xdmf_reads_back(tmp_path):
    from cgx_hip import xdmf
    cfg = _config("square8", time_steps=2, output_dir=str(tmp_path) + os.sep)
    rec = []
    from cgx_hip.emi_solver import SolverEMI
    orig = SolverEMI.save_xdmf

    def save(self):
        rec.append((self.problem.u_p[0].numpy().copy(), self.problem.u_p[1].numpy().copy()))
        orig(self)
    SolverEMI.save_xdmf = save
    try:
        s = _run("square8", 2, config=cfg, use_direct_solver=True, save_xdmfs=True, save_pngs=True)
    finally:
        SolverEMI.save_xdmf = orig
    assert len(rec) == 2 and os.path.exists(tmp_path / "subdomains.xdmf") and os.path.exists(tmp_path / "v.npy")
    f = xdmf.XdmfFile(tmp_path / "solution.xdmf")
    lm = s.problem.local_mesh
    cells, pts, _ = f.grid("mesh")
    assert np.array_equal(cells, lm.cells) and np.array_equal(pts, lm.coords)
    for k in (1, 2):
        g = f.grids[f"step_{k}"]
        vals = {a.get("Name"): np.asarray(f._data(f._child(a, "DataItem"))).reshape(-1) for a in g if a.tag.endswith("Attribute")}
        assert sorted(vals) == ["phi_e", "phi_i"]
        assert np.array_equal(vals["phi_i"], rec[k - 1][0]) and np.array_equal(vals["phi_e"], rec[k - 1][1])
        assert np.abs(vals["phi_i"]).max() > 0


def test_main_runs_the_reference_config(tmp_path, monkeypatch):
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emi_config.yaml")
    text = open(golden).read() + "\nquiet: true\n"
    (tmp_path / "config.yaml").write_text(text)
    monkeypatch.chdir(tmp_path)
    from CGx.EMI.main import main
    s = main(["--config", str(tmp_path / "config.yaml")])
    ni, ne = s.potential_norms()
    assert len(s.iterations) == 10 and all(r > 0 for r in s.reasons) and np.isfinite(ni) and ni > 0 and ne > 0
    assert os.path.exists(tmp_path / "output" / "solution.xdmf")


# ------------------------------------------------------------------------------------------ ABI errors
def test_abi_errors():
    from cgx_hip import _lib, amg
    from cgx_hip.emi_models import g_syn
    from cgx_hip.emi_problem import EmiBackend, ProblemEMI
    lib = _lib.load()
    E_ARG, E_STATE = -1, -3
    p = ProblemEMI(_config("square8"))
    p.add_ionic_model("HH", stim_fun=g_syn)
    p.init_ionic_model()
    be = EmiBackend(p, np.zeros(p.local_mesh.gamma.shape[0], dtype=np.int32))
    n = be.n_nodes
    v = torch.zeros(n, dtype=torch.float64, device=be.device)
    nv = torch.zeros(p.mesh.num_vertices, dtype=torch.float64, device=be.device)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    its, rn, reason = C.c_int32(), C.c_double(), C.c_int32()
    f = _lib.Fields()
    f.phi_m = nv.data_ptr()
    rp, ci, va = np.zeros(n + 1, dtype=np.int32), np.zeros(16, dtype=np.int32), np.zeros(16)
    i32, f64 = (lambda a: a.ctypes.data_as(_lib.i32p)), (lambda a: a.ctypes.data_as(_lib.f64p))
    before = [lib.knp_emi_get_csr(be.ctx, i32(rp), i32(ci), f64(va)), lib.knp_emi_set_dirichlet(be.ctx, 0, None),
              lib.knp_emi_spmv(be.ctx, ptr(v), ptr(v)), lib.knp_emi_assemble_rhs(be.ctx, C.byref(f), None, None, None, 1.0, ptr(v)),
              lib.knp_emi_pc_setup(be.ctx, 0), lib.knp_emi_pc_apply(be.ctx, ptr(v), ptr(v)),
              lib.knp_emi_cg_solve(be.ctx, ptr(v), ptr(v), 1e-8, 0.0, 10, 1, C.byref(its), C.byref(rn), C.byref(reason)),
              lib.knp_emi_update(be.ctx, ptr(v), ptr(nv), ptr(nv), ptr(nv))]
    assert before == [E_STATE] * 8, before
    sz = (C.c_int64 * _lib.KNP_SZ_COUNT)()
    lib.knp_get_sizes(be.ctx, sz)
    assert sz[_lib.SZ_EMI_NNZ] == 0
    # level 0 with n_nodes rows without knp_emi_setup: refused as before
    A = emi_ref.EmiRef(p.local_mesh.coords, p.local_mesh.cells, p.cell_side, p.local_mesh.gamma, DT, CM, SI, SE).A
    dinv = 1.0 / A.diagonal()

    def set_level0(M):
        be.check(lib.knp_amg_reset(be.ctx, 0, 1, 1, 1, 1))
        return lib.knp_amg_set_level(be.ctx, 0, 0, M.shape[0], M.shape[0], i32(M.indptr.astype(np.int32)), i32(M.indices.astype(np.int32)),
                                     f64(M.data), f64(np.ones(M.shape[0])), 1.0, 0, None, None, None, None, None, None)
    import scipy.sparse as sp
    I4 = sp.identity(4 * n, format="csr")
    assert set_level0(A) == E_ARG and set_level0(I4) == 0
    for bad in ((0.0, CM, SI, SE), (DT, -1.0, SI, SE), (DT, CM, 0.0, SE), (DT, CM, SI, float("nan"))):
        assert lib.knp_emi_setup(be.ctx, *bad) == E_ARG
    assert lib.knp_emi_setup(None, DT, CM, SI, SE) == E_ARG
    be.setup(DT, CM, SI, SE)
    lib.knp_get_sizes(be.ctx, sz)
    assert sz[_lib.SZ_EMI_NNZ] == be.n_pairs + 2 * be.n_gamma_pairs >= A.nnz       # (the reference drops entries that are exactly zero)
    assert set_level0(I4) == E_ARG and set_level0(A) == 0          # an EMI context: n_nodes rows, n_dof rows refused
    null = [lib.knp_emi_get_csr(be.ctx, None, i32(ci), f64(va)), lib.knp_emi_set_dirichlet(be.ctx, 2, None),
            lib.knp_emi_spmv(be.ctx, None, ptr(v)), lib.knp_emi_spmv(be.ctx, ptr(v), None),
            lib.knp_emi_assemble_rhs(be.ctx, None, None, None, None, 1.0, ptr(v)), lib.knp_emi_assemble_rhs(be.ctx, C.byref(f), None, None, None, 1.0, None),
            lib.knp_emi_pc_apply(be.ctx, None, ptr(v)), lib.knp_emi_pc_setup(be.ctx, 3),
            lib.knp_emi_cg_solve(be.ctx, None, ptr(v), 1e-8, 0.0, 10, 1, C.byref(its), C.byref(rn), C.byref(reason)),
            lib.knp_emi_cg_solve(be.ctx, ptr(v), ptr(v), 1e-8, 0.0, 10, 1, None, C.byref(rn), C.byref(reason)),
            lib.knp_emi_cg_solve(be.ctx, ptr(v), ptr(v), 1e-8, 0.0, 10, 5, C.byref(its), C.byref(rn), C.byref(reason)),
            lib.knp_emi_update(be.ctx, ptr(v), None, ptr(nv), ptr(nv))]
    assert null == [E_ARG] * len(null), null
    bad_node = np.array([n], dtype=np.int32)
    assert lib.knp_emi_set_dirichlet(be.ctx, 1, i32(bad_node)) == E_ARG
    assert lib.knp_emi_pc_setup(be.ctx, _lib.PC_AMG) == 0          # the one-level hierarchy uploaded above
    # a program that reads a gating variable the fields do not carry
    p.phi_M.x.array[:] = -0.065
    be.upload_programs(p.compile_programs())
    assert lib.knp_emi_assemble_rhs(be.ctx, C.byref(f), None, None, None, 1.0, ptr(v)) == E_ARG
    assert b"aux" in lib.knp_last_error(be.ctx)
    # zero right-hand side: converged at once
    v.zero_()
    x = torch.zeros_like(v)
    assert lib.knp_emi_cg_solve(be.ctx, ptr(v), ptr(x), 1e-8, 1e-50, 10, 1, C.byref(its), C.byref(rn), C.byref(reason)) == 0
    assert its.value == 0 and reason.value == 3 and float(x.abs().max()) == 0.0
