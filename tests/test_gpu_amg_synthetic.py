"""The AMG cycle kernels on synthetic hierarchies (tests/synthetic_hierarchies.py; preconditions in
tests/test_synthetic_hierarchies_host.py) at every lane width the launch switches can choose: 2 to 64 lanes per row of the generic
CSR kernels (k_spmv, k_cheby, k_restrict_first, k_prolong_rows, k_level_up), 2 to 32 lanes per node row of the node-blocked ones
(k_brestrict, k_bresidual, k_blevel_up, k_blevel_up_dots, in their three NF/XS forms), every branch and loop edge of k_dense_matvec,
and the cycle parameters no other GPU test sets (several pre- and post-sweeps, none, Chebyshev degrees 2 and 3, a last level that
only smooths).  The hierarchies built from the small test meshes reach widths 2 to 16 only; production meshes run at 32 and 64.

A. the level-by-level cycle on an uploaded level 0; B. the fused cycle with synthetic coarse levels under the library's own level 0
(all fields, and ion + potential hierarchy of the block-triangular form), node-blocked and scalar, KNP_COARSE_FUSED on and off;
C. two-level cycles whose dense coarse matrix has every size at which k_dense_matvec changes its path.  Every case asserts through
knp_amg_get_level_info that the width, storage and cycle form it was written for did run, and the last test counts, from those
read-outs, that the cases together reached every (kernel, width, storage) the switches can reach.

References: knpemi_oracle.pc_amg_vcycle / pc_amg_vcycle_fused / pc_btcc on the same hierarchy (rounded by amg.fp32_stored when the
library stores fp32).  Tolerances are the project's own, per field block max|z - z_ref| <= tol max|z_ref| with tol = 1e-10 (fp64
storage) and 2e-6 (fp32 storage), and 1e-12 for the dense product on its own.  Largest ratios measured on an MI355X:
A 6.9e-15 (fp64 storage) / 8.3e-08 (fp32 storage: the levels in fused form apply c A D^-1 rounded to fp32 once more);
B 1.7e-15 / 1.5e-15; C 4.0e-15 / 9.7e-16, the dense product alone 4.0e-15; the folded reduction leg 3.9e-15 after six GMRES
iterations.  No kernel or launch bug was found: every case holds with five or more orders of magnitude to spare in fp64."""
import numpy as np
import pytest
import torch

import synthetic_hierarchies as SH
from parity_utils import ci_config, make_oracle, make_problem

pytestmark = pytest.mark.gpu

CASES_A, CASES_B = SH.cases_a(), SH.cases_b()
COVERAGE = set()          # (kernel family, lanes, fp32 storage) the cases launched, from the read-outs
RAN = set()
WORST = {}                # (part, storage) -> largest ratio seen
SWITCHES = ("KNP_FUSED", "KNP_BLOCKED", "KNP_COARSE_FUSED", "KNP_FUSED_LEVELS", "KNP_FUSED_DOTS")
KIND = {"hypre": 2, "btcc": 3}     # KNP_PC_AMG, KNP_PC_AMG_BT


@pytest.fixture(scope="module")
def square8():
    """the 8 x 8 square of ci_config: it only supplies the level-0 size and, for Part B, the library's own level-0 operator"""
    import knpemi_oracle  # noqa: F401
    p = make_problem(ci_config(N=8, steps=1))
    be = p.create_backend()
    assert be.n_dof_owned == SH.N0_SQUARE8
    be.set_nullspace(False)
    be.assemble_precond()
    P = be.precond_csr().tocsr()
    P = P if P.shape[1] == be.n_dof_owned else P[:, :be.n_dof_owned].tocsr()
    be.assemble_rhs()
    be.assemble_matrix()      # A and the Schur diagonal of the block-triangular form, written while no preconditioner kind is set
    return be, make_oracle(8, "square"), P


def _env(monkeypatch, **switches):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)      # read at every knp_pc_setup


def _upload(be, hiers, fp32, pre, post, deg, modes):
    be.check(be.lib.knp_amg_set_precision(be.ctx, 1 if fp32 else 0))
    for index, (h, mode) in enumerate(zip(hiers, modes)):
        SH.amg.upload(be.lib, be.ctx, be.check, h, pre, post, deg, index=index, level0_native=mode != 0)
        be.check(be.lib.knp_amg_use_native_level0(be.ctx, index, mode))


def _info(be, index, h):
    return [be.amg_level_info(index, l) for l in range(len(h.levels))]


def _apply(be, r):
    rt = torch.as_tensor(r, device=be.device)
    z = torch.full_like(rt, float("nan"))       # every entry must be written
    be.pc_apply(rt, z)
    return z.cpu().numpy()


def _compare(be, ref, tolerance, part, fp32, label):
    worst = 0.0
    for r in SH.residuals(be.n_dof_owned):
        z, zo = _apply(be, r), ref(r.copy())
        assert np.all(np.isfinite(z)), label
        worst = max(worst, SH.block_ratio(z, zo))
    print(f"{label}: max|z - z_ref| / max|z_ref| per field block = {worst:.3e} (tolerance {tolerance:.0e})")
    WORST[(part, fp32)] = max(WORST.get((part, fp32), 0.0), worst)
    assert worst <= tolerance, (label, worst)


def _record(request, launches, fp32, cinv_f32=False):
    """what the case launched, from its read-outs: noted BEFORE the numerical comparison, which it does not depend on, so that a case
    that fails still counts for the coverage table and the last test reports instead of staying silent.  The dense product has a
    storage of its own (``cinv_f32`` of the read-out)."""
    COVERAGE.update((k, w, bool(cinv_f32) if k == "k_dense_matvec" else fp32) for k, w in launches)
    RAN.add(request.node.nodeid)


def _generic_lanes(M, rows=None):
    return SH.pick_lanes(M.nnz / (rows or M.shape[0]))


# ---- A. level-by-level cycle on an uploaded level 0 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES_A, ids=[c["id"] for c in CASES_A])
def test_level_by_level_cycle(square8, case, monkeypatch, request):
    import knpemi_oracle as K
    be, _, _ = square8
    _env(monkeypatch)
    h, fp32, (pre, post, deg) = SH.build_a(case), case["fp32"], case["triple"]
    _upload(be, [h], fp32, pre, post, deg, [0])
    be.pc_setup(KIND["hypre"])
    info = _info(be, 0, h)
    _record(request, SH.launches_level_by_level(info, pre, post, deg), fp32, info[0]["cinv_f32"])
    _, s_levels = SH.operators_a(case)
    for l, (lv, I) in enumerate(zip(h.levels, info)):
        assert (I["fused"], I["blocked"], I["cfused"], I["l0_fused"], I["cinv_f32"]) == (0, 0, 0, 0, 0), I
        assert I["n"] == lv.A.shape[0] and I["fp32"] == int(fp32) and I["nc"] == (h.levels[-1].A.shape[0] if case["dense"] else 0)
        assert I["lfused"] == int(l in s_levels), (l, I)
        assert I["A_lanes"] == _generic_lanes(lv.A)
        if lv.P is None:
            assert (I["P_lanes"], I["R_lanes"], I["n_coarse"]) == (0, 0, 0)
            continue
        n_act = int((np.diff(lv.P.indptr) > 0).sum())
        assert (I["P_n_act"] > 0) == case["sparse_P"] and I["P_n_act"] in (0, n_act)
        assert I["P_lanes"] == _generic_lanes(lv.P, I["P_n_act"] or None) and I["R_lanes"] == _generic_lanes(lv.R)
        assert I["S_lanes"] == (_generic_lanes(lv.S) if lv.S is not None else 0)
        if l == 0:
            want = (case["width"],) * 2 + ((case["width"],) if not case.get("r_transpose") else (I["R_lanes"],))
            assert (I["A_lanes"], I["P_lanes"], I["R_lanes"]) == want, I       # the width the case was written for
    hs = SH.fp32_stored(h) if fp32 else h
    ref = K.pc_amg_vcycle(hs.levels, hs.coarse_inv, pre, post, deg)
    _compare(be, ref, SH.tol(fp32), "A", fp32, case["id"])


# ---- B. fused cycle on the library's own level 0 ----------------------------------------------------------------------------------------
def _settings(case):
    base = [{}] if case["levels"] == 2 else [{}, {"KNP_COARSE_FUSED": "0"}]
    if case["kind"] == "generic":
        return [dict(s, KNP_BLOCKED="0") for s in base]
    return base + [dict(s, KNP_BLOCKED="0") for s in base]


@pytest.mark.parametrize("case", CASES_B, ids=[c["id"] for c in CASES_B])
def test_fused_cycle(square8, case, monkeypatch, request):
    be, o, P = square8
    _env(monkeypatch)
    hs, fp32, form, width, nl = SH.build_b(case, P), case["fp32"], case["form"], case["width"], case["levels"]
    nf = getattr(hs[0], "node_fields", 0)
    _upload(be, hs, fp32, 1, 1, 1, [1] if form == "hypre" else [2, 3])
    for switches in _settings(case):
        _env(monkeypatch, **switches)
        be.pc_setup(KIND[form])
        infos = [_info(be, i, h) for i, h in enumerate(hs)]
        _record(request, SH.launches_fused(infos[0], nf or (4 if form == "hypre" else 3), False), fp32, infos[0][0]["cinv_f32"])
        if form == "btcc":
            _record(request, SH.launches_fused(infos[1], 0, True), fp32, infos[1][0]["cinv_f32"])
        blocked = int(case["kind"] == "blocked" and "KNP_BLOCKED" not in switches)
        cfused = int(nl == 3 and "KNP_COARSE_FUSED" not in switches)
        for i, info in enumerate(infos):
            for I in info:
                assert (I["fused"], I["blocked"], I["cfused"], I["l0_fused"], I["lfused"]) == (1, blocked if i == 0 else 0, cfused, 0, 0), (switches, i, I)
                assert I["fp32"] == int(fp32) or I["n_coarse"] == 0
                assert I["cinv_f32"] == int(fp32 and form == "btcc" and i == 0) and I["nc"] == hs[i].levels[-1].A.shape[0]
        I0, I1 = infos[0][0], infos[0][1]
        if case["kind"] == "blocked":      # the node-blocked copies exist and sit at the wanted width (level 0's restrictor: 97 node columns)
            w_r0 = SH.feasible_width(width, 2 * (SH.N0_SQUARE8 // 4), SH.BLOCKED_AVG)
            assert (I0["bR_lanes"], I0["bS_lanes"]) == (w_r0, width), I0
            if nl == 3:
                assert (I1["bA_lanes"], I1["bR_lanes"], I1["bS_lanes"], I1["bRt_lanes"], I1["bU_lanes"]) == (width,) * 5, I1
        elif case["kind"] == "unsync":     # S of level 0 is refused, the cycle stays on the scalar kernels
            assert I0["bS_lanes"] == 0 and I0["bR_lanes"] > 0 and I0["blocked"] == 0
        else:
            assert I0["bS_lanes"] == 0 and I0["S_lanes"] == width
            if nl == 3:
                assert (I1["A_lanes"], I1["R_lanes"], I1["S_lanes"], I1["Rt_lanes"], I1["U_lanes"]) == (width,) * 5, I1
        for i, (h, info) in enumerate(zip(hs, infos)):      # the read-out restated from the matrices
            for lv, I in zip(h.levels[:-1], info):
                rows_S = I["S_n_act"] or lv.S.shape[0]
                assert (I["R_lanes"], I["S_lanes"]) == (_generic_lanes(lv.R), _generic_lanes(lv.S, rows_S)), (i, I)
        if form == "btcc":      # the potential hierarchy is a scalar one of the case's width whatever the ion hierarchy is: compact rows of S
            assert infos[1][0]["S_n_act"] == SH.N0_SQUARE8 // 4 and infos[1][0]["S_lanes"] == width, infos[1][0]
        label = case["id"] + "".join(f" {k}={v}" for k, v in switches.items())
        _compare(be, SH.reference_b(form, hs, fp32, bool(cfused), o), SH.tol(fp32), "B", fp32, label)


@pytest.mark.parametrize("width", SH.BLOCKED_WIDTHS)
def test_folded_reduction_leg(square8, width, monkeypatch, request):
    """k_blevel_up_dots (the last leg of the node-blocked cycle on four fields with the first stage of the GMRES reductions in its
    epilogue): a few GMRES iterations with and without KNP_FUSED_DOTS, as test_gpu_fused_reductions.py compares them -- the same
    iteration count and the same iterate to 1e-10 per field block (the partial sums are partitioned differently)."""
    be, _, P = square8
    h = SH.part_b_blocked(P, 4, width, 3)
    _env(monkeypatch)
    _upload(be, [h], True, 1, 1, 1, [1])

    def solve(**switches):
        _env(monkeypatch, **switches)
        be.pc_setup(KIND["hypre"])
        be.profile_reset()
        be.x.zero_()
        its, _, _ = be.gmres(1e-30, max_it=6)
        return its, be.x.cpu().numpy().copy(), be.stats(), _info(be, 0, h)
    its1, x1, st1, info = solve()
    _record(request, SH.launches_fused(info, 4, False, dots=st1["fused_dots"] > 0), True)      # (the fold counter says the folded leg ran)
    its0, x0, st0, _ = solve(KNP_FUSED_DOTS="0")
    assert (info[0]["blocked"], info[0]["cfused"], info[0]["bS_lanes"]) == (1, 1, width), info[0]
    assert st1["fused_dots"] >= its1 and st0["fused_dots"] == 0 and its1 == its0 == 6, (its1, its0, st1, st0)
    ratio = SH.block_ratio(x1, x0)
    print(f"folded leg at {width} lanes: iterate after {its1} iterations differs by {ratio:.3e} per field block")
    WORST[("dots", True)] = max(WORST.get(("dots", True), 0.0), ratio)
    assert np.all(np.isfinite(x0)) and ratio <= 1e-10


# ---- C. the dense coarse product -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SH.DENSE_N_FP64)
def test_dense_coarse_product_fp64(square8, n, monkeypatch, request):
    """no smoothing, injection as prolongator: z = P Cinv R r shows the dense product itself, compared with the product evaluated in
    extended precision on the reference's R r"""
    import knpemi_oracle as K
    be, _, _ = square8
    _env(monkeypatch)
    r = SH.residuals(be.n_dof_owned)[0]
    for shift in range(0, n, SH.N0_SQUARE8):
        h = SH.part_c_fp64(n, shift)
        _upload(be, [h], False, 0, 0, 1, [0])
        be.pc_setup(KIND["hypre"])
        I = _info(be, 0, h)[0]
        _record(request, {("k_dense_matvec", I["nc"])}, bool(I["fp32"]), I["cinv_f32"])
        assert (I["nc"], I["cinv_f32"], I["fused"], I["fp32"]) == (n, 0, 0, 0), I
        _compare(be, K.pc_amg_vcycle(h.levels, h.coarse_inv, 0, 0, 1), SH.TOL_FP64, "C", False, f"dense n={n} shift={shift}")
        x = h.coarse_inv.astype(np.longdouble) @ (h.levels[0].R @ r).astype(np.longdouble)
        z = _apply(be, r)
        ratio = float(np.max(np.abs(z - x[h.levels[0].P.indices].astype(np.float64))) / np.max(np.abs(x)))
        print(f"dense product alone, n={n} shift={shift}: {ratio:.3e}")
        WORST[("C-product", False)] = max(WORST.get(("C-product", False), 0.0), ratio)
        assert ratio <= SH.TOL_DENSE


@pytest.mark.parametrize("n", SH.DENSE_N_FP32)
def test_dense_coarse_product_fp32(square8, n, monkeypatch, request):
    """the fp32 copy of the dense matrix exists only for the ion hierarchy of the fused block-triangular form"""
    be, o, P = square8
    _env(monkeypatch)
    hs = SH.build_c_fp32(n, P)
    _upload(be, hs, True, 1, 1, 1, [2, 3])
    be.pc_setup(KIND["btcc"])
    I = _info(be, 0, hs[0])[0]
    _record(request, {("k_dense_matvec", I["nc"])}, bool(I["fp32"]), I["cinv_f32"])
    assert (I["nc"], I["cinv_f32"], I["fused"], I["fp32"]) == (n, 1, 1, 1), I
    _compare(be, SH.reference_b("btcc", hs, True, False, o), SH.TOL_FP32, "C", True, f"dense fp32 n={n}")


def test_the_cases_together_reach_every_kernel_width_and_storage(request):
    """Counted from what the cases recorded right after their read-outs.  A collected case that did not record (it failed before its
    read-out, was skipped, or ran in another process) makes this test FAIL; it skips only when cases of this module were deselected on
    the command line, which the collection shows, or when the module is spread over worker processes."""
    expected = len(CASES_A) + len(CASES_B) + len(SH.BLOCKED_WIDTHS) + len(SH.DENSE_N_FP64) + len(SH.DENSE_N_FP32)
    mine = [it.nodeid for it in request.session.items if it.nodeid.split("::")[0] == request.node.nodeid.split("::")[0] and it.nodeid != request.node.nodeid]
    silent = sorted(set(mine) - RAN)
    if hasattr(request.config, "workerinput"):
        pytest.skip("the table is kept per process: run this module in one process")
    assert not silent, f"{len(silent)} collected case(s) left no read-out, the coverage table cannot be trusted: {silent[:8]}"
    if len(mine) < expected:
        pytest.skip(f"{expected - len(mine)} case(s) of this module were deselected: the table is asserted on the whole module only")
    for key in sorted(WORST):
        print("largest ratio", key, f"{WORST[key]:.3e}")
    table = {}
    for k, w, fp32 in sorted(COVERAGE, key=str):
        if k != "k_dense_matvec":
            table.setdefault((k, fp32), []).append(w)
    for (k, fp32), ws in sorted(table.items()):
        print(f"{k:20s} {'fp32' if fp32 else 'fp64'}: lanes {sorted(set(ws))}")
    print("k_dense_matvec n:", sorted({(w, fp32) for k, w, fp32 in COVERAGE if k == "k_dense_matvec"}))
    missing = SH.coverage_wanted() - COVERAGE
    assert not missing, sorted(missing, key=str)
