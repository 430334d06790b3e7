"""Host-side checks of tests/synthetic_hierarchies.py and of the references tests/test_gpu_amg_synthetic.py compares with -- the
generator and the NumPy cycles, not the library: the operators have the prescribed row-length profiles and land in the band of the
wanted lane width, the level operators are symmetric and strictly diagonally dominant, the node-synchronised operators pass (or, in
the variant made for it, fail) the structure test of the library's node-blocked copies; the fused restatement of the cycle equals the
level-by-level one; the fp64 references agree with the same cycles evaluated in extended precision to 1e-13; and deleting the last
entry of the longest row of any operator a case's cycle reads moves the reference by at least 100 x the tolerance the GPU test uses
for that case (the constants are imported from the generator, as the GPU tests do)."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

import synthetic_hierarchies as SH
from parity_utils import fp32_stored, make_oracle

import knpemi_oracle as K

CASES_A = SH.cases_a()
CASES_B = SH.cases_b()
_cache = {}


def _a(case):
    if case["id"] not in _cache:
        _cache[case["id"]] = SH.build_a(case)
    return _cache[case["id"]]


@pytest.fixture(scope="module")
def square8():
    o = make_oracle(8, "square")
    P = o.assemble_P().tocsr()
    assert P.shape[0] == SH.N0_SQUARE8
    return o, P


def _b(case, P):
    if case["id"] not in _cache:
        _cache[case["id"]] = SH.build_b(case, P)
    return _cache[case["id"]]


def _lengths(M):
    return np.diff(sp.csr_matrix(M).indptr)


def _has_edges(M, L, empty=True):
    have = set(_lengths(M).tolist())
    want = SH.edge_lengths(L, M.shape[1], empty)
    if not empty:
        want[-1] = min(want[-1], M.shape[1] - 2)
    short = [e for e in want[:-1] if e < want[-1]]          # (capped lengths fall together with the longest row)
    return all(e in have for e in short) and max(have) >= want[-1]


def _ends_in_last_column(M):
    M = sp.csr_matrix(M, copy=True)
    M.sort_indices()
    i = int(np.argmax(np.diff(M.indptr)))
    return M.indices[M.indptr[i + 1] - 1] == M.shape[1] - 1


def _blocked(M, nf, rs, cs, restrictor=False):
    """the structure test of build_blocked (knp_kernels.hip): lanes of the node-blocked copy, 0 when it is refused"""
    M = sp.csr_matrix(M).tocoo()
    if M.shape[0] % rs or np.any(M.row % rs >= nf) or np.any(M.col % cs != M.row % rs):
        return 0
    nodes = len(set(zip((M.row // rs).tolist(), (M.col // cs).tolist())))
    if nodes * nf > 1.25 * M.nnz + 64.0:
        return 0
    return SH.blocked_lanes(nodes / (M.shape[0] // rs), restrictor)


@pytest.mark.parametrize("width", SH.GENERIC_WIDTHS)
def test_part_a_profiles_and_dominance(width):
    h = SH.part_a_hierarchy(width)
    assert [lv.A.shape[0] for lv in h.levels] == list(SH.A_SIZES)
    for l, lv in enumerate(h.levels):
        A = lv.A
        wa = SH.feasible_width(width, A.shape[0])
        d = A.diagonal()
        off = np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(d)
        assert abs(A - A.T).max() == 0.0 and np.all(d > 0.0) and np.all(d > off) and np.array_equal(lv.dinv, 1.0 / d)
        assert SH.pick_lanes(A.nnz / A.shape[0]) == wa and _has_edges(A, wa, empty=False) and _ends_in_last_column(A)
        assert lv.lambda_max > 0.0
        if lv.P is None:
            continue
        wp, wr = SH.feasible_width(width, lv.P.shape[1]), SH.feasible_width(width, lv.R.shape[1])
        if l == 0:
            assert wa == wp == wr == width          # level 0 carries the wanted width in all three roles
        rs = np.asarray(lv.P.sum(axis=1)).ravel()
        assert lv.P.data.min() > 0.0 and np.allclose(rs[_lengths(lv.P) > 0], 1.0, rtol=0, atol=1e-14)
        for M, w in ((lv.P, wp), (lv.R, wr)):
            assert SH.pick_lanes(M.nnz / M.shape[0]) == w and _has_edges(M, w) and _ends_in_last_column(M), (l, w)
        assert abs(lv.S - SH.amg.post_smoothed_prolongator(A, lv.dinv, lv.lambda_max, lv.P)).max() == 0.0
    hs = SH.part_a_hierarchy(width, n_levels=2, sparse_P=True)
    Pm = hs.levels[0].P
    n_act = int((_lengths(Pm) > 0).sum())
    assert n_act <= 0.8 * Pm.shape[0] and SH.pick_lanes(Pm.nnz / n_act) == width


@pytest.mark.parametrize("nf", [3, 4])
@pytest.mark.parametrize("width", SH.BLOCKED_WIDTHS)
def test_node_synchronised_operators_take_the_wanted_blocked_width(square8, nf, width):
    _, P = square8
    h = SH.part_b_blocked(P, nf, width, 3)
    nodes = [P.shape[0] // 4] + list(SH.B_NODES[width])
    assert h.node_fields == nf and [lv.A.shape[0] for lv in h.levels] == [4 * nodes[0], nf * nodes[1], nf * nodes[2]]
    l0, l1 = h.levels[0], h.levels[1]
    w_r0 = SH.feasible_width(width, 2 * nodes[0], SH.BLOCKED_AVG)
    assert _blocked(l0.R, nf, nf, 4, True) == w_r0 and _blocked(l0.S, nf, 4, nf) == width
    assert _blocked(l1.A, nf, nf, nf) == width and _blocked(l1.R, nf, nf, nf, True) == width and _blocked(l1.S, nf, nf, nf) == width
    assert _blocked(l1.Rt, nf, nf, nf, True) == width and _blocked(l1.U, nf, nf, nf) == width
    for lv in h.levels[1:]:
        d = lv.A.diagonal()
        assert abs(lv.A - lv.A.T).max() == 0.0 and np.all(d > np.asarray(abs(lv.A).sum(axis=1)).ravel() - d)
    # node rows carry the edge lengths of the width, as far as the node columns reach
    for M, rs, cs in ((l0.S, 4, nf), (l1.A, nf, nf), (l1.S, nf, nf), (l1.U, nf, nf)):
        node = sp.csr_matrix(M)[0::rs][:, 0::cs]
        assert _has_edges(node, width, empty=M is not l1.A) and _ends_in_last_column(node)
    hu = SH.part_b_blocked(P, nf, 8, 3, unsync=True)
    assert _blocked(hu.levels[0].S, nf, 4, nf) == 0 and _blocked(hu.levels[0].R, nf, nf, 4, True) > 0


@pytest.mark.parametrize("width", SH.GENERIC_WIDTHS)
def test_free_operators_of_part_b_take_the_wanted_width(square8, width):
    _, P = square8
    for fields in ((0, 1, 2, 3), (0, 1, 2), (3,)):
        h = SH.part_b_generic(P, fields, width, 3)
        l0, l1 = h.levels[0], h.levels[1]
        n_act = len(fields) * P.shape[0] // 4
        in_class = np.isin(np.arange(P.shape[0]) % 4, fields)
        # S has rows and R has columns on the unknowns of the class only (one row of S is the empty edge row); the inverse diagonal,
        # which makes the library keep a row in its compact list, is zero on the other fields and positive on the class
        assert int((_lengths(l0.S) > 0).sum()) == n_act - 1 and not np.any(_lengths(l0.S)[~in_class]) and in_class[l0.R.indices].all()
        assert np.all(l0.dinv[in_class] > 0.0) and not np.any(l0.dinv[~in_class])
        # rows the library counts for the width of S: the compact list (rows with a non-zero inverse diagonal) when it is at most 80 %
        rows_counted = n_act if n_act <= 0.8 * P.shape[0] else P.shape[0]
        assert SH.pick_lanes(l0.S.nnz / rows_counted) == width
        assert SH.pick_lanes(l0.R.nnz / l0.R.shape[0]) == SH.feasible_width(width, n_act)      # (its columns: the unknowns of the class)
        for M in (l1.A, l1.R, l1.S, l1.Rt, l1.U):
            assert SH.pick_lanes(M.nnz / M.shape[0]) == width and _ends_in_last_column(M)


@pytest.mark.parametrize("width", SH.GENERIC_WIDTHS)
def test_fused_restatement_equals_the_level_by_level_cycle(width):
    """on the Part A hierarchies, whose S, Rt and U are built from A, P and R: 1e-12"""
    h = SH.part_a_hierarchy(width)
    for r in SH.residuals(SH.N0_SQUARE8):
        z = K.pc_amg_vcycle(h.levels, h.coarse_inv, 1, 1, 1)(r.copy())
        zf = K.pc_amg_vcycle_fused(h.levels, h.coarse_inv)(r.copy())
        zs = K.pc_amg_vcycle_fused(SH.strip_coarse_fused(h).levels, h.coarse_inv)(r.copy())
        zr = SH.restated_cycle(h.levels, h.coarse_inv, 1, 1, 1, s_levels=(1,))(r)
        for other in (zf, zs, zr):
            assert np.max(np.abs(other - z)) <= 1e-12 * np.max(np.abs(z))


def _longdouble(h):
    """the hierarchy with dense extended-precision operators: the oracle's cycles then run in that precision unchanged"""
    ld = lambda M: None if M is None else np.asarray(M.toarray() if sp.issparse(M) else M, dtype=np.longdouble)
    h2 = copy.copy(h)
    h2.levels = []
    for lv in h.levels:
        l2 = copy.copy(lv)
        for name in ("A", "P", "R", "S", "Rt", "U"):
            setattr(l2, name, ld(getattr(lv, name, None)))
        l2.dinv = np.asarray(lv.dinv, dtype=np.longdouble)
        Pt = getattr(lv, "Pt", None)
        l2.Pt = ld(Pt) if Pt is not None else l2.A * l2.dinv[None, :]
        h2.levels.append(l2)
    h2.coarse_inv = ld(h.coarse_inv)
    return h2


@pytest.mark.parametrize("case", CASES_A, ids=[c["id"] for c in CASES_A])
def test_part_a_reference_against_extended_precision(case):
    h = _a(case)
    h = fp32_stored(h) if case["fp32"] else h
    hl = _longdouble(h)
    pre, post, deg = case["triple"]
    for r in SH.residuals(SH.N0_SQUARE8):
        z = K.pc_amg_vcycle(h.levels, h.coarse_inv, pre, post, deg)(r.copy())
        zl = K.pc_amg_vcycle(hl.levels, hl.coarse_inv, pre, post, deg)(r.astype(np.longdouble))
        zr = SH.restated_cycle(h.levels, h.coarse_inv, pre, post, deg, np.longdouble)(r)
        err = float(np.max(np.abs(z - zl)) / np.max(np.abs(zl)))
        assert err <= 1e-13, err
        assert float(np.max(np.abs(zr - zl)) / np.max(np.abs(zl))) <= 1e-14      # (the oracle rounds its Chebyshev coefficients to fp64)


@pytest.mark.parametrize("case", CASES_B, ids=[c["id"] for c in CASES_B])
def test_part_b_reference_against_extended_precision(square8, case):
    """per hierarchy (the block-triangular form only adds pointwise terms around the two cycles)"""
    _, P = square8
    for h in SH.stored(_b(case, P), case["form"], case["fp32"]):
        for hh in ([h, SH.strip_coarse_fused(h)] if case["levels"] == 3 else [h]):
            hl = _longdouble(hh)
            for r in SH.residuals(SH.N0_SQUARE8):
                z = K.pc_amg_vcycle_fused(hh.levels, hh.coarse_inv)(r.copy())
                zl = K.pc_amg_vcycle_fused(hl.levels, hl.coarse_inv)(r.astype(np.longdouble))
                assert SH.block_ratio(z, zl.astype(np.float64)) <= 1e-13


def _moved(ref, ref_changed, fp32):
    """largest movement over the residuals, per field block, in units of the GPU test's tolerance"""
    return max(SH.block_ratio(ref_changed(r.copy()), ref(r.copy())) for r in SH.residuals(SH.N0_SQUARE8)) / SH.tol(fp32)


@pytest.mark.parametrize("case", CASES_A, ids=[c["id"] for c in CASES_A])
def test_part_a_cases_notice_a_dropped_lane_tail(case):
    h = _a(case)
    rnd = fp32_stored if case["fp32"] else (lambda x: x)
    pre, post, deg = case["triple"]
    ops, s_levels = SH.operators_a(case)
    ref = lambda hh: SH.restated_cycle(rnd(hh).levels, hh.coarse_inv, pre, post, deg, s_levels=s_levels)
    for level, name in ops:
        moved = _moved(ref(h), ref(SH.with_operator_changed(h, level, name)), case["fp32"])
        assert moved >= SH.GUARD, (level, name, moved)


@pytest.mark.parametrize("case", CASES_B, ids=[c["id"] for c in CASES_B])
def test_part_b_cases_notice_a_dropped_lane_tail(square8, case):
    o, P = square8
    hs = _b(case, P)
    for cfused in ((True, False) if case["levels"] == 3 else (False,)):
        ref = SH.reference_b(case["form"], hs, case["fp32"], cfused, o)
        for hi, h in enumerate(hs):
            for level, name in SH.operators_b(h, cfused):
                hs2 = list(hs)
                hs2[hi] = SH.with_operator_changed(h, level, name)
                moved = _moved(ref, SH.reference_b(case["form"], hs2, case["fp32"], cfused, o), case["fp32"])
                assert moved >= SH.GUARD, (cfused, hi, level, name, moved)


@pytest.mark.parametrize("n", SH.DENSE_N_FP64)
def test_dense_cases_show_the_whole_product_and_notice_a_dropped_entry(n):
    seen = np.zeros(n, dtype=bool)
    for shift in range(0, n, SH.N0_SQUARE8):
        h = SH.part_c_fp64(n, shift)
        P = h.levels[0].P
        assert np.array_equal(_lengths(P), np.ones(SH.N0_SQUARE8)) and np.all(P.data == 1.0)
        seen[P.indices] = True
        r = SH.residuals(SH.N0_SQUARE8)[0]
        z = K.pc_amg_vcycle(h.levels, h.coarse_inv, 0, 0, 1)(r.copy())
        x = h.coarse_inv.astype(np.longdouble) @ (h.levels[0].R @ r).astype(np.longdouble)
        assert np.max(np.abs(z - x[P.indices].astype(np.float64))) <= 1e-14 * float(np.max(np.abs(x)))
    assert seen.all()
    C = h.coarse_inv
    assert np.array_equal(C, C.T) and np.linalg.cond(C) < 50.0
    if n > 1:     # the entry a dropped tail of the first row would lose
        b = h.levels[0].R @ r
        assert abs(C[0, n - 1] * b[n - 1]) >= SH.GUARD * SH.TOL_DENSE * np.max(np.abs(C @ b))


@pytest.mark.parametrize("n", SH.DENSE_N_FP32)
def test_fp32_dense_cases_notice_a_dropped_entry(square8, n):
    o, P = square8
    hs = SH.build_c_fp32(n, P)
    assert hs[0].coarse_inv.shape == (n, n)
    ref = SH.reference_b("btcc", hs, True, False, o)
    hs2 = [copy.copy(hs[0]), hs[1]]
    hs2[0].coarse_inv = hs[0].coarse_inv.copy()
    hs2[0].coarse_inv[:, n - 1] = 0.0        # what a dropped tail of the row loop loses: the last entry of every row
    assert _moved(ref, SH.reference_b("btcc", hs2, True, False, o), True) >= SH.GUARD
    for level, name in SH.operators_b(hs[0], False):
        hs3 = [SH.with_operator_changed(hs[0], level, name), hs[1]]
        assert _moved(ref, SH.reference_b("btcc", hs3, True, False, o), True) >= SH.GUARD, (level, name)


def _level(**kw):
    """a read-out as knp_amg_get_level_info gives it, zero where the test does not care"""
    from cgx_hip.backend import Backend
    return dict(dict.fromkeys(Backend.AMG_LEVEL_INFO, 0), **kw)


def test_launch_restatement_and_coverage_table_are_consistent():
    """launches_level_by_level / launches_fused restate the launch sequence of amg_vcycle / amg_cycle_fused; every branch of them on
    hand-made read-outs whose lanes are all different, so that a wrong operator or level shows"""
    want = SH.coverage_wanted()
    assert len(want) == 2 * (5 * 6 + 4) + 9 * 5 + len(SH.DENSE_N_FP64) + len(SH.DENSE_N_FP32)
    # level by level: compact prolongator on the switch's default, first Chebyshev step folded into the restriction, smoothing-only end
    info = [_level(A_lanes=8, P_lanes=32, R_lanes=4, S_lanes=16, P_n_act=5), _level(A_lanes=2)]
    assert SH.launches_level_by_level(info, 1, 1, 2) == {("k_cheby", 8), ("k_spmv", 8), ("k_restrict_first", 4), ("k_cheby", 2), ("k_prolong_rows", 16)}
    # ... no pre-sweep and none at all: the restriction is a plain product when the coarse level does not start with a smoothing step
    assert SH.launches_level_by_level(info, 0, 1, 1) == {("k_spmv", 8), ("k_restrict_first", 4), ("k_prolong_rows", 16), ("k_cheby", 8)}
    assert SH.launches_level_by_level(info, 0, 0, 1) == {("k_spmv", 8), ("k_spmv", 4), ("k_prolong_rows", 16)}
    # ... three levels with the dense end, level 1 in fused form: plain restriction in front of it, S on the way up, no P of level 1
    info = [_level(A_lanes=64, P_lanes=32, R_lanes=16, nc=7), _level(A_lanes=8, P_lanes=4, R_lanes=2, S_lanes=16, lfused=1, nc=7), _level(A_lanes=2, nc=7)]
    assert SH.launches_level_by_level(info, 1, 1, 1) == {("k_spmv", 64), ("k_spmv", 16), ("k_spmv", 8), ("k_spmv", 2), ("k_level_up", 16),
                                                        ("k_dense_matvec", 7), ("k_spmv", 32), ("k_cheby", 64)}
    info[1]["lfused"] = 0
    assert SH.launches_level_by_level(info, 1, 1, 1) == {("k_spmv", 64), ("k_restrict_first", 16), ("k_spmv", 8), ("k_spmv", 2), ("k_spmv", 4),
                                                        ("k_cheby", 8), ("k_dense_matvec", 7), ("k_spmv", 32), ("k_cheby", 64)}
    # fused cycle, three levels, scalar rows: R and A down, S up; compact potential vectors change the kernel of level 0 only
    F = lambda **kw: [_level(R_lanes=2, S_lanes=4, bR_lanes=8, bS_lanes=16, nc=9, fused=1, **kw),
                      _level(A_lanes=8, R_lanes=16, S_lanes=32, Rt_lanes=64, U_lanes=2, bA_lanes=4, bR_lanes=2, bS_lanes=32, bRt_lanes=16,
                             bU_lanes=8, nc=9, fused=1, **kw), _level(A_lanes=4, nc=9, fused=1, **kw)]
    dense = ("k_dense_matvec", 9)
    assert SH.launches_fused(F(), 4, False) == {dense, ("k_restrict_first", 2), ("k_spmv", 8), ("k_spmv", 16), ("k_level_up", 32), ("k_level_up", 4)}
    assert SH.launches_fused(F(), 0, True) == {dense, ("k_restrict_first", 2), ("k_spmv", 8), ("k_spmv", 16), ("k_level_up", 32), ("k_level_up<1>", 4)}
    # ... intermediate levels as two plain products
    assert SH.launches_fused(F(cfused=1), 4, False) == {dense, ("k_spmv", 2), ("k_spmv", 64), ("k_level_up", 4)}
    # ... node-blocked: XS / RS = 4 on level 0, NF below; the residual of the intermediate level on bA
    assert SH.launches_fused(F(blocked=1), 3, False) == {dense, ("k_brestrict<3,4>", 8), ("k_bresidual<3>", 4), ("k_brestrict<3,3>", 2),
                                                        ("k_blevel_up<3,3>", 32), ("k_blevel_up<3,4>", 16)}
    assert SH.launches_fused(F(blocked=1, cfused=1), 4, False) == {dense, ("k_brestrict<4,4>", 8), ("k_brestrict<4,4>", 16), ("k_blevel_up<4,4>", 16)}
    assert SH.launches_fused(F(blocked=1, cfused=1), 4, False, dots=True) == {dense, ("k_brestrict<4,4>", 8), ("k_brestrict<4,4>", 16), ("k_blevel_up_dots", 16)}
    # two levels: no intermediate level at all
    assert SH.launches_fused(F()[:1] + F()[2:], 4, False) == {dense, ("k_spmv", 2), ("k_level_up", 4)}
    assert set(SH.launches_fused(F(blocked=1)[:1] + F()[2:], 4, False)) == {dense, ("k_brestrict<4,4>", 8), ("k_blevel_up<4,4>", 16)}


def test_backend_names_the_read_out_in_the_order_of_the_header():
    """Backend.AMG_LEVEL_INFO repeats the KNP_AI_* enum of include/knpemi_hip.h by hand: same names, same order, same count"""
    import os
    import re
    from cgx_hip.backend import Backend
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "knpemi_hip.h")).read()
    enum = dict((name, int(val)) for name, val in re.findall(r"\bKNP_AI_([A-Z0-9_]+) = (\d+)", txt))
    count = enum.pop("COUNT")
    names = [n for n, _ in sorted(enum.items(), key=lambda kv: kv[1])]
    assert sorted(enum.values()) == list(range(count)) and count == len(Backend.AMG_LEVEL_INFO)

    # KNP_AI_BRT_LANES is bRt_lanes, KNP_AI_H_FUSED (of the hierarchy) is fused: the same words, whatever the letter case
    assert [(n[2:] if n.startswith("H_") else n).lower() for n in names] == [n.lower() for n in Backend.AMG_LEVEL_INFO]
