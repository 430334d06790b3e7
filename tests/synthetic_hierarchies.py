"""Synthetic AMG hierarchies with prescribed row-length profiles (host only, seeded), for tests/test_gpu_amg_synthetic.py.

The hierarchies that smoothed aggregation builds from the small test meshes reach lane widths 2 to 16 of the CSR kernels and 2 to 16
of the node-blocked ones; the production meshes run at 32 and 64.  A V-cycle is a fixed composition of the uploaded matrices and needs
no Galerkin relation between them to be a well-defined operator, so the operators here are drawn at random with the AVERAGE row length
that makes ``pick_lanes`` / ``build_blocked`` choose a wanted width, and with the row lengths at which a lane loop changes its trip
count: for width L an empty row, a row of one entry, rows of 4L-1, 4L and 4L+1 entries, a row of more than 8L entries, and a long row
that ends in the last column.  (A level operator has a positive diagonal, hence no empty row; a length is capped at the number of
columns -- on the 388 unknowns of the 8 x 8 square a row of more than 512 entries does not exist, the longest row of width 64 is a
full one.)

Level operators are symmetric, strictly diagonally dominant with a positive diagonal, scaled to a mean diagonal of one; prolongators
have non-negative rows that sum to one; restrictors and the free operators of the fused cycle (S, Rt, U) have rows of unit Euclidean
norm with mixed signs.  The last entry of the longest row of every operator carries a large part of its row's weight (a third of the
Euclidean norm in the free operators, half of the off-diagonal mass in a level operator, nine tenths of the row sum in a prolongator,
where every other row also has one entry of half its sum): dropping it (a lane tail that is not summed) moves the cycle's result far
above the comparison tolerance, which test_synthetic_hierarchies_host.py asserts for every operator of every case with the constants
below -- the GPU tests import the same ones."""
from __future__ import annotations

import copy

import numpy as np
import scipy.sparse as sp

from parity_utils import fp32_stored          # noqa: F401  (also puts the package on sys.path)
from cgx_hip import amg

# ---- tolerances: the project's own (test_gpu_irregular.test_pc_apply_against_the_numpy_cycle, test_gpu_parity.test_fused_cycle_is_the_same_operator...)
TOL_FP64 = 1e-10        # per field block, max|z - z_ref| <= tol * max|z_ref|, operators stored in fp64
TOL_FP32 = 2e-6         # ... stored in fp32 (the reference rounds the same values)
TOL_DENSE = 1e-12       # the dense coarse product on its own, fp64: summation order only
GUARD = 100.0           # deleting the last entry of an operator's longest row must move the reference by GUARD * tol


def tol(fp32):
    return TOL_FP32 if fp32 else TOL_FP64


GENERIC_WIDTHS = (2, 4, 8, 16, 32, 64)
BLOCKED_WIDTHS = (2, 4, 8, 16, 32)
# average row length in the middle of the band of each width (pick_lanes: <= 8, 16, 32, 80, 192, more)
GENERIC_AVG = {2: 5.0, 4: 12.0, 8: 24.0, 16: 56.0, 32: 130.0, 64: 230.0}
# average NODE entries per node row in the band of each width (build_blocked: <= 10, 20, 44, 100, more; a restrictor counts twice)
BLOCKED_AVG = {2: 6.0, 4: 15.0, 8: 32.0, 16: 70.0, 32: 125.0}
N0_SQUARE8 = 388        # unknowns of the 8 x 8 square of ci_config: 97 nodes (25 intracellular, 72 extracellular) x 4 fields


def pick_lanes(avg):
    """knp_kernels.hip pick_lanes without the KNP_LANE_SCALE* knobs"""
    for bound, lanes in ((8.0, 2), (16.0, 4), (32.0, 8), (80.0, 16), (192.0, 32)):
        if avg <= bound:
            return lanes
    return 64


def blocked_lanes(avg_node_entries, restrictor=False):
    """knp_kernels.hip build_blocked without KNP_LANE_SCALE_B"""
    avg = (2.0 if restrictor else 1.0) * avg_node_entries
    for bound, lanes in ((10.0, 2), (20.0, 4), (44.0, 8), (100.0, 16)):
        if avg <= bound:
            return lanes
    return 32


def feasible_width(width, n_cols, table=GENERIC_AVG):
    """the widest width <= ``width`` whose band an operator with ``n_cols`` columns can reach"""
    ok = [w for w in sorted(table) if w <= width and table[w] <= 0.9 * n_cols]
    return ok[-1] if ok else min(table)


# ---- row-length profiles ---------------------------------------------------------------------------------------------------------
def edge_lengths(L, n_cols, empty=True):
    e = [1, 4 * L - 1, 4 * L, 4 * L + 1, 8 * L + 1 + L // 2]
    if empty:
        e = [0] + e
    return [min(x, n_cols) for x in e]


def row_lengths(n_rows, n_cols, L, avg, rng, empty=True, frac_empty=0.0):
    """lengths per row: the edges of width L at random rows (never the last one), the others around the mean that makes the average
    over the COUNTED rows ``avg`` -- all rows, or the non-empty ones when ``frac_empty`` leaves a compact row list (>= 20 % empty)"""
    edges = edge_lengths(L, n_cols, empty)
    n_extra = int(round(frac_empty * n_rows))
    n_bulk = n_rows - len(edges) - n_extra
    assert n_bulk >= 8, (n_rows, L)
    n_zero = n_extra + (1 if empty else 0)
    counted = n_rows - n_zero if (n_rows - n_zero) <= 0.8 * n_rows else n_rows
    mean = (avg * counted - sum(edges)) / n_bulk
    assert 1.0 <= mean <= n_cols, (mean, n_rows, n_cols, L, avg)
    w = max(0.0, min(0.4 * mean, n_cols - mean, mean - 1.0))
    bulk = np.clip(np.rint(mean + w * rng.uniform(-1.0, 1.0, n_bulk)), 1, n_cols).astype(np.int64)
    where = rng.permutation(n_rows - 1)[:len(edges) + n_extra]
    lengths = np.zeros(n_rows, dtype=np.int64)
    mask = np.ones(n_rows, dtype=bool)
    mask[where] = False
    lengths[mask] = bulk
    lengths[where[:len(edges)]] = edges
    return lengths, counted


def random_pattern(lengths, n_cols, rng, pin_rows=False):
    """CSR pattern with sorted columns and, per row, the column it is pinned to (-1: none): the longest row to the last column;
    with ``pin_rows`` every other row of two entries or more to column (row mod n_cols), so that every column below the row count has
    a row of its own.  No column stays empty where the entries allow it (the effect of a row must not end in a column nobody reads)."""
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.empty(indptr[-1], dtype=np.int64)
    star = int(np.argmax(lengths))
    pinned = np.full(len(lengths), -1, dtype=np.int64)
    pinned[star] = n_cols - 1
    if pin_rows:
        rows = np.nonzero(lengths >= 2)[0]
        pinned[rows[rows != star]] = rows[rows != star] % n_cols
    for i, k in enumerate(lengths):
        if k == 0:
            continue
        if pinned[i] >= 0:
            others = rng.permutation(n_cols - 1)[:k - 1]
            cols = np.concatenate([others + (others >= pinned[i]), [pinned[i]]])
        else:
            cols = rng.permutation(n_cols)[:k]
        indices[indptr[i]:indptr[i + 1]] = np.sort(cols)
    count = np.bincount(indices, minlength=n_cols)
    for c in np.nonzero(count == 0)[0]:
        for i in rng.permutation(len(lengths)):
            row = indices[indptr[i]:indptr[i + 1]]
            spare = [k for k in range(row.size) if count[row[k]] > 1 and row[k] != pinned[i]]
            if i != star and spare:
                k = spare[int(rng.integers(len(spare)))]
                count[row[k]] -= 1
                row[k] = c
                count[c] += 1
                row.sort()
                break
    return indptr, indices, pinned


def _values(indptr, indices, pinned, rng, kind):
    """kind 'P': non-negative, rows sum to one, a pinned entry carries half of its row (nine tenths in the longest row); 'free': mixed
    signs, rows of unit Euclidean norm, the pinned entry of the longest row carries a third of its row's weight"""
    nnz = int(indptr[-1])
    if kind == "P":
        v = rng.random(nnz) ** 3 + 0.02
    else:
        v = rng.uniform(0.2, 1.0, nnz) * rng.choice([-1.0, 1.0], nnz)
    star = int(np.argmax(np.diff(indptr)))
    for i in np.nonzero(pinned >= 0)[0]:
        a, b = indptr[i], indptr[i + 1]
        if b - a >= 2:
            k = a + int(np.searchsorted(indices[a:b], pinned[i]))
            rest = np.delete(v[a:b], k - a)
            v[k] = (9.0 if i == star else 1.0) * np.sum(rest) if kind == "P" else 0.7 * np.linalg.norm(rest)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    if kind == "P":
        s = np.bincount(rows, weights=v, minlength=len(indptr) - 1)
    else:
        s = np.sqrt(np.bincount(rows, weights=v * v, minlength=len(indptr) - 1))
    return v / s[rows]


def transfer(n_rows, n_cols, L, avg, rng, kind, frac_empty=0.0):
    lengths, _ = row_lengths(n_rows, n_cols, L, avg, rng, True, frac_empty)
    indptr, indices, pinned = random_pattern(lengths, n_cols, rng, pin_rows=(kind == "P"))
    M = sp.csr_matrix((_values(indptr, indices, pinned, rng, kind), indices, indptr), shape=(n_rows, n_cols))
    M.has_sorted_indices = True
    return M


def free_operator(n_rows, n_cols, width, rng):
    """``transfer`` of kind 'free' in the widest feasible band; a dense block with unit rows when either size is below 16"""
    if min(n_rows, n_cols) < 16:
        D = rng.uniform(0.2, 1.0, (n_rows, n_cols)) * rng.choice([-1.0, 1.0], (n_rows, n_cols))
        M = sp.csr_matrix(D / np.linalg.norm(D, axis=1)[:, None])
        M.sort_indices()
        return M
    w = feasible_width(width, n_cols)
    return transfer(n_rows, n_cols, w, GENERIC_AVG[w], rng, "free")


def symmetric_pattern(n, L, avg, rng):
    """boolean off-diagonal pattern of a symmetric operator whose rows (diagonal included) hold the edge lengths of width L exactly
    and ``avg`` entries on average; the longest row is adjacent to the last one.  Returns (pattern, longest row)."""
    edges = edge_lengths(L, n, empty=False)
    edges[-1] = min(edges[-1], n - 2)
    for k in (3, 2, 1):                      # capped lengths stay distinct rows of the profile where the size allows
        edges[k] = min(edges[k], edges[k + 1] - 1) if edges[k] >= edges[k + 1] else edges[k]
    special = [int(r) for r in rng.permutation(n - 1)[:len(edges)]]
    want = dict(zip(special, (e - 1 for e in edges)))
    M = np.zeros((n, n), dtype=bool)
    bulk = np.setdiff1d(np.arange(n), special)
    order = sorted(special, key=lambda r: -want[r])
    star = order[0]
    for idx, s in enumerate(order):
        need = want[s] - int(M[s].sum())
        assert need >= 0, (n, L, s)
        cand = [int(c) for c in rng.permutation(bulk) if not M[s, c]]
        if idx == 0 and (n - 1) in cand:
            cand.remove(n - 1)
            cand.insert(0, n - 1)
        if need > len(cand):                 # a nearly full row: the other edge rows with room left
            rest = [t for t in order[idx + 1:] if want[t] - int(M[t].sum()) > 0 and want[t] > 0]
            cand += sorted(rest, key=lambda t: -(want[t] - int(M[t].sum())))
        assert need <= len(cand), (n, L, need, len(cand))
        for c in cand[:need]:
            M[s, c] = M[c, s] = True
    for s in special:
        assert int(M[s].sum()) == want[s]
    left = int(round(avg * n)) - n - int(M.sum())
    iu = np.triu_indices(len(bulk), 1)
    m = min(max(left // 2, 0), iu[0].size)
    pick = rng.permutation(iu[0].size)[:m]
    r, c = bulk[iu[0][pick]], bulk[iu[1][pick]]
    M[r, c] = True
    M[c, r] = True
    return M, star


def sdd_values(M, star, rng):
    """symmetric, strictly diagonally dominant values on the pattern M + I; mean diagonal one"""
    n = M.shape[0]
    W = np.triu(rng.uniform(0.2, 1.0, (n, n)) * rng.choice([-1.0, 1.0], (n, n)), 1)
    W = (W + W.T) * M
    j = int(np.nonzero(M[star])[0][-1])
    others = np.abs(W[star]).sum() - abs(W[star, j])
    W[star, j] = W[j, star] = -1.0 * max(others, 1.0)
    rs = np.abs(W).sum(axis=1)
    d = (1.0 + rng.uniform(0.1, 0.6, n)) * np.maximum(rs, np.median(rs))
    A = W + np.diag(d)
    A /= d.mean()
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def level_operator(n, L, avg, rng):
    M, star = symmetric_pattern(n, L, avg, rng)
    return sdd_values(M, star, rng)


def make_level(A, P=None, R=None, S=None, Rt=None, U=None):
    dinv = 1.0 / A.diagonal()
    return amg.Level(A, dinv, amg.estimate_lambda_max(A, dinv), P, R, S, Rt, U)


# ---- node-synchronised operators: one pattern per node row, nf fields behind it ------------------------------------------------------
def expand_fields(indptr, indices, pinned, nf, rs, cs, n_rows, n_cols, rng, kind, keep=1.0):
    """node pattern -> scalar CSR with entry (rs * i + k, cs * j + k) for every node entry (i, j) and field k < nf; values per field.
    ``keep`` < 1: every field keeps a random part of the node entries (row ``star`` whole) -- patterns that differ between the fields"""
    mats = []
    lens = np.diff(indptr)
    rows_n = np.repeat(np.arange(len(lens)), lens)
    star = int(np.argmax(lens))
    for k in range(nf):
        v = _values(indptr, indices, pinned, rng, kind)
        sel = np.ones(v.size, dtype=bool)
        if keep < 1.0:
            sel = (rng.random(v.size) < keep) | (rows_n == star)
        mats.append(sp.coo_matrix((v[sel], (rs * rows_n[sel] + k, cs * indices[sel] + k)), shape=(n_rows, n_cols)))
    out = sum(mats[1:], mats[0]).tocsr()
    out.sort_indices()
    return out


def node_transfer(m_rows, m_cols, L, avg, nf, rs, cs, rng, kind, keep=1.0):
    lengths, _ = row_lengths(m_rows, m_cols, L, avg, rng)
    indptr, indices, pinned = random_pattern(lengths, m_cols, rng)
    return expand_fields(indptr, indices, pinned, nf, rs, cs, rs * m_rows, cs * m_cols, rng, kind, keep)


def node_level_operator(m, L, avg, nf, rng):
    M, star = symmetric_pattern(m, L, avg, rng)
    blocks = [sdd_values(M, star, rng).tocoo() for _ in range(nf)]
    out = sum((sp.coo_matrix((b.data, (nf * b.row + k, nf * b.col + k)), shape=(nf * m, nf * m)) for k, b in enumerate(blocks)),
              sp.coo_matrix((nf * m, nf * m))).tocsr()
    out.sort_indices()
    return out


# ---- Part A: level-by-level cycle on an uploaded level 0 ---------------------------------------------------------------------------
A_SIZES = (N0_SQUARE8, 261, 67)       # odd on purpose below level 0; 261 columns hold a row of 4 * 64 + 1 entries


def part_a_hierarchy(width, n_levels=3, dense=True, sparse_P=False, with_S=True, r_transpose=False, seed=0, sizes=A_SIZES, r_norm=None):
    """A, P and R of every level in the band of ``width`` (or the widest band their column count can reach); S, Rt and U from the
    level's A, P and R as the host setup builds them.  ``sparse_P``: 30 % of the prolongator rows are empty (compact row list)."""
    rng = np.random.default_rng([seed, width, n_levels, int(dense), int(sparse_P)])
    levels = []
    for l in range(n_levels):
        n = sizes[l]
        wa = feasible_width(width, n)
        A = level_operator(n, wa, GENERIC_AVG[wa], rng)
        if l == n_levels - 1:
            levels.append(make_level(A))
            break
        nc = sizes[l + 1]
        wp, wr = feasible_width(width, nc), feasible_width(width, n)
        P = transfer(n, nc, wp, GENERIC_AVG[wp], rng, "P", 0.3 if sparse_P else 0.0)
        R = P.T.tocsr() if r_transpose else (r_norm or R_NORM_A) * transfer(nc, n, wr, GENERIC_AVG[wr], rng, "free")
        R.sort_indices()
        lv = make_level(A, P, R)
        if with_S:
            lv.S = amg.post_smoothed_prolongator(A, lv.dinv, lv.lambda_max, P)
            if l >= 1:
                lv.Rt, lv.U = amg.coarse_fused_operators(A, lv.dinv, lv.lambda_max, R, lv.S)
        levels.append(lv)
    cinv = np.linalg.inv(levels[-1].A.toarray()) if dense else None
    return amg.Hierarchy(levels, cinv)


R_NORM_A = 12.0      # Euclidean norm of the restrictor rows of Part A: the coarse correction then weighs as much as the smoothing


OTHER_TRIPLES = [(1, 1, 2), (2, 1, 1), (0, 1, 1), (1, 0, 1), (2, 2, 3), (1, 1, 1)]      # the last one without S


def cases_a():
    """(id, dict) of Part A.  Per width and storage: a three-level V(1,1)/degree-1 cycle with S (levels >= 1 in fused form), a three-level
    cycle with one of the other parameter triples, and a two-level cycle with a compact prolongator; the endings (dense inverse or
    smoothing only) alternate so that every triple meets both."""
    out = []
    for i, w in enumerate(GENERIC_WIDTHS):
        for s, fp32 in enumerate((False, True)):
            k = 2 * i + s
            out.append(dict(width=w, fp32=fp32, levels=3, dense=(k % 2 == 0), triple=(1, 1, 1), with_S=True, sparse_P=False))
            out.append(dict(width=w, fp32=fp32, levels=3, dense=(k // 6 == 0), triple=OTHER_TRIPLES[k % 6], with_S=False, sparse_P=False))
            out.append(dict(width=w, fp32=fp32, levels=2, dense=(k // 6 == 1), triple=OTHER_TRIPLES[(k + 3) % 6], with_S=False, sparse_P=True))
    # what the rotation above leaves out: the S form with the other ending, restrictor = transposed prolongator
    out.append(dict(width=8, fp32=False, levels=3, dense=False, triple=(1, 1, 1), with_S=True, sparse_P=False, r_transpose=True))
    out.append(dict(width=16, fp32=False, levels=3, dense=True, triple=(1, 1, 1), with_S=True, sparse_P=False, r_transpose=True))
    for c in out:
        c["id"] = "w{width}-{st}-{levels}lv-{end}-v{t[0]}{t[1]}d{t[2]}{s}{p}{r}".format(
            st="fp32" if c["fp32"] else "fp64", end="dense" if c["dense"] else "smooth", t=c["triple"], s="-S" if c["with_S"] else "",
            p="-compactP" if c["sparse_P"] else "", r="-Rt" if c.get("r_transpose") else "", **{k: c[k] for k in ("width", "levels")})
    return out


def build_a(case):
    return part_a_hierarchy(case["width"], case["levels"], case["dense"], case["sparse_P"], case["with_S"], case.get("r_transpose", False),
                            r_norm=R_NORM_A * (4.0 if case["triple"][0] >= 2 else 1.0))     # two pre-sweeps leave a quarter of the residual


# ---- Part B: fused cycle, synthetic coarse levels under the library's own level 0 ------------------------------------------------------
def level0_of(P, fields):
    """level 0 of a hierarchy of one field class of the preconditioner matrix P, as amg.build_hierarchy starts it"""
    A = amg.restrict_to_fields(P, fields) if len(fields) < 4 else sp.csr_matrix(P)
    A.sort_indices()
    diag = A.diagonal()
    dinv = np.where(diag != 0.0, 1.0 / np.where(diag != 0.0, diag, 1.0), 0.0)
    return amg.Level(A, dinv, amg.estimate_lambda_max(A, dinv))


PHI_GAIN = 30.0     # the potential block of the block-triangular form also carries the Schur term cc t, ~20 x its smoothing part


def _scale_rows_level0(S, lv0, gain=1.0):
    """free S of level 0 brought to the scale of the smoothing part of the up-leg, c Dinv (b + r)"""
    return (sp.diags(gain * amg.cheby_first_coefficient(lv0.lambda_max) * lv0.dinv) @ S).tocsr()


B_NODES = {2: (37, 33), 4: (53, 49), 8: (89, 85), 16: (151, 147), 32: (281, 277)}      # node rows of levels 1 and 2 per blocked width


def part_b_blocked(P, nf, width, n_levels, seed=0, unsync=False):
    """node-synchronised hierarchy (nf = 4: all fields, 3: ion fields) whose node-blocked copies land on ``width`` lanes: S and the
    level operators at BLOCKED_AVG[width] node entries per node row, the restrictors at half of it.  ``unsync``: the fields of S on
    level 0 keep different parts of the node pattern, so that its union is refused (more than 1.25 x the stored values)."""
    rng = np.random.default_rng([seed, 11, nf, width, n_levels, int(unsync)])
    fields = tuple(range(nf))
    lv0 = level0_of(P, fields)
    m = [P.shape[0] // 4] + list(B_NODES[width][:n_levels - 1])
    levels = []
    for l in range(n_levels - 1):
        rs = 4 if l == 0 else nf          # unknowns per node in this level's vectors
        ws, wr = feasible_width(width, m[l + 1], BLOCKED_AVG), feasible_width(width, 2 * m[l], BLOCKED_AVG)
        lv = lv0 if l == 0 else make_level(node_level_operator(m[l], feasible_width(width, m[l], BLOCKED_AVG),
                                                               BLOCKED_AVG[feasible_width(width, m[l], BLOCKED_AVG)], nf, rng))
        lv.R = node_transfer(m[l + 1], m[l], wr, BLOCKED_AVG[wr] / 2.0, nf, nf, rs, rng, "free")
        lv.S = node_transfer(m[l], m[l + 1], ws, BLOCKED_AVG[ws], nf, rs, nf, rng, "free", keep=0.55 if (unsync and l == 0) else 1.0)
        lv.P = lv.R.T.tocsr()             # (not applied by the fused cycle; the upload wants one)
        lv.P.sort_indices()
        if l == 0:
            lv.S = _scale_rows_level0(lv.S, lv0)
        else:
            wu = feasible_width(width, m[l] + m[l + 1], BLOCKED_AVG)
            lv.Rt = node_transfer(m[l + 1], m[l], wr, BLOCKED_AVG[wr] / 2.0, nf, nf, nf, rng, "free")
            lv.U = node_transfer(m[l], m[l] + m[l + 1], wu, BLOCKED_AVG[wu], nf, nf, nf, rng, "free")
        levels.append(lv)
    wl = feasible_width(width, m[-1], BLOCKED_AVG)
    levels.append(make_level(node_level_operator(m[-1], wl, BLOCKED_AVG[wl], nf, rng)))
    h = amg.Hierarchy(levels, np.linalg.inv(levels[-1].A.toarray()))
    h.node_fields = nf
    return h


B_SIZES = (N0_SQUARE8, 263, 257)


def part_b_generic(P, fields, width, n_levels, seed=0, sizes=B_SIZES, coarse=None):
    """scalar hierarchy of the field class ``fields`` of P with free R, S (and Rt, U on intermediate levels) in the band of ``width``:
    the rows of S and the columns of R on level 0 are those of the class.  ``coarse``: size of the last level when it is not sizes[...]"""
    rng = np.random.default_rng([seed, 13, len(fields), width, n_levels, 0 if coarse is None else coarse])
    lv0 = level0_of(P, fields)
    n = list(sizes[:n_levels])
    if coarse is not None:
        n[-1] = coarse
    n_act = lv0.A.shape[0] // 4 * len(fields)        # unknowns of the class on level 0
    levels = []
    for l in range(n_levels - 1):
        rows = n_act if l == 0 else n[l]
        lv = lv0 if l == 0 else make_level(level_operator(n[l], feasible_width(width, n[l]), GENERIC_AVG[feasible_width(width, n[l])], rng))
        R = free_operator(n[l + 1], rows, width, rng)
        S = free_operator(rows, n[l + 1], width, rng)
        if l == 0:                         # embed the class into the 4-per-node numbering of level 0
            idx = np.array([4 * i + f for i in range(lv0.A.shape[0] // 4) for f in fields])
            E = sp.csr_matrix((np.ones(n_act), (idx, np.arange(n_act))), shape=(lv0.A.shape[0], n_act))
            R, S = (R @ E.T).tocsr(), _scale_rows_level0((E @ S).tocsr(), lv0, PHI_GAIN if tuple(fields) == (3,) else 1.0)
        else:
            lv.Rt = free_operator(n[l + 1], n[l], width, rng)
            lv.U = free_operator(n[l], n[l] + n[l + 1], width, rng)
        for M in (R, S):
            M.sort_indices()
        lv.R, lv.S, lv.P = R, S, R.T.tocsr()
        lv.P.sort_indices()
        levels.append(lv)
    if coarse is None:
        wl = feasible_width(width, n[-1])
        levels.append(make_level(level_operator(n[-1], wl, GENERIC_AVG[wl], rng)))
        cinv = np.linalg.inv(levels[-1].A.toarray())
    else:
        levels.append(make_level(sp.identity(n[-1], format="csr")))
        cinv = dense_coarse(n[-1], rng)
    return amg.Hierarchy(levels, cinv)


# ---- Part C: the dense coarse product ---------------------------------------------------------------------------------------------------
DENSE_N_FP64 = (1, 2, 126, 127, 128, 130, 256, 258, 510, 511, 512, 513, 514, 1024, 1028, 1030)
DENSE_N_FP32 = (4, 252, 256, 260, 508, 510, 512, 516, 1028, 1030)


def dense_coarse(n, rng):
    """a well-conditioned symmetric matrix in the place of the coarse inverse; the last entry of its first row carries a third of the row"""
    G = rng.standard_normal((n, n)) / np.sqrt(max(n, 1))
    C = 0.5 * (G + G.T) + 2.0 * np.eye(n)
    if n > 1:
        C[0, n - 1] = C[n - 1, 0] = 0.7 * np.linalg.norm(C[0, :n - 1])
    return np.ascontiguousarray(C)


def part_c_fp64(n, shift=0, seed=0):
    """two levels on an uploaded level 0 whose prolongator is an injection (row i holds a one in column (i + shift) mod n): with no
    smoothing, z = P Cinv R r, and z[i] is entry (i + shift) mod n of the dense product itself; shifts 0, n0, 2 n0, ... show all of it"""
    rng = np.random.default_rng([seed, 17, n])
    n0 = N0_SQUARE8
    A = level_operator(n0, 2, GENERIC_AVG[2], rng)
    R = free_operator(n, n0, 2, rng)
    P = sp.csr_matrix((np.ones(n0), (np.arange(n0), (np.arange(n0) + shift) % n)), shape=(n0, n))
    for M in (R, P):
        M.sort_indices()
    return amg.Hierarchy([make_level(A, P, R), make_level(sp.identity(n, format="csr"))], dense_coarse(n, rng))


# ---- references and the operators a case's cycle reads ------------------------------------------------------------------------------------
def restated_cycle(levels, cinv, pre, post, deg, dtype=np.float64, s_levels=()):
    """knpemi_oracle.pc_amg_vcycle restated with dense matrices in ``dtype`` (np.longdouble: what the fp64 reference is measured
    against); levels in ``s_levels`` (intermediate ones, V(1,1), degree 1) run in the fused form the library gives them when S is
    uploaded: r = b - c A Dinv b, x = c Dinv (b + r) + S x_coarse"""
    dense = lambda M: None if M is None else np.asarray(M.toarray() if sp.issparse(M) else M, dtype=dtype)
    Ls = [dict(A=dense(lv.A), P=dense(lv.P), R=dense(lv.R), S=dense(getattr(lv, "S", None)), dinv=np.asarray(lv.dinv, dtype=dtype),
               lam=dtype(lv.lambda_max)) for lv in levels]
    C = dense(cinv)
    f = dtype

    def smooth(L, b, x, zero):
        lmax, lmin = f(1.1) * L["lam"], f(0.1) * L["lam"]
        theta, delta = f(0.5) * (lmax + lmin), f(0.5) * (lmax - lmin)
        sigma = theta / delta
        rho_old = f(1.0) / sigma
        if zero:
            d = L["dinv"] * b / theta
            x = d.copy()
        else:
            d = L["dinv"] * (b - L["A"] @ x) / theta
            x = x + d
        for _ in range(1, deg):
            rho = f(1.0) / (f(2.0) * sigma - rho_old)
            d = rho * rho_old * d + (f(2.0) * rho / delta) * (L["dinv"] * (b - L["A"] @ x))
            x = x + d
            rho_old = rho
        return x

    def cycle(l, b):
        L = Ls[l]
        if l == len(Ls) - 1:
            if C is not None:
                return C @ b
            x = smooth(L, b, None, True)
            for _ in range(1, pre + post):
                x = smooth(L, b, x, False)
            return x if pre + post > 0 else np.zeros_like(b)
        if l in s_levels:
            c = f(1.0) / (f(0.5) * (f(1.1) + f(0.1)) * L["lam"])
            r = b - c * (L["A"] @ (L["dinv"] * b))
            return c * L["dinv"] * b + c * L["dinv"] * r + L["S"] @ cycle(l + 1, L["R"] @ r)
        x = None
        for _ in range(pre):
            x = smooth(L, b, x, x is None)
        if x is None:
            x = np.zeros_like(b)
        x = x + L["P"] @ cycle(l + 1, L["R"] @ (b - L["A"] @ x))
        for _ in range(post):
            x = smooth(L, b, x, False)
        return x
    return lambda r: cycle(0, np.asarray(r, dtype=dtype))


def without_last_entry_of_longest_row(M):
    """M with the last stored entry of its longest row removed (a lane tail that is not summed; a kernel that drops it does so in
    every row of that length: among equally long rows the one whose last entry is largest stands for them)"""
    M = sp.csr_matrix(M, copy=True)
    M.sort_indices()
    lens = np.diff(M.indptr)
    rows = np.nonzero(lens == lens.max())[0]
    k = M.indptr[rows + 1] - 1
    k = int(k[np.argmax(np.abs(M.data[k]))])
    M.data[k] = 0.0
    M.eliminate_zeros()
    return M


def with_operator_changed(h, level, name):
    h2 = copy.copy(h)
    h2.levels = list(h.levels)
    lv = copy.copy(h.levels[level])
    setattr(lv, name, without_last_entry_of_longest_row(getattr(lv, name)))
    h2.levels[level] = lv
    return h2


def residuals(n, count=2):
    """the seeded random residuals every case is applied to"""
    return [np.random.default_rng(3 + k).standard_normal(n) for k in range(count)]


def block_ratio(z, zref, only=None):
    """largest max|z - zref| / max|zref| over the field blocks (unknown = 4 node + field)"""
    out = []
    for fld in range(4) if only is None else only:
        s = np.max(np.abs(zref[fld::4]))
        if s > 0.0:
            out.append(float(np.max(np.abs(z[fld::4] - zref[fld::4])) / s))
    return max(out)


# ---- Part B / C cases -----------------------------------------------------------------------------------------------------------------
def strip_coarse_fused(h):
    """the hierarchy without Rt and U: what the fused cycle applies with KNP_COARSE_FUSED=0 (here they are free data, not composites of
    the level's other operators, so the reference must drop them too)"""
    h2 = copy.copy(h)
    h2.levels = []
    for lv in h.levels:
        l2 = copy.copy(lv)
        l2.Rt = l2.U = None
        h2.levels.append(l2)
    return h2


def cases_b():
    """Part B.  'blocked': node-synchronised hierarchies at every node-blocked width (fp32 storage; the same hierarchy then runs the
    scalar kernels under KNP_BLOCKED=0); 'unsync': the fields of S differ, the blocked copy is refused; 'generic': scalar hierarchies
    at every width of the generic kernels in both storages.  form 'hypre': all fields, kind KNP_PC_AMG; 'btcc': ion + potential
    hierarchy, kind KNP_PC_AMG_BT.  Every case runs with KNP_COARSE_FUSED on and off when it has three levels."""
    out = []
    for w in BLOCKED_WIDTHS:
        for form in ("hypre", "btcc"):
            for nl in (2, 3):
                out.append(dict(kind="blocked", form=form, width=w, levels=nl, fp32=True))
    for form in ("hypre", "btcc"):
        out.append(dict(kind="unsync", form=form, width=8, levels=3, fp32=True))
    for w in GENERIC_WIDTHS:
        for fp32 in (False, True):
            for form in ("hypre", "btcc"):
                out.append(dict(kind="generic", form=form, width=w, levels=3, fp32=fp32))
    out.append(dict(kind="generic", form="hypre", width=64, levels=2, fp32=False))
    out.append(dict(kind="generic", form="btcc", width=32, levels=2, fp32=True))
    for c in out:
        c["id"] = "{kind}-{form}-w{width}-{levels}lv-{st}".format(st="fp32" if c["fp32"] else "fp64", **c)
    return out


def build_b(case, P):
    """the hierarchies of a Part B case on the preconditioner matrix P of the mesh: [all fields] or [ions, potential]"""
    k, w, nl = case["kind"], case["width"], case["levels"]
    if case["form"] == "hypre":
        return [part_b_generic(P, (0, 1, 2, 3), w, nl)] if k == "generic" else [part_b_blocked(P, 4, w, nl, unsync=(k == "unsync"))]
    hp = part_b_generic(P, (3,), w, nl)
    return [part_b_generic(P, (0, 1, 2), w, nl) if k == "generic" else part_b_blocked(P, 3, w, nl, unsync=(k == "unsync")), hp]


def build_c_fp32(n, P):
    """Part C with fp32 storage: two-level ion hierarchy with a dense coarse matrix of size n, next to a small potential hierarchy"""
    return [part_b_generic(P, (0, 1, 2), 2, 2, coarse=n), part_b_generic(P, (3,), 2, 2)]


def stored(hiers, form, fp32):
    """the hierarchies as the library holds them in the fused cycle (amg.fp32_stored; the ion hierarchy's dense matrix in fp32 too)"""
    if not fp32:
        return list(hiers)
    if form == "hypre":
        return [fp32_stored(hiers[0])]
    return [fp32_stored(hiers[0], coarse=True), fp32_stored(hiers[1])]


def reference_b(form, hiers, fp32, cfused, o=None):
    """knpemi_oracle's fused cycle on the hierarchies as stored; ``cfused`` False: intermediate levels through R, A and S"""
    import knpemi_oracle as K
    hs = stored(hiers if cfused else [strip_coarse_fused(h) for h in hiers], form, fp32)
    if form == "hypre":
        return K.pc_amg_vcycle(hs[0].levels, hs[0].coarse_inv, 1, 1, 1, fused=True)
    return K.pc_btcc(o, hs[0], hs[1], 1, 1, 1, fused=True)


def operators_b(h, cfused):
    """(level, name) of the uploaded operators the fused cycle reads (level 0's own operator is the library's)"""
    nl = len(h.levels)
    ops = [(0, "R"), (0, "S")]
    for l in range(1, nl - 1):
        ops += [(l, "Rt"), (l, "U")] if cfused else [(l, "A"), (l, "R"), (l, "S")]
    return ops


def operators_a(case):
    """(level, name) of the operators a Part A case's cycle reads, and the levels that run in fused form (S uploaded, V(1,1), degree 1)"""
    nl = case["levels"]
    s_levels = tuple(range(1, nl - 1)) if (case["with_S"] and case["triple"] == (1, 1, 1)) else ()
    pre, post, deg = case["triple"]
    ops = []
    for l in range(nl - 1):
        ops += [(l, "A"), (l, "R"), (l, "S" if l in s_levels else "P")]
    if not case["dense"] and pre + post > 1 or (not case["dense"] and deg > 1):
        ops.append((nl - 1, "A"))
    return ops, s_levels


# ---- which kernels a cycle launches, from the read-out of knp_amg_get_level_info (knp_kernels.hip amg_vcycle / amg_cycle_fused) ---------
# The library reports what it CHOSE (lanes, copies, cycle form), not what it launched: the two functions below restate the launch
# sequence of amg_vcycle and amg_cycle_fused on those read-outs (the fuse_first predicate, the switch defaults -- 16 lanes for
# k_prolong_rows, 32 for the blocked kernels --, the NF/XS forms).  A change to the launch sequence in knp_kernels.hip must be repeated
# here, or the coverage table of test_gpu_amg_synthetic.py counts kernels that no longer run; every branch of the restatement is pinned
# on hand-made read-outs in test_synthetic_hierarchies_host.test_launch_restatement_and_coverage_table_are_consistent.
def launches_level_by_level(info, pre, post, deg):
    """set of (kernel family, lanes) of one amg_vcycle; ``info``: the read-out per level"""
    out = set()
    nl, nc = len(info), info[0]["nc"]

    def smooth(L, zero):
        for _ in range((0 if zero else 1) + deg - 1):
            out.add(("k_cheby", L["A_lanes"]))

    def cycle(l):
        L = info[l]
        if l == nl - 1:
            if nc > 0:
                out.add(("k_dense_matvec", nc))
            else:
                for sw in range(pre + post):
                    smooth(L, sw == 0)
            return
        fl = l > 0 and L["lfused"]
        if not fl:
            for sw in range(pre):
                smooth(L, sw == 0)
        out.add(("k_spmv", L["A_lanes"]))
        c_last = l + 1 == nl - 1
        c_first = (nc == 0 and pre + post > 0) if c_last else pre > 0
        fuse_first = c_first and not (not c_last and info[l + 1]["lfused"])
        out.add(("k_restrict_first" if fuse_first else "k_spmv", L["R_lanes"]))
        cycle(l + 1)
        if fl:
            out.add(("k_level_up", L["S_lanes"]))
            return
        out.add(("k_prolong_rows", min(L["P_lanes"], 16)) if L["P_n_act"] > 0 else ("k_spmv", L["P_lanes"]))
        for _ in range(post):
            smooth(L, False)
    cycle(0)
    return out


def launches_fused(info, nf, phi, dots=False):
    """set of (kernel family, lanes) of one amg_cycle_fused; blocked families carry their NF/XS form in the name"""
    out = set()
    nl, H = len(info), info[0]
    out.add(("k_dense_matvec", H["nc"]))
    if H["blocked"]:
        form = lambda l: f"<{nf},{4 if l == 0 else nf}>"
        if H["cfused"]:
            out.add(("k_brestrict" + form(0), info[0]["bR_lanes"]))
            for l in range(1, nl - 1):
                out.add(("k_brestrict" + form(l), info[l]["bRt_lanes"]))
                out.add(("k_brestrict" + form(l), info[l]["bU_lanes"]))
            out.add(("k_blevel_up_dots" if dots else "k_blevel_up" + form(0), info[0]["bS_lanes"]))
            return out
        for l in range(nl - 1):
            out.add(("k_brestrict" + form(l), info[l]["bR_lanes"]))
            if l + 1 < nl - 1:
                out.add((f"k_bresidual<{nf}>", info[l + 1]["bA_lanes"]))
            out.add(("k_blevel_up" + form(l), info[l]["bS_lanes"]))
        return out
    up0 = "k_level_up<1>" if phi else "k_level_up"
    if H["cfused"]:
        out.add(("k_spmv", info[0]["R_lanes"]))
        for l in range(1, nl - 1):
            out.add(("k_spmv", info[l]["Rt_lanes"]))
            out.add(("k_spmv", info[l]["U_lanes"]))
        out.add((up0, info[0]["S_lanes"]))
        return out
    for l in range(nl - 1):
        if l + 1 == nl - 1:
            out.add(("k_spmv", info[l]["R_lanes"]))
        else:
            out.add(("k_restrict_first", info[l]["R_lanes"]))
            out.add(("k_spmv", info[l + 1]["A_lanes"]))
        out.add((up0 if l == 0 else "k_level_up", info[l]["S_lanes"]))
    return out


def coverage_wanted():
    """every (kernel family, lanes, fp32 storage) the launch switches of the cycle kernels can reach"""
    want = set()
    for fp32 in (False, True):
        for w in GENERIC_WIDTHS:
            want |= {(k, w, fp32) for k in ("k_spmv", "k_cheby", "k_restrict_first", "k_level_up", "k_level_up<1>")}
        want |= {("k_prolong_rows", w, fp32) for w in (2, 4, 8, 16)}       # its switch runs every wider choice on 16 lanes
    for w in BLOCKED_WIDTHS:
        want |= {(k, w, True) for k in ("k_brestrict<4,4>", "k_brestrict<3,4>", "k_brestrict<3,3>", "k_bresidual<4>", "k_bresidual<3>",
                                        "k_blevel_up<4,4>", "k_blevel_up<3,4>", "k_blevel_up<3,3>", "k_blevel_up_dots")}
    want |= {("k_dense_matvec", n, False) for n in DENSE_N_FP64} | {("k_dense_matvec", n, True) for n in DENSE_N_FP32}
    return want
