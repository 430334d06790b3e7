"""NumPy restatement of what ``pc_apply_proj`` (csrc/knp_kernels.hip) does behind the preconditioner B: the Dirichlet copy, the
deflation correction z += Z Einv Z^T r (k_defl_sums<8> -> k_reduce_partials -> k_defl_add) and the gauge projection (k_phi_sum ->
k_reduce_partials -> k_phi_sub), with every sum in ``np.longdouble``; and the seeded inputs of tests/test_pc_tail_host.py (which
shows them to be well-posed) and tests/test_gpu_pc_tail.py.

Unknowns are node-major, four per node: 4n + 0..2 the ions, 4n + 3 the potential.  Only potential entries take part."""
from __future__ import annotations

import numpy as np

LD = np.longdouble
M_VALUES = [1, 7, 8, 9, 32]       # modes: k_defl_sums<8> takes eight per launch -- one launch (partly, exactly) filled, a lone mode in
#                                   the second launch, and DEFL_MAX = 32 in four
PATTERNS = ["random", "empty_mode", "single_node", "one_mode", "last_block", "descending"]
BLOCK = 256                        # nodes per block of the kernels (NT)
GPU_TOL = 1e-13                    # of ``bound``: tests/test_gpu_pc_tail.py derives it
MESHES = ["delaunay2d_24", "delaunay3d_7"]


def einv(m, seed=0):
    """dense, NOT symmetric, entries uniform in [-1, 1]: a transposed index changes the answer"""
    return np.ascontiguousarray(np.random.default_rng([seed, m, 101]).uniform(-1.0, 1.0, (m, m)))


def special_mode(pattern, m):
    """the mode a pattern singles out: the empty one sits in the middle, the single-node one and the one that holds every node are the
    LAST mode (with m = 9 the lone mode of the second launch)"""
    return {"empty_mode": m // 2, "single_node": m - 1, "one_mode": m - 1}.get(pattern)


def node_mode(pattern, m, n_nodes, seed=0):
    """int32 [n_nodes], -1 = not deflated.  ``random``: about a third at -1, every mode present.  The other patterns change it as
    their name says; ``last_block``: only nodes of the last, partial block of 256 are deflated, cyclically over all modes from a
    random start, so that the block holds every mode it has room for."""
    rng = np.random.default_rng([seed, m, n_nodes, PATTERNS.index(pattern)])
    md = rng.integers(0, m, n_nodes).astype(np.int32)
    md[rng.random(n_nodes) < 1.0 / 3.0] = -1
    first = rng.permutation(n_nodes)[:m]               # every mode at least once
    md[first] = np.arange(m, dtype=np.int32)
    sp = special_mode(pattern, m)
    if pattern == "empty_mode":
        md[md == sp] = (sp + 1) % m if m > 1 else -1
    elif pattern == "single_node":
        idx = np.nonzero(md == sp)[0]
        md[idx[rng.permutation(idx.size)[1:]]] = 0 if m > 1 else -1
    elif pattern == "one_mode":
        md[:] = sp
    elif pattern == "last_block":
        start = (n_nodes - 1) // BLOCK * BLOCK
        md[:] = -1
        k = n_nodes - start
        md[start:] = (np.arange(k) + int(rng.integers(0, m))) % m
    elif pattern == "descending":
        md = ((m - 1) - (np.arange(n_nodes, dtype=np.int64) * m) // n_nodes).astype(np.int32)
    return np.ascontiguousarray(md)


def residual(n_nodes, seed=0):
    """the input vector of the tests: standard normal, [4 n_nodes]"""
    return np.random.default_rng([seed, n_nodes, 7]).standard_normal(4 * n_nodes)


def mode_sums(v_phi, md, m, dtype=LD):
    s = np.zeros(m, dtype=dtype)
    for c in range(m):
        s[c] = np.sum(v_phi[md == c].astype(dtype), dtype=dtype)
    return s


def tail_ref(z_plain, r, node_mode, Einv, ns_on, bc_dofs=None, dtype=LD):
    """(z, bound).  z_plain = B r without deflation and projection; bc_dofs: rows on which z = r is (re)stated before the correction,
    as k_bc_copy does (nothing changes when z_plain comes from the library, which has copied them already).
    s_c = sum of r[4n+3] over the nodes of mode c; z[4n+3] += sum_c Einv[mode(n), c] s_c where mode(n) >= 0 -- pinned rows included;
    then, with ``ns_on``, the mean of ALL potential entries of z is subtracted from every one of them.
    bound[n]: the scale rounding errors of entry 4n+3 are measured in (module docstring of tests/test_gpu_pc_tail.py)."""
    md = np.asarray(node_mode)
    m = Einv.shape[0]
    n = md.size
    z = np.array(z_plain, dtype=np.float64, copy=True)
    if bc_dofs is not None and len(bc_dofs):
        z[np.asarray(bc_dofs)] = r[np.asarray(bc_dofs)]
    on = md >= 0
    zphi = z[3::4].astype(dtype)
    bound = np.abs(z[3::4]).astype(np.float64)
    if m > 0 and on.any():
        s = mode_sums(r[3::4], md, m, dtype)
        sabs = mode_sums(np.abs(r[3::4]), md, m, np.float64)
        E = Einv.astype(dtype)
        zphi[on] += (E @ s)[md[on]]
        bound[on] += (np.abs(Einv) @ sabs)[md[on]]
    if ns_on:
        bound = bound + float(np.sum(np.abs(zphi), dtype=dtype) / n)
        zphi = zphi - np.sum(zphi, dtype=dtype) / dtype(n)
    z[3::4] = zphi.astype(np.float64)
    return z, bound


def tail_f64(z_plain, r, node_mode, Einv, ns_on, bc_dofs=None):
    """the same in float64 with other tools (bincount, matrix product, mean): the cross-check of the long-double reference"""
    md = np.asarray(node_mode)
    m = Einv.shape[0]
    z = np.array(z_plain, dtype=np.float64, copy=True)
    if bc_dofs is not None and len(bc_dofs):
        z[np.asarray(bc_dofs)] = r[np.asarray(bc_dofs)]
    on = md >= 0
    s = np.bincount(md[on], weights=r[3::4][on], minlength=m)
    y = Einv @ s
    zp = z[3::4].copy()
    zp[on] += y[md[on]]
    if ns_on:
        zp -= zp.mean()
    z[3::4] = zp
    return z


# ---- wrong variants of the reference: what a subtly wrong kernel would compute (tests/test_pc_tail_host.py) ----------------------
WRONG = ["einv_transposed", "modes_from_8_dropped", "c0_twice", "sums_over_z", "all_four_fields", "mean_over_deflated"]


def tail_wrong(kind, z_plain, r, node_mode, Einv, ns_on):
    md = np.asarray(node_mode)
    m = Einv.shape[0]
    n = md.size
    on = md >= 0
    z = np.array(z_plain, dtype=np.float64, copy=True)
    s = mode_sums((z_plain if kind == "sums_over_z" else r)[3::4], md, m)
    if kind == "modes_from_8_dropped":
        s[8:] = 0
    if kind == "c0_twice":           # launch c0 looks for mode c0 + (c0 + g) and stores it as mode c0 + g
        t = s.copy()
        for c in range(8, m):
            c0 = c // 8 * 8
            t[c] = s[c + c0] if c + c0 < m else 0
        s = t
    E = (Einv.T if kind == "einv_transposed" else Einv).astype(LD)
    y = np.zeros(n, dtype=LD)
    y[on] = (E @ s)[md[on]]
    zphi = z[3::4].astype(LD) + y
    if kind == "all_four_fields":
        for f in range(3):
            z[f::4] = (z[f::4].astype(LD) + y).astype(np.float64)
    if ns_on:
        zphi = zphi - (np.sum(zphi[on], dtype=LD) / LD(max(int(on.sum()), 1)) if kind == "mean_over_deflated" else np.sum(zphi, dtype=LD) / LD(n))
    z[3::4] = zphi.astype(np.float64)
    return z


def indistinguishable(kind, pattern, m, ns_on):
    """Where a wrong variant cannot be told from the reference, by construction of the case (the host test asserts each).
    "same": the variant IS the reference, bit for bit -- no mode from 8 on and a single launch up to m = 8; one populated mode reads
    the diagonal of Einv only; the mean of the deflated nodes is the mean of all where every node is deflated, and no mean is taken
    without the null space.  "cancels": with every node in one mode the correction is a constant, which the gauge projection removes
    whatever its value, so no variant of the sums or of Einv shows with the null space on (it does with it off).  None: detectable."""
    if kind != "all_four_fields" and pattern == "one_mode" and ns_on:
        return "cancels"
    if kind in ("modes_from_8_dropped", "c0_twice"):
        return "same" if m <= 8 else None
    if kind == "einv_transposed":
        return "same" if pattern == "one_mode" else None
    if kind == "mean_over_deflated":
        return "same" if not ns_on or pattern in ("one_mode", "descending") else None
    return None
