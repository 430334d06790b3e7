"""Preconditions of tests/test_gpu_pc_tail.py, on the CPU: the long-double reference of the stages behind the preconditioner
(tests/pc_tail_ref.py) agrees with a float64 restatement, every generated case has the shape its name claims, the two meshes put
the kernels into a partial last block behind full ones, and the inputs are sensitive -- each of six wrong variants of the reference
(what a subtly wrong kernel would compute) misses the reference by at least 1e3 x the GPU tolerance somewhere, wherever the case
does not make the variant the reference itself; those exceptions are listed by ``pc_tail_ref.indistinguishable`` and asserted
(bit for bit, or a constant that the projection removes), and every variant is detected on the random pattern of every m it applies
to."""
import numpy as np
import pytest

import irregular_meshes as IM
import pc_tail_ref as T

_N = {}


def n_nodes(name):
    if name not in _N:
        _N[name] = int(IM.oracle(name).lay.n_nodes)
    return _N[name]


def _inputs(name, pattern, m):
    n = n_nodes(name)
    r = T.residual(n)
    zp = T.residual(n, seed=1)          # a z_plain that is not r: the output of some preconditioner
    return n, r, zp, T.node_mode(pattern, m, n), T.einv(m)


CASES = [(name, m, pat) for name in T.MESHES for m in T.M_VALUES for pat in T.PATTERNS]


@pytest.mark.parametrize("name", T.MESHES)
def test_meshes_end_in_a_partial_block_behind_full_ones(name):
    """delaunay2d_24 has 672 nodes and delaunay3d_7 608: three blocks of 256 threads each, the last one partial (160 and 96 nodes),
    so neither needed the next larger mesh of its family.  All nodes are owned on one rank."""
    n = n_nodes(name)
    assert n % T.BLOCK != 0 and -(-n // T.BLOCK) >= 3, n
    assert n == {"delaunay2d_24": 672, "delaunay3d_7": 608}[name]


@pytest.mark.parametrize("name,m,pattern", CASES)
def test_each_case_has_the_shape_it_claims(name, m, pattern):
    n, r, zp, md, E = _inputs(name, pattern, m)
    assert md.dtype == np.int32 and md.shape == (n,) and md.min() >= -1 and md.max() < m
    assert E.shape == (m, m) and np.abs(E).max() <= 1.0 and (m == 1 or np.abs(E - E.T).max() > 0.1)
    assert np.array_equal(md, T.node_mode(pattern, m, n)) and np.array_equal(E, T.einv(m))        # seeded
    cnt = np.bincount(md[md >= 0], minlength=m)
    sp = T.special_mode(pattern, m)
    if pattern == "random":
        assert cnt.min() >= 1 and 0.25 * n <= (md < 0).sum() <= 0.42 * n
    elif pattern == "empty_mode":
        assert cnt[sp] == 0 and np.all(np.delete(cnt, sp) >= 1)
    elif pattern == "single_node":
        assert cnt[sp] == 1 and np.all(np.delete(cnt, sp) >= 1) and sp == m - 1
    elif pattern == "one_mode":
        assert cnt[sp] == n and sp == m - 1 and cnt.sum() == n
    elif pattern == "last_block":
        start = (n - 1) // T.BLOCK * T.BLOCK
        assert start == 512 and np.all(md[:start] == -1) and np.all(md[start:] >= 0) and cnt.min() >= 1
    else:
        assert np.all(np.diff(md) <= 0) and md[0] == m - 1 and md[-1] == 0 and cnt.min() >= 1


@pytest.mark.parametrize("ns_on", [False, True])
@pytest.mark.parametrize("name,m,pattern", CASES)
def test_long_double_reference_agrees_with_float64(name, m, pattern, ns_on):
    n, r, zp, md, E = _inputs(name, pattern, m)
    z, bound = T.tail_ref(zp, r, md, E, ns_on)
    z64 = T.tail_f64(zp, r, md, E, ns_on)
    assert np.array_equal(z[0::4], zp[0::4]) and np.array_equal(z[1::4], zp[1::4]) and np.array_equal(z[2::4], zp[2::4])
    assert np.all(bound > 0)
    assert np.all(np.abs(z[3::4] - z64[3::4]) <= 1e-14 * bound)
    if not ns_on:
        assert np.array_equal(z[3::4][md < 0], zp[3::4][md < 0])
    # the Dirichlet copy restated: rows of bc_dofs take r before the correction, pinned potential rows inside a mode receive it
    bc = np.concatenate([4 * np.arange(0, n, 9) + 3, 4 * np.arange(0, n, 11) + 1])
    zb, _ = T.tail_ref(zp, r, md, E, False, bc_dofs=bc)
    zr, _ = T.tail_ref(np.where(np.isin(np.arange(4 * n), bc), r, zp), r, md, E, False)
    assert np.array_equal(zb, zr) and np.array_equal(zb[bc[bc % 4 == 1]], r[bc[bc % 4 == 1]])


@pytest.mark.parametrize("ns_on", [False, True])
@pytest.mark.parametrize("name,m,pattern", [c for c in CASES if c[1] >= 2])
def test_wrong_variants_are_detected(name, m, pattern, ns_on):
    n, r, zp, md, E = _inputs(name, pattern, m)
    z, bound = T.tail_ref(zp, r, md, E, ns_on)
    b4 = np.repeat(bound, 4)             # a correction that lands on an ion entry is measured on the node's scale
    for kind in T.WRONG:
        zw = T.tail_wrong(kind, zp, r, md, E, ns_on)
        ratio = float((np.abs(zw - z) / b4).max())
        why = T.indistinguishable(kind, pattern, m, ns_on)
        if why == "same":
            assert np.array_equal(zw, z), (kind, ratio)
        elif why == "cancels":
            assert ratio <= 1e-2 * T.GPU_TOL, (kind, ratio)
        else:
            assert ratio >= 1e3 * T.GPU_TOL, (kind, ratio)


def test_every_variant_is_detected_at_every_m_it_applies_to():
    """no variant hides behind the exceptions: the random pattern with the null space on is distinguishable for each of them"""
    for kind in T.WRONG:
        for m in T.M_VALUES:
            if m >= 2 and not (kind in ("modes_from_8_dropped", "c0_twice") and m <= 8):
                assert not T.indistinguishable(kind, "random", m, True), (kind, m)
    assert T.indistinguishable("c0_twice", "random", 8, True) and not T.indistinguishable("c0_twice", "random", 9, True)


def test_backend_keeps_pinned_potential_rows_out_of_the_modes():
    """``backend.deflation_node_modes``: -1 on every node whose potential row is a Dirichlet row (include/knpemi_hip.h,
    knp_set_deflation), the mode of the vertex or the extracellular mode elsewhere; a pinned ion row changes nothing"""
    from cgx_hip.backend import deflation_node_modes
    node_i = np.array([0, -1, 2, -1, 5], dtype=np.int32)
    node_e = np.array([-1, 1, 3, 4, -1], dtype=np.int32)
    vmode = np.array([0, -1, 1, -1, -1], dtype=np.int32)
    free = deflation_node_modes(node_i, node_e, 5, 6, vmode, 2)
    assert free.dtype == np.int32 and free.tolist() == [0, 2, 1, 2, 2, -1]
    pinned = deflation_node_modes(node_i, node_e, 5, 6, vmode, 2, bc_dofs=np.array([4 * 3 + 3, 4 * 4 + 0, 4 * 2 + 3], dtype=np.int32))
    assert pinned.tolist() == [0, 2, -1, -1, 2, -1]
