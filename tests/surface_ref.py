"""NumPy restatement of the level-set cut of include/knpemi_hip.h ("level-set surfaces"): fp64 for t = s - iso and for every decision
(inside / outside, the sign of the signed volume), long double for w, positions and fields.  Items that the level does not touch are
filtered out by array operations; the tables run item by item in Python, so the restatement shares no code path with the kernels.
The cases of tests/test_surface_host.py and tests/test_gpu_surfaces.py are generated here, once per process."""
import math

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


# ---- the definitions ------------------------------------------------------------------------------------------------------------------
def plane_s(coords, origin, normal):
    """s_v = ((x0 - o0) n0 + (x1 - o1) n1) + (x2 - o2) n2 in fp64, every operation rounded on its own"""
    x, o, n = np.asarray(coords, dtype=np.float64), np.asarray(origin, dtype=np.float64), np.asarray(normal, dtype=np.float64)
    s = (x[:, 0] - o[0]) * n[0] + (x[:, 1] - o[1]) * n[1]
    if x.shape[1] == 3:
        s = s + (x[:, 2] - o[2]) * n[2]
    return s


def parity(seq):
    inv = sum(1 for i in range(len(seq)) for j in range(i) if seq[j] > seq[i])
    return -1 if inv & 1 else 1


def volume_sign(x, v):
    """sign of det[x1 - x0, x2 - x0(, x3 - x0)] of the simplex with vertex ids ``v`` in the stored order, fp64, first row expanded"""
    e = [x[v[k + 1]] - x[v[0]] for k in range(len(v) - 1)]
    if len(v) == 4:
        c0 = e[1][1] * e[2][2] - e[1][2] * e[2][1]
        c1 = e[1][2] * e[2][0] - e[1][0] * e[2][2]
        c2 = e[1][0] * e[2][1] - e[1][1] * e[2][0]
        d = (e[0][0] * c0 + e[0][1] * c1) + e[0][2] * c2
    else:
        d = e[0][0] * e[1][1] - e[0][1] * e[1][0]
    return 1 if d > 0 else -1 if d < 0 else 0


def _flip(el, rev):
    el = list(el)
    if rev:
        el[-2], el[-1] = el[-1], el[-2]
    return el


def cut_item(v, inside, sd):
    """elements of one item as lists of (a, b) vertex pairs: ``v`` its vertex ids, ``inside`` per local vertex, ``sd`` sign of its volume"""
    ins = [k for k in range(len(v)) if inside[k]]
    out = [k for k in range(len(v)) if not inside[k]]
    c = lambda a, b: (v[a], v[b])
    if len(v) == 4:
        if len(ins) == 1:
            p, (r, t, u) = ins[0], out
            return [_flip([c(p, r), c(p, t), c(p, u)], sd * parity([p, r, t, u]) < 0)]
        if len(ins) == 3:
            (p, q, u), r = ins, out[0]
            return [_flip([c(p, r), c(q, r), c(u, r)], sd * parity([r, p, q, u]) > 0)]
        if len(ins) == 2:
            (p, q), (r, t) = ins, out
            quad, rev = [c(p, r), c(p, t), c(q, t), c(q, r)], sd * parity([p, q, r, t]) < 0
            return [_flip([quad[0], quad[1], quad[2]], rev), _flip([quad[0], quad[2], quad[3]], rev)]
        return []
    if len(ins) == 1:
        p, (r, t) = ins[0], out
        return [_flip([c(p, r), c(p, t)], sd * parity([p, r, t]) < 0)]
    if len(ins) == 2:
        (p, q), r = ins, out[0]
        return [_flip([c(p, r), c(q, r)], sd * parity([r, p, q]) > 0)]
    return []


def clip_facet(f, inside):
    """a boundary facet clipped to the inside, keeping its cyclic order"""
    n_in = sum(inside)
    own, c = (lambda a: (f[a], f[a])), (lambda a, b: (f[a], f[b]))
    if len(f) == 2:
        if n_in == 0:
            return []
        return [[own(0) if inside[0] else c(1, 0), own(1) if inside[1] else c(0, 1)]]
    if n_in == 3:
        return [[own(0), own(1), own(2)]]
    if n_in == 1:
        a = inside.index(True)
        b, cc = (a + 1) % 3, (a + 2) % 3
        return [[own(a), c(a, b), c(a, cc)]]
    if n_in == 2:
        cc = inside.index(False)
        a, b = (cc + 1) % 3, (cc + 2) % 3
        return [[own(a), own(b), c(b, cc)], [own(a), c(b, cc), c(a, cc)]]
    return []


def cut(coords, items, item_side, item_ref, s, iso, bfacets=None, bfacet_item=None):
    """The surface as a dict: ``elements`` [n, npi - 1] (output vertex numbers), ``element_item``, ``element_tag``, ``element_kind``;
    per output vertex ``a``, ``b``, ``side``, ``key`` (Python ints), ``w`` and ``xyz`` (long double); ``margin``: the smallest nonzero
    |t| over max |s| (inf without one)."""
    x = np.asarray(coords, dtype=np.float64)
    items = np.asarray(items, dtype=np.int64)
    nv, dim, npi = x.shape[0], x.shape[1], items.shape[1]
    s = np.asarray(s, dtype=np.float64)
    t = s - np.float64(iso)
    inside = t >= 0
    bad = np.isnan(t)
    finite = t[~bad]
    nz = np.abs(finite[finite != 0])
    scale = float(np.abs(s[~bad]).max()) if finite.size else 0.0
    margin = float(nz.min()) / scale if nz.size and scale > 0 else math.inf
    keys, el_item, el_tag, el_kind = [], [], [], []
    n_in = inside[items].sum(axis=1)
    touched = np.nonzero((n_in > 0) & (n_in < npi) & ~bad[items].any(axis=1))[0]
    for i in touched:
        v = [int(a) for a in items[i]]
        sd = volume_sign(x, v) if dim == npi - 1 else 1
        for el in cut_item(v, [bool(inside[a]) for a in v], sd):
            keys.append([(int(item_side[i]), a, b) for a, b in el])
            el_item.append(int(i)); el_tag.append(int(item_ref[i])); el_kind.append(0)
    if bfacets is not None and len(bfacets):
        bf, bi = np.asarray(bfacets, dtype=np.int64), np.asarray(bfacet_item, dtype=np.int64)
        for f in np.nonzero((inside[bf].sum(axis=1) > 0) & ~bad[bf].any(axis=1))[0]:
            v, it = [int(a) for a in bf[f]], int(bi[f])
            for el in clip_facet(v, [bool(inside[a]) for a in v]):
                keys.append([(int(item_side[it]), a, b) for a, b in el])
                el_item.append(it); el_tag.append(int(item_ref[it])); el_kind.append(1)
    npe = npi - 1
    as_int = lambda k: (k[0] << 62) + k[1] * nv + k[2]
    uniq = sorted({as_int(k) for el in keys for k in el})
    number = {k: n for n, k in enumerate(uniq)}
    elements = np.array([[number[as_int(k)] for k in el] for el in keys], dtype=np.int64).reshape(-1, npe)
    side = np.array([k >> 62 for k in uniq], dtype=np.int64)
    rem = [k & ((1 << 62) - 1) for k in uniq]
    a = np.array([r // nv for r in rem], dtype=np.int64)
    b = np.array([r % nv for r in rem], dtype=np.int64)
    ta, tb = t[a].astype(LD), t[b].astype(LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(a == b, LD(0), ta / (ta - tb))
    xl = x.astype(LD)
    xyz = (1 - w)[:, None] * xl[a] + w[:, None] * xl[b]
    return {"elements": elements, "element_item": np.array(el_item, dtype=np.int64), "element_tag": np.array(el_tag, dtype=np.int64),
            "element_kind": np.array(el_kind, dtype=np.int64), "a": a, "b": b, "side": side, "key": uniq, "w": w, "xyz": xyz,
            "margin": margin, "dim": dim, "npe": npe}


def gather(R, f_i, f_e):
    """(long-double values of one field pair at the output vertices of ``R``, max(|F_a|, |F_b|) per vertex)"""
    fi, fe = np.asarray(f_i, dtype=LD), np.asarray(f_e, dtype=LD)
    Fa = np.where(R["side"] == 0, fi[R["a"]], fe[R["a"]])
    Fb = np.where(R["side"] == 0, fi[R["b"]], fe[R["b"]])
    return (1 - R["w"]) * Fa + R["w"] * Fb, np.maximum(np.abs(Fa), np.abs(Fb)).astype(np.float64)


# ---- what a surface measures ------------------------------------------------------------------------------------------------------
def measures(xyz, elements):
    X = np.asarray(xyz, dtype=np.float64)[elements]
    if elements.shape[1] == 2:
        return np.linalg.norm(X[:, 1] - X[:, 0], axis=1)
    return 0.5 * np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)


def enclosed_volume(xyz, elements):
    X = np.asarray(xyz, dtype=np.float64)[elements]
    return float(np.einsum("ij,ij->i", X[:, 0], np.cross(X[:, 1], X[:, 2])).sum() / 6.0)


def topology(elements, merge=None):
    """(closed and consistently oriented: every directed edge once and its reverse once; Euler characteristic V - E + F) of a triangle
    surface; ``merge``: a label per vertex, vertices with equal labels count as one"""
    el = np.asarray(elements, dtype=np.int64)
    if merge is not None:
        _, lab = np.unique(np.asarray(merge), axis=0, return_inverse=True)
        el = lab.reshape(-1)[el]
    d = np.concatenate([el[:, [0, 1]], el[:, [1, 2]], el[:, [2, 0]]])
    n = int(el.max()) + 1 if el.size else 1
    fwd, cnt = np.unique(d[:, 0] * n + d[:, 1], return_counts=True)
    rev = np.unique(d[:, 1] * n + d[:, 0])
    closed = bool(np.all(cnt == 1) and np.array_equal(fwd, rev))
    und = np.unique(np.minimum(d[:, 0], d[:, 1]) * n + np.maximum(d[:, 0], d[:, 1]))
    return closed, len(np.unique(el)) - len(und) + len(el)


def balanced(elements):
    """every directed edge of the triangles occurs as often as its reverse (the boundary of the surface is empty, as a chain)"""
    el = np.asarray(elements, dtype=np.int64)
    d = np.concatenate([el[:, [0, 1]], el[:, [1, 2]], el[:, [2, 0]]])
    n = int(el.max()) + 1 if el.size else 1
    fwd, cf = np.unique(d[:, 0] * n + d[:, 1], return_counts=True)
    rev, cr = np.unique(d[:, 1] * n + d[:, 0], return_counts=True)
    return bool(np.array_equal(fwd, rev) and np.array_equal(cf, cr))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def permuted_cells(cells, seed):
    rng = np.random.default_rng(seed)
    order = rng.permuted(np.tile(np.arange(cells.shape[1]), (cells.shape[0], 1)), axis=1)
    return np.ascontiguousarray(np.take_along_axis(np.asarray(cells), order, axis=1))


_CUBES = {}


def cube(N, seed=3):
    """``create_unit_cube(N)`` with ``mark_subdomains_box`` tags after a random permutation of every cell's vertex order"""
    if N not in _CUBES:
        from cgx_hip import mesh as meshmod
        coords, cells = meshmod.create_unit_cube(N)
        tags = meshmod.mark_subdomains_box(coords, cells)
        _CUBES[N] = (coords, permuted_cells(cells, seed), tags)
    return _CUBES[N]


def kept_arrays(coords, cells, tags, keep, intra, boundary):
    """(items, item_side, item_ref, bfacets, bfacet_item, item_cell) of the cells whose tag is in ``keep``; ``intra``: the tags of side 0"""
    from cgx_hip.surfaces import kept_boundary
    kept = np.isin(tags, keep)
    cell = np.nonzero(kept)[0]
    side = np.where(np.isin(tags[kept], intra), 0, 1).astype(np.uint8)
    bf = bi = None
    if boundary:
        bf, bc = kept_boundary(coords, cells, kept)
        to_item = np.full(len(cells), -1, dtype=np.int64)
        to_item[cell] = np.arange(len(cell))
        bi = to_item[bc]
    return np.asarray(cells)[kept], side, np.asarray(tags)[kept], bf, bi, cell


def sphere_s(coords):
    d = np.asarray(coords, dtype=np.float64) - 0.5
    return 0.16 - ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def diagonal_s(coords, N):
    """N (x + y + z) on the vertices of ``create_unit_cube(N)``, exact: the sum of the three lattice indices"""
    return np.rint(np.asarray(coords, dtype=np.float64) * N).sum(axis=1)


OBLIQUE = (np.array([0.43, 0.51, 0.47]), np.array([0.8, -0.5, 0.33]))       # a plane through no vertex of the cubes or the irregular meshes
