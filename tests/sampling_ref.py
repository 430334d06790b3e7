"""Independent reference of the point locator and the P1 sampling (cgx_hip/sampling.py, csrc/knp_sample.inc), and the inputs the host
and GPU tests share.

``locate_ref`` tests every (point, cell) pair: no bins, no bounding boxes.  The barycentric weights come from Cramer's rule in closed
form, evaluated in ``np.longdouble``.  The rule is the one the library states: a cell contains a point iff all dim + 1 weights are
>= -1e-9; the lowest cell index among the containing cells wins; the weights of the winner are clipped to [0, 1] and renormalised to
sum 1.  ``margin`` is the smallest |w + 1e-9| over all pairs and weights: the distance of the input from a changed decision.
"""
from __future__ import annotations

import numpy as np

TOL = 1e-9
LD = np.longdouble


def pair_weights(coords, cell, pts):
    """long-double weights [n_pts, dim + 1] of all points in one cell (vertex ids ``cell``); None for a flat cell"""
    x = np.asarray(coords, dtype=LD)[np.asarray(cell)]
    d = x.shape[1]
    e = x[1:] - x[0]                                   # rows: edge vectors
    q = np.asarray(pts, dtype=LD) - x[0]               # [n, d]
    if d == 2:
        det = e[0, 0] * e[1, 1] - e[0, 1] * e[1, 0]
        if det == 0:
            return None
        lam = [(q[:, 0] * e[1, 1] - q[:, 1] * e[1, 0]) / det, (e[0, 0] * q[:, 1] - e[0, 1] * q[:, 0]) / det]
    else:
        cr = [np.cross(e[1], e[2]), np.cross(e[2], e[0]), np.cross(e[0], e[1])]
        det = e[0] @ cr[0]
        if det == 0:
            return None
        lam = [(q @ c) / det for c in cr]
    lam = np.stack(lam, axis=1)
    return np.concatenate([1 - lam.sum(axis=1, keepdims=True), lam], axis=1)


def locate_ref(coords, cells, pts, select=None):
    """cell [n] (index into ``cells``, -1: none), weights [n, dim + 1] float64, margin.  ``select``: the cell indices searched (all)"""
    pts = np.atleast_2d(np.asarray(pts, dtype=np.float64))
    n, nv1 = pts.shape[0], cells.shape[1]
    out_c = np.full(n, -1, dtype=np.int64)
    out_w = np.zeros((n, nv1), dtype=LD)
    margin = np.inf
    for c in (range(cells.shape[0]) if select is None else select):      # ascending: the first hit of a point is its lowest cell
        w = pair_weights(coords, cells[c], pts)
        if w is None:
            continue
        margin = min(margin, float(np.abs(w + LD(TOL)).min()))
        hit = np.all(w >= -LD(TOL), axis=1) & (out_c < 0)
        out_c[hit] = c
        out_w[hit] = w[hit]
    found = out_c >= 0
    wc = np.clip(out_w[found], 0, 1)
    out_w[found] = wc / wc.sum(axis=1, keepdims=True)
    return out_c, out_w.astype(np.float64), margin


def interpolate_ref(cells, cell_side, cell, w, f_i, f_e, fill=np.nan):
    """values [n] of the merged field: sum_a w_a F[v_a] with F = f_i / f_e by the side of the point's cell, ``fill`` where cell < 0"""
    out = np.full(cell.shape[0], fill, dtype=np.float64)
    ok = cell >= 0
    v = cells[cell[ok]]
    F = np.where((np.asarray(cell_side)[cell[ok]] != 0)[:, None], np.asarray(f_e)[v], np.asarray(f_i)[v])
    acc = np.zeros(v.shape[0])
    for a in range(v.shape[1]):
        acc = acc + w[ok][:, a] * F[:, a]
    out[ok] = acc
    return out


# ---- shared inputs ---------------------------------------------------------------------------------------------------------------
def box_grid(coords, shape, widen=0.0):
    """(origin, axes, shape) of the lattice over the bounding box of ``coords``, each side moved out by ``widen`` of the extent"""
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    ext = hi - lo
    return lo - widen * ext, np.diag((1.0 + 2.0 * widen) * ext), tuple(shape)


IRREGULAR = ["delaunay2d_12", "delaunay3d_5", "hub2d_12_40", "hub3d_5_60", "hub2d_12_300", "hub3d_5_140"]
WIDENED = {2: (17, 13), 3: (9, 7, 5)}
GENERATED = {"square8": dict(N=8, kind="square"), "cube4": dict(N=4, kind="cube"), "cube8": dict(N=8, kind="cube")}

# case -> (mesh, grid): the meshes and point sets of tests/test_gpu_sampling.py
CASES = {"square8_aligned": ("square8", "aligned17"), "cube4_aligned": ("cube4", "aligned9"), "cube4_oblique": ("cube4", "oblique"),
         "two_tag": ("two_tag", "widened"), "square8_257": ("square8", "aligned257"), "cube8_five": ("cube8", "five"),
         "cube8_one": ("cube8", "one")}
CASES.update({name: (name, "widened") for name in IRREGULAR})


def mesh_config(mesh, tmp_path):
    from parity_utils import ci_config
    import irregular_meshes as IM
    if mesh in GENERATED:
        return ci_config(steps=1, **GENERATED[mesh])
    if mesh == "two_tag":
        return IM.two_tag_config(tmp_path)
    return IM.config(tmp_path, mesh)


def case_points(case, coords):
    """points [n, dim] in metres of the named case on a mesh with vertex coordinates ``coords``, and the grid (origin, axes, shape)
    they form (None for a loose point set)"""
    from cgx_hip.sampling import grid_points
    dim = coords.shape[1]
    L = coords.max(axis=0) - coords.min(axis=0)
    grid = CASES[case][1]
    if grid.startswith("aligned"):
        g = box_grid(coords, (int(grid[7:]),) * dim)
    elif grid == "widened":
        g = box_grid(coords, WIDENED[dim], 0.05)
    elif grid == "oblique":     # a plane through the cube that is parallel to no face and leaves it on two sides
        g = (coords.min(axis=0) + L * np.array([0.07, -0.04, 0.13]), np.array([[0.83, 0.21, 0.33], [-0.11, 0.97, 0.42]]) * L, (11, 9))
    elif grid == "five":
        return coords.min(axis=0) + L * np.array([[0.31, 0.52, 0.77], [0.5, 0.5, 0.5], [0.013, 0.98, 0.4], [1.2, 0.5, 0.5], [0.26, 0.26, 0.26]]), None
    elif grid == "one":
        return coords.min(axis=0) + L * np.array([[0.41, 0.37, 0.66]]), None
    xyz = grid_points(*g)
    return xyz.reshape(-1, dim), g


_REF = {}


def case_reference(case, problem):
    """(points, grid, cell, weights, margin) of the case on the problem's mesh: computed once per process, not to be written to"""
    if case not in _REF:
        lm = problem.local_mesh
        coords = np.asarray(lm.coords)
        pts, grid = case_points(case, coords)
        cell, w, margin = locate_ref(coords, np.asarray(lm.cells), pts)
        for a in (pts, cell, w):
            a.setflags(write=False)
        _REF[case] = (pts, grid, cell, w, margin)
    return _REF[case]
