"""NumPy restatement of the uniform red refinement of cgx_hip/refine.py (include/knpemi_hip.h, "mesh refinement"): the fixture the
GPU tests compare the device arrays against, array for array.  Nothing here comes from the product.

Numbering.  Coarse vertices keep ``0 .. nv-1``; the unique edge ``(a, b)``, ``a < b``, gets vertex ``nv + rank of a*nv + b among
the sorted unique keys``, at ``(x[a] + x[b]) * 0.5``.  Cell ``c`` becomes the children ``2^dim c .. 2^dim c + 2^dim - 1`` in the order of
``CHILDREN``; every child has its parent's orientation.  The tables name local vertices: ``0 .. dim`` are the parent's, the
following ones the midpoints of the local edges in the order of ``EDGES``.
"""
from __future__ import annotations

import math

import numpy as np

EDGES = {2: ((0, 1), (0, 2), (1, 2)),
         3: ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))}
# 2D: 3 = m01, 4 = m02, 5 = m12: three corner triangles and the middle one
CHILDREN_2D = ((0, 3, 4), (3, 1, 5), (4, 5, 2), (3, 5, 4))
# 3D: 4 = m01, 5 = m02, 6 = m03, 7 = m12, 8 = m13, 9 = m23: four corner tetrahedra, then four around the diagonal of the octahedron
CORNERS_3D = ((0, 4, 5, 6), (4, 1, 7, 8), (5, 7, 2, 9), (6, 8, 9, 3))
INNER_3D = (((4, 9, 5, 6), (4, 9, 6, 8), (4, 9, 8, 7), (4, 9, 7, 5)),        # diagonal 0: m01-m23
            ((5, 8, 6, 4), (5, 8, 9, 6), (5, 8, 7, 9), (5, 8, 4, 7)),        # diagonal 1: m02-m13
            ((6, 7, 4, 5), (6, 7, 5, 9), (6, 7, 9, 8), (6, 7, 8, 4)))        # diagonal 2: m03-m12
DIAGONALS = ((0, 1, 2, 3), (0, 2, 1, 3), (0, 3, 1, 2))                       # (p, q, r, t): d = ((x_p + x_q) - x_r) - x_t
# a tagged facet: 2D (a, b) -> 2 = mab; 3D (a, b, c) -> 3 = mab, 4 = mac, 5 = mbc
FACET_EDGES = {2: ((0, 1),), 3: ((0, 1), (0, 2), (1, 2))}
FACET_CHILDREN = {2: ((0, 2), (2, 1)), 3: ((0, 3, 4), (3, 1, 5), (4, 5, 2), (3, 5, 4))}
TIE = 1.0 - 2.0 ** -30


def edge_keys(items, nv, edges):
    items = np.asarray(items, dtype=np.int64)
    a = np.stack([np.minimum(items[:, i], items[:, j]) for i, j in edges], axis=1)
    b = np.stack([np.maximum(items[:, i], items[:, j]) for i, j in edges], axis=1)
    return a * np.int64(nv) + b


def validate(cells, nv):
    cells = np.asarray(cells, dtype=np.int64)
    if cells.size and (cells.min() < 0 or cells.max() >= nv):
        raise ValueError("vertex index out of range")
    for i in range(cells.shape[1]):
        for j in range(i + 1, cells.shape[1]):
            if (cells[:, i] == cells[:, j]).any():
                raise ValueError("vertex twice in a cell")


def choose_diagonal(coords, cells):
    """candidate k replaces the best so far only if s_k < (1 - 2^-30) s_best; every operation rounded on its own (NumPy never fuses)"""
    X = coords[cells]                                                      # (nc, 4, 3)
    s = []
    for p, q, r, t in DIAGONALS:
        d = ((X[:, p] + X[:, q]) - X[:, r]) - X[:, t]
        s.append((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    best = np.zeros(len(cells), dtype=np.uint8)
    sb = s[0].copy()
    for k in (1, 2):
        take = s[k] < TIE * sb
        best[take] = k
        sb[take] = s[k][take]
    return best


def refine_once(coords, cells, cell_tags, facet_tags=None):
    """one level: dict with coords, cells, cell_tags, facet_tags, edge_vertices [n_edges, 2], diagonal (3D, else None)"""
    coords = np.asarray(coords, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    nv, dim = coords.shape
    validate(cells, nv)
    keys = edge_keys(cells, nv, EDGES[dim])
    ukeys = np.unique(keys)
    a, b = ukeys // nv, ukeys % nv
    fine_coords = np.vstack([coords, (coords[a] + coords[b]) * 0.5])
    local = np.concatenate([cells, nv + np.searchsorted(ukeys, keys)], axis=1)          # parent vertices, then the midpoints
    nc = len(cells)
    diag = None
    if dim == 2:
        fine = local[:, np.array(CHILDREN_2D)].reshape(nc * 4, 3)
    else:
        diag = choose_diagonal(coords, cells)
        table = np.array([CORNERS_3D + INNER_3D[k] for k in range(3)])                   # (3, 8, 4)
        fine = np.take_along_axis(local[:, None, :], table[diag].reshape(nc, 1, 32), axis=2).reshape(nc * 8, 4)
    out = {"coords": fine_coords, "cells": fine.astype(np.int32), "cell_tags": np.repeat(np.asarray(cell_tags), 2 ** dim).astype(np.int32),
           "edge_vertices": np.column_stack([a, b]).astype(np.int32), "diagonal": diag, "facet_tags": facet_tags}
    if facet_tags is not None and not isinstance(facet_tags, str):
        fv, vals = np.asarray(facet_tags[0], dtype=np.int64), np.asarray(facet_tags[1])
        fk = edge_keys(fv, nv, FACET_EDGES[dim])
        pos = np.searchsorted(ukeys, fk)
        hit = ukeys[np.minimum(pos, len(ukeys) - 1)] == fk
        bad = int((~hit.all(axis=1)).sum())
        if bad:
            raise ValueError(f"{bad} tagged facets have an edge that no cell has")
        flocal = np.concatenate([fv, nv + pos], axis=1)
        out["facet_tags"] = (flocal[:, np.array(FACET_CHILDREN[dim])].reshape(-1, dim), np.repeat(vals, 2 ** (dim - 1)))
    return out


def refine(coords, cells, cell_tags, facet_tags=None, levels=1):
    """``levels`` times ``refine_once``; returns the list of the per-level dicts (the last one is the fine mesh)"""
    out = []
    for _ in range(levels):
        r = refine_once(coords, cells, cell_tags, facet_tags)
        coords, cells, cell_tags, facet_tags = r["coords"], r["cells"], r["cell_tags"], r["facet_tags"]
        out.append(r)
    return out


def prolong(levels, f):
    """nodal values on the coarse mesh -> on the fine mesh of ``levels`` (list of ``refine_once`` dicts)"""
    f = np.asarray(f, dtype=np.float64)
    for r in levels:
        ev = r["edge_vertices"]
        f = np.concatenate([f, 0.5 * (f[ev[:, 0]] + f[ev[:, 1]])])
    return f


def signed_volumes(coords, cells):
    d = coords.shape[1]
    X = coords[np.asarray(cells, dtype=np.int64)]
    return np.linalg.det(X[:, 1:, :] - X[:, :1, :]) / math.factorial(d)


def facet_measures(coords, fverts):
    X = coords[np.asarray(fverts, dtype=np.int64)]
    if coords.shape[1] == 2:
        return np.linalg.norm(X[:, 1] - X[:, 0], axis=1)
    return 0.5 * np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)
