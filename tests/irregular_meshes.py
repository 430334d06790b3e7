"""Irregular meshes for the node-graph kernels: seeded Delaunay triangulations of a jittered grid, randomly renumbered, with and
without one high-valence "hub" vertex.  Every other mesh of the suite comes from ``create_unit_square`` / ``create_unit_cube``:
at most 7 (2D) / 15 (3D) pairs per node, one cell volume, one facet measure, lexicographic vertex numbers.  Here a node has up to
301 pairs, cell volumes and membrane facet measures spread over more than a factor of 3, and neighbours sit anywhere in memory.

Each generator returns ``(coords, cells, cell_tags)`` on the unit square / cube; cells whose centroid lies in (0.25, 0.75)^d carry
tag 1 (intracellular), the others tag 2.  The generators are the fixture: nothing is written to the repository.
"""
from __future__ import annotations

import copy
import math
import os

import numpy as np

from parity_utils import CI_BASE

RADIUS = {2: 0.6, 3: 0.45}          # hub ring radius in grid spacings
CLEAR = {2: 1.4, 3: 1.35}           # grid points closer than this many radii to the hub are removed


def _jittered_grid(dim, N, rng):
    ax = np.linspace(0.0, 1.0, N + 1)
    X = np.stack(np.meshgrid(*([ax] * dim), indexing="ij"), axis=-1).reshape(-1, dim)
    on_face = (X == 0.0) | (X == 1.0)                    # a boundary point moves inside its face only
    X = X + np.where(on_face, 0.0, rng.uniform(-0.3 / N, 0.3 / N, size=X.shape))
    return X


def _fibonacci_sphere(n):
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    th = math.pi * (1.0 + math.sqrt(5.0)) * k
    r = np.sqrt(1.0 - z * z)
    return np.column_stack([r * np.cos(th), r * np.sin(th), z])


def _triangulate(X, rng):
    from scipy.spatial import Delaunay
    cells = Delaunay(X).simplices.astype(np.int64)
    # flat cells between coplanar boundary points carry nothing: drop them (they sit in the boundary faces, no hole opens)
    vol = cell_volumes(X, cells)
    cells = cells[vol > 1e-9 * vol.mean()]
    perm = rng.permutation(X.shape[0])                   # new number of old vertex v: perm[v]
    coords = np.empty_like(X)
    coords[perm] = X
    cells = perm[cells]
    cells = cells[rng.permutation(cells.shape[0])]
    cx = coords[cells].mean(axis=1)
    tags = np.where(np.all((cx > 0.25) & (cx < 0.75), axis=1), 1, 2).astype(np.int32)
    return np.ascontiguousarray(coords), np.ascontiguousarray(cells.astype(np.int32)), tags


def cell_volumes(coords, cells):
    d = coords.shape[1]
    J = coords[cells][:, 1:, :] - coords[cells][:, :1, :]
    return np.abs(np.linalg.det(J)) / math.factorial(d)


def delaunay2d(N, seed=11):
    rng = np.random.default_rng(seed)
    return _triangulate(_jittered_grid(2, N, rng), rng)


def delaunay3d(N, seed=13):
    rng = np.random.default_rng(seed)
    return _triangulate(_jittered_grid(3, N, rng), rng)


def _with_hub(dim, N, ring, centre, seed):
    rng = np.random.default_rng(seed)
    X = _jittered_grid(dim, N, rng)
    c = np.asarray(centre, dtype=np.float64)
    r = RADIUS[dim] / N
    X = X[np.linalg.norm(X - c, axis=1) > CLEAR[dim] * r]
    if dim == 2:
        th = 2.0 * math.pi * (np.arange(ring) + 0.25) / ring
        R = np.column_stack([np.cos(th), np.sin(th)])
    else:
        R = _fibonacci_sphere(ring)
    return _triangulate(np.vstack([X, c[None, :], c[None, :] + r * R]), rng)


def hub2d(N, ring, centre=(0.5, 0.5), seed=17):
    """one vertex joined to ``ring`` points on a circle of radius 0.6/N around ``centre``"""
    return _with_hub(2, N, ring, centre, seed)


def hub3d(N, ring, centre=(0.5, 0.5, 0.5), seed=19):
    """one vertex joined to ``ring`` points of a Fibonacci sphere of radius 0.45/N around ``centre``"""
    return _with_hub(3, N, ring, centre, seed)


def hub_vertex(coords, centre):
    d = np.linalg.norm(coords - np.asarray(centre, dtype=np.float64), axis=1)
    v = int(np.argmin(d))
    assert d[v] == 0.0
    return v


MEMBRANE_HUB = (0.25, 0.5)

# name -> generator: the eight meshes of DESIGN.md section 4, "Irregular meshes".  The seeds of the two plain 2D meshes are the ones
# whose membrane edges span more than a factor of 3 in length (most seeds give 2 to 3 on so few membrane edges).
MESHES = {
    "delaunay2d_12": lambda: delaunay2d(12, seed=27),
    "hub2d_12_40": lambda: hub2d(12, 40),
    "hub2d_12_48m": lambda: hub2d(12, 48, centre=MEMBRANE_HUB),
    "hub2d_12_300": lambda: hub2d(12, 300),
    "delaunay3d_5": lambda: delaunay3d(5),
    "delaunay3d_7": lambda: delaunay3d(7),
    "hub3d_5_60": lambda: hub3d(5, 60),
    "hub3d_5_140": lambda: hub3d(5, 140),
    "delaunay2d_24": lambda: delaunay2d(24, seed=18),       # preconditioner cases only: three AMG levels need the unknowns
}
EIGHT = [k for k in MESHES if k != "delaunay2d_24"]

# What each mesh is for: the volume-assembly kernel ``knp_create`` must choose by itself (0 plain gather + k_cell_means, 1 staged with
# pair-major lists, 2 staged with transposed lists), whether the cell means are fused into it, the lanes per node of the assembly, and
# the trips of the assembly's ``q += G`` loop at the node with the most pairs (the SpMV runs half the lanes with two pairs in flight
# per lane: the same number of trips).
EXPECT = {
    "delaunay2d_12": {"asm_variant": 2, "fused": True, "asm_group": 8, "trips": 2},
    "hub2d_12_40": {"asm_variant": 2, "fused": True, "asm_group": 8, "trips": 6},
    "hub2d_12_48m": {"asm_variant": 2, "fused": True, "asm_group": 8, "trips": 4},
    "hub2d_12_300": {"asm_variant": 0, "fused": False, "asm_group": 8, "trips": 38},
    "delaunay3d_5": {"asm_variant": 1, "fused": True, "asm_group": 16, "trips": 2},
    "delaunay3d_7": {"asm_variant": 1, "fused": True, "asm_group": 16, "trips": 2},
    "hub3d_5_60": {"asm_variant": 1, "fused": False, "asm_group": 16, "trips": 4},
    "hub3d_5_140": {"asm_variant": 0, "fused": False, "asm_group": 16, "trips": 9},
    "delaunay2d_24": {"asm_variant": 2, "fused": True, "asm_group": 8, "trips": 2},
}


def check_launch(info, name):
    """``info`` (``Backend.launch_info()`` or ``predicted_launch``) against what the mesh is for"""
    e = EXPECT[name]
    assert info["asm_variant"] == e["asm_variant"], (name, info)
    assert (info["asm_dmax"] > 0) == e["fused"], (name, info)
    assert (info["asm_stage"] > 0) == (e["asm_variant"] > 0), (name, info)
    assert info["asm_group"] == e["asm_group"] and info["spmv_group"] == info["pc_group"] == e["asm_group"] // 2, (name, info)
    assert -(-info["max_node_pairs"] // info["asm_group"]) == e["trips"], (name, info)


# Meshes for the EMI kernels (csrc/knp_emi.inc; DESIGN.md section 4, "Irregular meshes"): a 3D hub ON the membrane, and two plain 2D
# meshes sized by the fixed grids of the EMI solver's kernels.  Kept apart from MESHES: the KNP-EMI parametrisations do not change.
MEMBRANE_HUB_3D = (0.25, 0.5, 0.5)
EMI_MESHES = {
    "hub3d_5_60m": lambda: hub3d(5, 60, centre=MEMBRANE_HUB_3D),
    "delaunay2d_92": lambda: delaunay2d(92, seed=3),
    "delaunay2d_365": lambda: delaunay2d(365, seed=3),
}


def reoriented(name, seed):
    """The named mesh with the vertex order inside every cell permuted by a seeded RNG: half the permutations are odd, so about half
    the 2D cells come out clockwise (negative edge determinant; the Delaunay generators emit counter-clockwise triangles only).
    Coordinates, tags, the vertex numbering and the order of the cells are the parent's, so the node graph is the parent's."""
    coords, cells, tags = mesh(name)
    rng = np.random.default_rng(seed)
    order = rng.permuted(np.tile(np.arange(cells.shape[1]), (cells.shape[0], 1)), axis=1)
    return coords, np.ascontiguousarray(np.take_along_axis(cells, order, axis=1)), tags


# Reoriented twins for the functional kernels and the det < 0 branch of every 2D kernel ("Irregular meshes"); the
# launch expectations of a twin are its parent's (EXPECT[PARENT[name]]): the graph is identical.
ORIENTED = {
    "delaunay2d_12_cw": lambda: reoriented("delaunay2d_12", seed=5),
    "hub2d_12_48m_cw": lambda: reoriented("hub2d_12_48m", seed=7),
}
PARENT = {"delaunay2d_12_cw": "delaunay2d_12", "hub2d_12_48m_cw": "hub2d_12_48m"}
_CACHE = {}


def mesh(name):
    """the mesh of that name, generated once per process; callers must not write into the arrays"""
    if name not in _CACHE:
        m = next(d for d in (MESHES, EMI_MESHES, ORIENTED) if name in d)[name]()
        for a in m:
            a.setflags(write=False)
        _CACHE[name] = m
    return _CACHE[name]


def two_tag(coords, cells, tags):
    """Two intracellular tags for the per-tag diagnostics: the intracellular cells split at x = 0.5 into tags 2 and 3, extracellular
    tag 1; membrane facets take the tag of their intracellular cell (``"intra"``, the convention of the tissue configs)."""
    cx = coords[cells].mean(axis=1)[:, 0]
    return np.where(tags == 1, np.where(cx < 0.5, 2, 3), 1).astype(np.int32)


def emi_arrays(name, two=False):
    """What ``ProblemEMI`` makes of the named mesh at ``mesh_conversion_factor`` 1e-6: ``(coords, cells, cell_tags, intra_tags,
    extra_tags, gamma, gamma_tags, facet_vertices)``.  ``two``: the ``two_tag`` split, membrane tag = tag of the intracellular cell
    (2 or 3); else one cell (tag 1 in 2) whose membrane carries the default tag 4."""
    from cgx_hip import mesh as meshmod
    coords, cells, tags = mesh(name)
    if two:
        tags, intra, extra, how = two_tag(coords, cells, tags), (2, 3), (1,), "intra"
    else:
        intra, extra, how = (1,), (2,), None
    gamma, gtags, fverts = meshmod.gamma_integration_entities(cells, tags, intra, extra, how)
    return coords * 1e-6, cells, tags, intra, extra, gamma, gtags, fverts


def emi_config(tmp_path, name, two=False):
    """config keys that put the named mesh (``tmp_path/<name>[_two_tag].npz``) under a ``ProblemEMI``: the arrays of ``emi_arrays``"""
    coords, cells, tags = mesh(name)
    if not two:
        path = write_npz(tmp_path, name, coords, cells, tags)
        return {"cell_tag_file": path, "facet_tag_file": path, "input_dir": "", "ics_tags": [1], "ecs_tags": [2], "membrane_tags": [4]}
    _, _, t2, _, _, _, gtags, fverts = emi_arrays(name, True)
    path = write_npz(tmp_path, name + "_two_tag", coords, cells, t2, fverts, gtags)
    return {"cell_tag_file": path, "facet_tag_file": path, "input_dir": "", "ics_tags": [2, 3], "ecs_tags": [1], "membrane_tags": [2, 3]}


def write_npz(tmp_path, name, coords, cells, tags, facets=None, facet_tags=None):
    path = os.path.join(str(tmp_path), name + ".npz")
    extra = {} if facets is None else {"facets": facets, "facet_tags": facet_tags}
    np.savez(path, coords=coords, cells=cells, cell_tags=tags, **extra)
    return path


def config(tmp_path, name, steps=1, rtol=1e-9, pc="hypre"):
    """the CI physics on the named mesh, read from ``tmp_path/name.npz`` (the route of ``two_cell_config``)"""
    path = write_npz(tmp_path, name, *mesh(name))
    cfg = copy.deepcopy(CI_BASE)
    cfg.update({"time_steps": steps, "cell_tag_file": path, "facet_tag_file": path, "input_dir": "",
                "ics_tags": [1], "ecs_tags": [2], "membrane_tags": [4], "mesh_conversion_factor": 1e-6})
    cfg["solver"]["ksp_settings"]["ksp_rtol"] = rtol
    cfg["solver"]["ksp_settings"]["pc_type"] = pc
    return cfg


def two_tag_config(tmp_path, steps=1, rtol=1e-9, pc="hypre"):
    """``delaunay3d(5)`` with two cells (tags 2, 3 in extracellular space 1) and membrane tags equal to the cell tags"""
    from cgx_hip import mesh as meshmod
    coords, cells, tags = mesh("delaunay3d_5")
    t2 = two_tag(coords, cells, tags)
    gamma, ftags, fverts = meshmod.gamma_integration_entities(cells, t2, (2, 3), (1,), "intra")
    path = write_npz(tmp_path, "delaunay3d_5_two_tag", coords, cells, t2, fverts, ftags)
    cfg = copy.deepcopy(CI_BASE)
    cfg.update({"time_steps": steps, "cell_tag_file": path, "facet_tag_file": path, "input_dir": "",
                "ics_tags": [2, 3], "ecs_tags": [1], "membrane_tags": [2, 3], "mesh_conversion_factor": 1e-6})
    cfg["solver"]["ksp_settings"]["ksp_rtol"] = rtol
    cfg["solver"]["ksp_settings"]["pc_type"] = pc
    return cfg


def oracle(name, models="ci", params=None):
    import knpemi_oracle as K
    coords, cells, tags = mesh(name)
    mdl = K.CI_MODELS() if models == "ci" else [K.Model("passive", (4,))]
    return K.OracleKNPEMI(coords.copy(), cells.copy(), tags.copy(), models=mdl, params=params, mesh_conversion_factor=1e-6)


def perturb(o, p=None):
    """The smooth, numbering-independent previous state of ``test_gpu_parity._setup`` on an oracle (and, when given, the native
    problem built on the same mesh)."""
    X = o.coords / o.coords.max()
    s = 1.0 + 0.05 * np.sin(3.0 * X[:, 0] + 1.0) * np.cos(2.0 * X[:, 1] + 0.5)
    for side in range(2):
        for j in range(3):
            o.k[side][j] = o.k[side][j] * (s if (side + j) % 2 == 0 else 2.0 - s)
    o.phi_m = o.phi_m * (2.0 - s)
    for nm in ("n", "m", "h"):
        setattr(o, nm, getattr(o, nm) * s)
    if p is not None:
        import torch
        dev = p.mesh.device
        for side in range(2):
            for j in range(3):
                p.wh[side][j].x.array[:] = torch.as_tensor(o.k[side][j], device=dev)
        p.phi_m_prev.x.array[:] = torch.as_tensor(o.phi_m, device=dev)
        for nm in ("n", "m", "h"):
            if hasattr(p, nm):
                getattr(p, nm).x.array[:] = torch.as_tensor(getattr(o, nm), device=dev)
    return s


def graph_stats(o):
    """What the launch choices of ``knp_create`` depend on, restated from the oracle's layout: per node the number of pairs (self
    included) and of same-side cells, and the zero padding of the transposed contribution lists over the stored contributions."""
    import scipy.sparse as sp
    nn = o.lay.n_nodes
    cn = o.cnode
    nv1 = cn.shape[1]
    cells_per_node = np.bincount(cn.ravel(), minlength=nn)
    r = np.repeat(cn, nv1, axis=1).ravel()
    c = np.tile(cn, (1, nv1)).ravel()
    E = sp.coo_matrix((np.ones(r.size), (r, c)), shape=(nn, nn)).tocsr()      # entry = cells shared by the pair
    pairs = np.diff(E.indptr)
    off = E.copy().tolil()
    off.setdiag(0)
    off = off.tocsr()
    off.eliminate_zeros()
    contrib = int(off.data.sum())
    tmax = np.zeros(nn)
    for n in range(nn):
        d = off.data[off.indptr[n]:off.indptr[n + 1]]
        tmax[n] = (int(d.max()) + 1) // 2 * 2 if d.size else 0
    padded = int((tmax * np.diff(off.indptr)).sum())
    return {"pairs": pairs, "cells_per_node": cells_per_node, "contrib": contrib, "padded": padded,
            "avg_pairs": pairs.sum() / nn}


def predicted_launch(o, NT=256):
    """The selection rules of ``knp_create`` restated (a prediction to pick mesh parameters with; the GPU tests assert the
    library's own read-out, ``Backend.launch_info``)."""
    g = graph_stats(o)
    avg = g["avg_pairs"]
    G0 = 4 if avg <= 4.5 else 8 if avg <= 9.0 else 16 if avg <= 20.0 else 32
    mc, dmax = int(g["cells_per_node"].max()), int(g["pairs"].max())
    out = {"asm_group": G0, "spmv_group": max(4, G0 // 2), "pc_group": max(4, G0 // 2), "max_node_cells": mc, "max_node_pairs": dmax,
           "asm_variant": 0, "asm_stage": 0, "asm_dmax": 0}
    if mc <= 255 and (NT // G0) * mc * 24 <= 48 * 1024:
        out["asm_stage"] = mc
        out["asm_variant"] = 2 if g["padded"] <= 1.5 * g["contrib"] + 1024.0 else 1
        if dmax <= 255 and (NT // G0) * (mc + dmax) * 24 <= 64 * 1024:
            out["asm_dmax"] = dmax
    return out
