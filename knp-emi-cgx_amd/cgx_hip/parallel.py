"""Domain decomposition plumbing: one process per GPU, torch.distributed (RCCL = backend "nccl").

Replaces what DOLFINx/PETSc do over MPI in the reference: mesh partitioning with a shared-facet
ghost layer (src/CGx/utils/mixed_dim_problem.py:21,649,666), ghost updates of vectors
(src/CGx/KNPEMI/KNPEMIx_solver.py:439,459,468) and the all-reduces inside KSPSolve.

Design: vertices are partitioned; each rank keeps its owned vertices plus every cell touching one
of them (one ghost-cell layer), so that all rows of owned unknowns -- including the membrane
coupling rows that need both the '+' and the '-' cell -- are assembled locally with no off-device
adds (owner computes).  Per Krylov iteration the only exchanges are (i) the ghost entries of the
SpMV input vector, sent point-to-point to the neighbouring ranks, and (ii) small all-reduces of the
Gram-Schmidt coefficients.  Both are invoked by libknpemi_hip through the two hooks of
``knp_set_comm``; the hooks are implemented here with torch.distributed.
"""
from __future__ import annotations

import os
import traceback
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.distributed as dist


class Comm:
    """Thin stand-in for the ``MPI.COMM_WORLD`` the reference passes around."""

    def __init__(self):
        if dist.is_available() and dist.is_initialized():
            self.rank, self.size, self.backend = dist.get_rank(), dist.get_world_size(), dist.get_backend()
        else:
            self.rank, self.size, self.backend = 0, 1, None

    def _reduce(self, value, op):
        if self.size == 1:
            return float(value)
        dev = "cuda" if self.backend == "nccl" else "cpu"
        t = torch.tensor([float(value)], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=op)
        return float(t.item())

    def allreduce_sum(self, v): return self._reduce(v, dist.ReduceOp.SUM) if self.size > 1 else float(v)
    def allreduce_max(self, v): return self._reduce(v, dist.ReduceOp.MAX) if self.size > 1 else float(v)

    def allreduce(self, v, op="sum"):
        return self.allreduce_max(v) if str(op).lower().endswith("max") else self.allreduce_sum(v)

    def barrier(self):
        if self.size > 1:
            dist.barrier()

    def bcast(self, obj, root=0):
        """``MPI.Comm.bcast``: a picklable object from ``root`` to every rank (gloo on the host, NCCL through the rank's device)."""
        if self.size == 1:
            return obj
        buf = [obj]
        dev = torch.device("cuda", torch.cuda.current_device()) if self.backend == "nccl" else None
        dist.broadcast_object_list(buf, src=root, device=dev)
        return buf[0]

    def all_gather_object(self, obj):
        if self.size == 1:
            return [obj]
        out = [None] * self.size
        dist.all_gather_object(out, obj)
        return out


@dataclass
class LocalMesh:
    coords: np.ndarray            # (n_v_local, dim), owned vertices first
    cells: np.ndarray             # (n_c_local, dim+1) local vertex ids, owned cells first
    cell_tags: np.ndarray
    n_vertices_owned: int
    n_cells_owned: int
    gamma: np.ndarray             # (n_g, 4) local (cell+, lf+, cell-, lf-)
    gamma_tags: np.ndarray
    l2g: np.ndarray               # global vertex id of each local vertex
    ghost_owner: np.ndarray       # owner rank of each ghost vertex (len = n_v_local - n_vertices_owned)
    n_vertices_global: int = 0
    n_cells_global: int = 0
    description: str = ""
    # deflation of near-null potential modes cut by the partition (None on one rank):
    # {"vertex_mode_i": int32 per local vertex (-1 = intra node not deflated), "ecs_mode": int, "n_modes": int,
    #  "areas": membrane measure of each deflated intra component (global), "total_area": float | None}
    defl: dict | None = None


def vertex_partition(coords, size, method=None, weights=None):
    """Owner rank of every vertex.  ``rcb`` (default): recursive coordinate bisection -- the vertex set is cut at the
    (size-proportional) median along its longest axis, recursively, which gives compact subdomains with small
    interfaces (the geometric stand-in for the reference's METIS/ParMETIS partition of the dual graph; neither is
    available here).  ``slab``: 1-D slabs along the longest axis.  Deterministic; ``KNP_PARTITION`` overrides.
    ``weights`` (per vertex, > 0): the cuts balance the weight instead of the vertex count -- ``partition_mesh`` passes the
    number of unknowns a vertex carries (membrane vertices have an intra- and an extracellular node: twice the rows, plus
    the facet quadrature), the analogue of the vertex weights one would hand to METIS for these meshes."""
    import os
    n = coords.shape[0]
    if size == 1:
        return np.zeros(n, dtype=np.int32)
    method = method or os.environ.get("KNP_PARTITION", "rcb")
    dim = coords.shape[1]

    def sorted_along(idx, ax):
        # ties broken by the remaining coordinates (lexicographic), then by index: deterministic
        keys = tuple(coords[idx, k] for k in range(dim)) + (coords[idx, ax],)
        return idx[np.lexsort(keys)]
    owner = np.empty(n, dtype=np.int32)
    w = None if weights is None else np.asarray(weights, dtype=np.float64)
    if w is not None and (w.shape != (n,) or not (w > 0).all()):
        raise ValueError("vertex weights must be positive, one per vertex")
    if method == "slab":
        ext = coords.max(axis=0) - coords.min(axis=0)
        order = sorted_along(np.arange(n), int(np.argmax(ext)))
        if w is None:
            bounds = np.linspace(0, n, size + 1).astype(np.int64)
        else:
            cw = np.cumsum(w[order])
            bounds = np.concatenate([[0], np.searchsorted(cw, cw[-1] * np.arange(1, size) / size, side="left") + 1, [n]]).astype(np.int64)
        for r in range(size):
            owner[order[bounds[r]:bounds[r + 1]]] = r
        return owner
    stack = [(np.arange(n), 0, size)]
    while stack:
        idx, r0, parts = stack.pop()
        if parts == 1:
            owner[idx] = r0
            continue
        ext = coords[idx].max(axis=0) - coords[idx].min(axis=0)
        order = sorted_along(idx, int(np.argmax(ext)))
        left = parts // 2
        if w is None:
            cut = int(round(len(order) * left / parts))
        else:
            cw = np.cumsum(w[order])
            cut = int(np.searchsorted(cw, cw[-1] * left / parts, side="left")) + 1
            cut = min(max(cut, 1), len(order) - 1) if len(order) > 1 else len(order)
        stack.append((order[:cut], r0, left))
        stack.append((order[cut:], r0 + left, parts - left))
    return owner


def extract_local(coords, cells, cell_tags, gamma, gamma_tags, vertex_owner, rank, global_ids=None,
                  n_vertices_global=None, n_cells_global=None) -> LocalMesh:
    """Cut rank ``rank``'s piece (owned vertices + one layer of ghost cells) out of a mesh that contains
    at least all cells touching the rank's vertices."""
    nvtx = coords.shape[0]
    gid = np.arange(nvtx, dtype=np.int64) if global_ids is None else np.asarray(global_ids, dtype=np.int64)
    mine = vertex_owner == rank
    cell_sel = mine[cells].any(axis=1)
    lc = np.nonzero(cell_sel)[0]
    # owned cells (each global cell counted once): owner of the cell = owner of its smallest-global-id vertex
    sub = cells[lc]
    first = sub[np.arange(len(lc)), np.argmin(gid[sub], axis=1)]
    cell_owned = vertex_owner[first] == rank
    lc = np.concatenate([lc[cell_owned], lc[~cell_owned]])
    sub = cells[lc]
    used = np.zeros(nvtx, dtype=bool)
    used[sub.ravel()] = True
    owned_v = np.nonzero(mine & used)[0]
    owned_v = np.concatenate([owned_v, np.nonzero(mine & ~used)[0]])          # isolated owned vertices (none in practice)
    owned_v = owned_v[np.argsort(gid[owned_v], kind="stable")]
    ghost_v = np.nonzero(used & ~mine)[0]
    ghost_v = ghost_v[np.argsort(gid[ghost_v], kind="stable")]
    lv = np.concatenate([owned_v, ghost_v])
    g2l = np.full(nvtx, -1, dtype=np.int64)
    g2l[lv] = np.arange(len(lv))
    lcells = g2l[sub].astype(np.int32)
    c_g2l = np.full(cells.shape[0], -1, dtype=np.int64)
    c_g2l[lc] = np.arange(len(lc))
    if gamma is not None and len(gamma):
        loc = np.array([[a for a in range(cells.shape[1]) if a != lf] for lf in range(cells.shape[1])])
        fv = cells[gamma[:, 0][:, None], loc[gamma[:, 1]]]
        gsel = mine[fv].any(axis=1)
        g = gamma[gsel].copy()
        g[:, 0] = c_g2l[g[:, 0]]
        g[:, 2] = c_g2l[g[:, 2]]
        assert (g[:, [0, 2]] >= 0).all(), "ghost layer does not contain both cells of a membrane facet"
        gt = np.asarray(gamma_tags)[gsel]
    else:
        g = np.zeros((0, 4), dtype=np.int32)
        gt = np.zeros(0, dtype=np.int32)
    return LocalMesh(coords=np.ascontiguousarray(coords[lv]), cells=np.ascontiguousarray(lcells),
                     cell_tags=np.ascontiguousarray(np.asarray(cell_tags)[lc]).astype(np.int32),
                     n_vertices_owned=len(owned_v), n_cells_owned=int(cell_owned.sum()),
                     gamma=np.ascontiguousarray(g).astype(np.int32), gamma_tags=np.ascontiguousarray(gt).astype(np.int32),
                     l2g=gid[lv], ghost_owner=vertex_owner[ghost_v].astype(np.int32),
                     n_vertices_global=int(n_vertices_global if n_vertices_global is not None else nvtx),
                     n_cells_global=int(n_cells_global if n_cells_global is not None else cells.shape[0]))


def partition_mesh(coords, cells, cell_tags, gamma, gamma_tags, size, rank, intra_tags=None, max_modes=32, method=None) -> LocalMesh:
    """Cut the global mesh for ``size`` ranks and return rank ``rank``'s part (owned vertices + one ghost-cell layer).
    ``method``: ``rcb`` (weighted recursive coordinate bisection, the default for the generated lattices), ``slab``, or ``kway`` --
    the multilevel k-way partition of the weighted nodal graph (cgx_hip/partition.py), the native counterpart of the graph
    partitioner the reference inherits from DOLFINx (mixed_dim_problem.py:21,649,666) and the default for meshes READ from files.
    ``KNP_PARTITION`` overrides.  If the graph partitioner fails the geometric one is used (never a hard error at setup)."""
    method = os.environ.get("KNP_PARTITION", method or "rcb")
    if size > 1 and method == "kway":
        try:
            from .partition import partition_mesh_vertices
            owner = partition_mesh_vertices(coords, cells, size, None if intra_tags is None else np.isin(cell_tags, intra_tags))
            lm = extract_local(coords, cells, cell_tags, gamma, gamma_tags, owner, rank)
            if intra_tags is not None:
                lm.defl = cut_component_modes(coords, cells, np.isin(cell_tags, intra_tags), gamma, owner, lm.l2g, max_modes)
            return lm
        except Exception as exc:      # noqa: BLE001
            print(f"k-way graph partition failed ({type(exc).__name__}: {exc}); falling back to coordinate bisection", flush=True)
            method = "rcb"
    wts = None
    if size > 1 and intra_tags is not None and os.environ.get("KNP_PARTITION_WEIGHTS", "1") != "0":
        # unknowns per vertex: one node per side the vertex touches (membrane vertices: two)
        is_i = np.isin(cell_tags, intra_tags)
        touch_i = np.zeros(coords.shape[0], dtype=bool)
        touch_e = np.zeros(coords.shape[0], dtype=bool)
        touch_i[np.asarray(cells)[is_i].ravel()] = True
        touch_e[np.asarray(cells)[~is_i].ravel()] = True
        wts = touch_i.astype(np.float64) + touch_e.astype(np.float64)
        wts[wts == 0.0] = 1.0
    owner = vertex_partition(coords, size, method=method if method in ("rcb", "slab") else None, weights=wts)
    lm = extract_local(coords, cells, cell_tags, gamma, gamma_tags, owner, rank)
    if size > 1 and intra_tags is not None:
        lm.defl = cut_component_modes(coords, cells, np.isin(cell_tags, intra_tags), gamma, owner, lm.l2g, max_modes)
    return lm


def cut_component_modes(coords, cells, is_intra_cell, gamma, vertex_owner, l2g, max_modes=32):
    """Deflation modes for a partitioned mesh: the extracellular space plus every connected intracellular
    component whose vertices are spread over more than one rank (a per-rank preconditioner block cannot see
    the floating-constant mode of such a component)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    nv = coords.shape[0]
    ic = cells[is_intra_cell]
    rows = np.repeat(ic[:, 0], ic.shape[1] - 1)
    cols = ic[:, 1:].ravel()
    g = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(nv, nv))
    _, lab = connected_components(g, directed=False)
    intra_v = np.zeros(nv, dtype=bool)
    intra_v[ic.ravel()] = True
    lab = np.where(intra_v, lab, -1)
    comps = np.unique(lab[intra_v])
    # cut components: more than one owner among their vertices
    cut = []
    for c in comps:
        ow = vertex_owner[lab == c]
        if ow.min() != ow.max():
            cut.append(c)
    # membrane measure per component
    d = coords.shape[1]
    loc = np.array([[a for a in range(d + 1) if a != lf] for lf in range(d + 1)])
    fv = cells[gamma[:, 0][:, None], loc[gamma[:, 1]]]
    X = coords[fv]
    meas = np.linalg.norm(X[:, 1] - X[:, 0], axis=1) if d == 2 else \
        0.5 * np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)
    fcomp = lab[fv[:, 0]]
    areas_all = {int(c): float(meas[fcomp == c].sum()) for c in comps}
    cut = sorted(cut, key=lambda c: -areas_all[int(c)])[:max(max_modes - 1, 0)]
    mode_of = {int(c): k for k, c in enumerate(cut)}
    vmode_global = np.array([mode_of.get(int(c), -1) for c in lab], dtype=np.int32)
    return {"vertex_mode_i": vmode_global[l2g], "ecs_mode": len(cut), "n_modes": len(cut) + 1,
            "areas": np.array([areas_all[int(c)] for c in cut]), "total_area": float(meas.sum())}


def morton_keys(coords: np.ndarray) -> np.ndarray:
    """Z-order (Morton) key of every point: its coordinates quantised to 21 bits (3D) / 31 bits (2D) per axis, bits interleaved"""
    x = np.asarray(coords, dtype=np.float64)
    dim = x.shape[1]
    lo = x.min(axis=0) if len(x) else np.zeros(dim)
    span = (x.max(axis=0) - lo) if len(x) else np.ones(dim)
    span = float(max(span.max(), 1e-300))              # one scale for all axes: cells of the curve stay cubes
    bits = 21 if dim == 3 else 31
    q = np.minimum(((x - lo) / span * (2 ** bits - 1)).astype(np.uint64), np.uint64(2 ** bits - 1))

    def spread3(v):
        v = (v | (v << np.uint64(32))) & np.uint64(0x1f00000000ffff)
        v = (v | (v << np.uint64(16))) & np.uint64(0x1f0000ff0000ff)
        v = (v | (v << np.uint64(8))) & np.uint64(0x100f00f00f00f00f)
        v = (v | (v << np.uint64(4))) & np.uint64(0x10c30c30c30c30c3)
        return (v | (v << np.uint64(2))) & np.uint64(0x1249249249249249)

    def spread2(v):
        v = (v | (v << np.uint64(16))) & np.uint64(0x0000ffff0000ffff)
        v = (v | (v << np.uint64(8))) & np.uint64(0x00ff00ff00ff00ff)
        v = (v | (v << np.uint64(4))) & np.uint64(0x0f0f0f0f0f0f0f0f)
        v = (v | (v << np.uint64(2))) & np.uint64(0x3333333333333333)
        return (v | (v << np.uint64(1))) & np.uint64(0x5555555555555555)
    sp_ = spread3 if dim == 3 else spread2
    key = np.zeros(len(x), dtype=np.uint64)
    for a in range(dim):
        key |= sp_(q[:, a]) << np.uint64(a)
    return key


def reorder_local_mesh(lm: LocalMesh, order: str = "morton") -> LocalMesh:
    """The same local mesh with its vertices, cells and membrane facets renumbered along a space-filling curve (owned entities stay in
    front of the ghost ones, ``l2g`` follows): unknowns that are neighbours in space become neighbours in memory, so the gathers of the
    SpMV, of the level-0 preconditioner kernels and of the assembly find more of their operands in a cache line that is already there.
    The counterpart of the graph reordering DOLFINx applies to the meshes it reads (the reference inherits it)."""
    if order in (None, "", "native", "none"):
        return lm
    if order != "morton":
        raise ValueError(f"vertex order '{order}': native | morton")
    nvo, nv = int(lm.n_vertices_owned), lm.coords.shape[0]
    key = morton_keys(lm.coords)
    perm = np.concatenate([np.argsort(key[:nvo], kind="stable"), nvo + np.argsort(key[nvo:], kind="stable")])     # new -> old
    inv = np.empty(nv, dtype=np.int64)
    inv[perm] = np.arange(nv)
    cells = inv[lm.cells].astype(lm.cells.dtype)
    nco, nc = int(lm.n_cells_owned), cells.shape[0]
    ckey = morton_keys(lm.coords[lm.cells].mean(axis=1))
    cperm = np.concatenate([np.argsort(ckey[:nco], kind="stable"), nco + np.argsort(ckey[nco:], kind="stable")])
    cinv = np.empty(nc, dtype=np.int64)
    cinv[cperm] = np.arange(nc)
    gamma = lm.gamma.copy()
    gtags = lm.gamma_tags
    if len(gamma):
        gamma[:, 0] = cinv[lm.gamma[:, 0]]
        gamma[:, 2] = cinv[lm.gamma[:, 2]]
        gorder = np.argsort(gamma[:, 0], kind="stable")
        gamma, gtags = gamma[gorder], lm.gamma_tags[gorder]
    defl = lm.defl
    if defl is not None and "vertex_mode_i" in defl:
        defl = dict(defl, vertex_mode_i=np.asarray(defl["vertex_mode_i"])[perm])
    return LocalMesh(coords=lm.coords[perm], cells=cells[cperm], cell_tags=lm.cell_tags[cperm], n_vertices_owned=nvo, n_cells_owned=nco,
                     gamma=gamma, gamma_tags=gtags, l2g=lm.l2g[perm], ghost_owner=lm.ghost_owner[perm[nvo:] - nvo] if len(lm.ghost_owner) else lm.ghost_owner,
                     n_vertices_global=lm.n_vertices_global, n_cells_global=lm.n_cells_global,
                     description=lm.description + " (vertices and cells in Morton order)", defl=defl)


def stacked_cubes_local_mesh(N, size, rank, scale=1.0) -> LocalMesh:
    """Weak-scaling workload: ``size`` unit cubes stacked along z (each with the reference's inner
    cube [0.25,0.75]^3 as one intracellular cell, reference src/CGx/utils/misc.py:256-398), N^3 boxes
    per cube, rank r owning cube r (vertex layers [rN, (r+1)N), the last rank also the top layer).
    Only the rank's slab plus its ghost layers is generated."""
    from . import mesh as meshmod
    s = N + 1
    nz_tot = N * size
    k0 = max(rank * N - 1, 0)            # first local box layer
    k1 = (rank + 1) * N                  # one past the last local box layer
    nzb = k1 - k0
    nzv = nzb + 1                        # local vertex layers k0 .. k1
    ix = np.tile(np.arange(s), s * nzv)
    iy = np.tile(np.repeat(np.arange(s), s), nzv)
    iz = np.repeat(np.arange(k0, k1 + 1), s * s)
    coords = np.column_stack([ix / float(N), iy / float(N), iz / float(N)])
    idx = np.arange(nzb * N * N)
    k, rem = np.divmod(idx, N * N)
    j, i = np.divmod(rem, N)
    v0 = k * s * s + j * s + i
    c = np.column_stack([v0, v0 + 1, v0 + s, v0 + s + 1, v0 + s * s, v0 + s * s + 1, v0 + s * s + s, v0 + s * s + s + 1])
    pat = np.array([[0, 1, 3, 7], [0, 1, 7, 5], [0, 5, 7, 4], [0, 3, 2, 7], [0, 6, 4, 7], [0, 2, 6, 7]])
    cells = c[:, pat].reshape(-1, 4).astype(np.int32)
    # intracellular: every vertex of the cell inside the inner cube of the unit cube the cell lies in
    cube_of_cell = np.repeat(np.minimum((k + k0) // N, size - 1), 6)
    zrel = iz[cells] - (cube_of_cell * N)[:, None]
    ok_xy = ((4 * ix >= N) & (4 * ix <= 3 * N) & (4 * iy >= N) & (4 * iy <= 3 * N))[cells].all(axis=1)
    ok_z = ((4 * zrel >= N) & (4 * zrel <= 3 * N)).all(axis=1)
    tags = np.where(ok_xy & ok_z, 1, 2).astype(np.int32)
    gamma, gtags, _ = meshmod.gamma_integration_entities(cells, tags, (1,), (2,), None)
    owner = np.minimum(iz // N, size - 1).astype(np.int32)
    gid = iz.astype(np.int64) * s * s + iy.astype(np.int64) * s + ix
    lm = extract_local(coords * scale, cells, tags, gamma, gtags, owner, rank, global_ids=gid,
                       n_vertices_global=(nz_tot + 1) * s * s, n_cells_global=6 * N * N * nz_tot)
    lm.description = f"{size} stacked unit cubes, N={N} (rank {rank} slab)"
    if size > 1:   # inclusions never touch a slab interface: only the extracellular constant is cut
        lm.defl = {"vertex_mode_i": np.full(lm.coords.shape[0], -1, dtype=np.int32), "ecs_mode": 0, "n_modes": 1,
                   "areas": np.zeros(0), "total_area": None}
    return lm


def stacked_squares_local_mesh(N, size, rank, scale=1.0) -> LocalMesh:
    """2D analogue of ``stacked_cubes_local_mesh``: ``size`` unit squares stacked along y, each with the
    inner square [0.25,0.75]^2 (reference src/CGx/utils/misc.py:99-195), N^2 boxes per square (right
    diagonals), rank r owning square r."""
    from . import mesh as meshmod
    s = N + 1
    ny_tot = N * size
    k0 = max(rank * N - 1, 0)
    k1 = (rank + 1) * N
    nyb = k1 - k0
    nyv = nyb + 1
    ix = np.tile(np.arange(s), nyv)
    iy = np.repeat(np.arange(k0, k1 + 1), s)
    coords = np.column_stack([ix / float(N), iy / float(N)])
    idx = np.arange(nyb * N)
    j, i = np.divmod(idx, N)
    v0 = j * s + i
    quad = np.column_stack([v0, v0 + 1, v0 + s, v0 + s + 1])
    tri = np.empty((nyb * N, 2, 3), dtype=np.int32)
    tri[:, 0, :] = quad[:, [0, 1, 3]]
    tri[:, 1, :] = quad[:, [0, 2, 3]]
    cells = tri.reshape(-1, 3)
    sq_of_cell = np.repeat(np.minimum((j + k0) // N, size - 1), 2)
    yrel = iy[cells] - (sq_of_cell * N)[:, None]
    ok_x = ((4 * ix >= N) & (4 * ix <= 3 * N))[cells].all(axis=1)
    ok_y = ((4 * yrel >= N) & (4 * yrel <= 3 * N)).all(axis=1)
    tags = np.where(ok_x & ok_y, 1, 2).astype(np.int32)
    gamma, gtags, _ = meshmod.gamma_integration_entities(cells, tags, (1,), (2,), None)
    owner = np.minimum(iy // N, size - 1).astype(np.int32)
    gid = iy.astype(np.int64) * s + ix
    lm = extract_local(coords * scale, cells, tags, gamma, gtags, owner, rank, global_ids=gid,
                       n_vertices_global=(ny_tot + 1) * s, n_cells_global=2 * N * ny_tot)
    lm.description = f"{size} stacked unit squares, N={N} (rank {rank} slab)"
    if size > 1:
        lm.defl = {"vertex_mode_i": np.full(lm.coords.shape[0], -1, dtype=np.int32), "ecs_mode": 0, "n_modes": 1,
                   "areas": np.zeros(0), "total_area": None}
    return lm


class HaloPlan:
    """DoF-level halo of the solution-vector layout (built once after the DoF layout is known): ghost DoFs are the
    4 unknowns of every ghost node, requested from the owner of the node's vertex by global vertex id and side."""

    def __init__(self, comm: Comm, lm: LocalMesh, node_i: np.ndarray, node_e: np.ndarray, device):
        from .dist_amg import LevelHalo
        self.comm = comm
        self.device = device
        send_idx, recv_idx = {}, {}
        if comm.size > 1:
            nvo = lm.n_vertices_owned
            ghosts = np.arange(nvo, lm.coords.shape[0])
            requests = {}
            for o in np.unique(lm.ghost_owner):
                sel = ghosts[lm.ghost_owner == o]
                has_i = node_i[sel] >= 0
                has_e = node_e[sel] >= 0
                requests[int(o)] = (lm.l2g[sel], has_i, has_e)
                nodes = np.stack([node_i[sel], node_e[sel]], axis=1).ravel()
                nodes = nodes[np.stack([has_i, has_e], axis=1).ravel()]
                recv_idx[int(o)] = (4 * nodes[:, None] + np.arange(4)[None, :]).ravel()
            got = exchange_arrays(comm, {o: [np.asarray(g, dtype=np.int64), hi.astype(np.int64), he.astype(np.int64)]
                                         for o, (g, hi, he) in requests.items()})
            owned_gid = lm.l2g[:nvo]
            order = np.argsort(owned_gid, kind="stable")
            sorted_gid = owned_gid[order]
            for r in sorted(got):
                gids, has_i, has_e = got[r][0], got[r][1].astype(bool), got[r][2].astype(bool)
                pos = np.searchsorted(sorted_gid, gids)
                assert (pos < len(sorted_gid)).all() and (sorted_gid[pos] == gids).all(), "halo request for a vertex this rank does not own"
                lv = order[pos]
                nodes = np.stack([node_i[lv], node_e[lv]], axis=1).ravel()
                nodes = nodes[np.stack([has_i, has_e], axis=1).ravel()]
                assert (nodes >= 0).all(), "peer requests a node this rank does not have"
                send_idx[r] = (4 * nodes[:, None] + np.arange(4)[None, :]).ravel()
        h = LevelHalo.__new__(LevelHalo)
        h.comm, h.device = comm, device
        h.n_own, h.n_loc = 0, 0
        h._finish(send_idx, recv_idx)
        self._h = h
        self.peers = h.peers
        self.send_idx, self.recv_idx = h.send_idx, h.recv_idx

    def exchange(self, x: torch.Tensor):
        """Fill the ghost entries of the local vector x (owned part first) from their owners."""
        self._h.forward(x)


def exchange_arrays(comm: Comm, out: dict) -> dict:
    """Point-to-point exchange of NumPy arrays at setup time: ``out[dest] = [array, ...]`` (int or float, 1-D) -> ``{src: [...]}``.
    Packed: every message becomes one float64 buffer ``[n_arrays, (kind, length)..., data...]`` (integers are exact in float64
    below 2^53) and the whole exchange is TWO ``all_to_all_single`` calls (sizes, payload) -- no pickling, and nobody receives
    what is not addressed to it (the object all-gather this replaces shipped every message to every rank).  Collective."""
    size, rank = comm.size, comm.rank
    if size == 1:
        return {}
    dev = torch.device("cuda") if comm.backend == "nccl" else torch.device("cpu")
    bufs = []
    for r in range(size):
        arrs = out.get(r, None) if r != rank else None
        if not arrs:
            bufs.append(np.zeros(0))
            continue
        head = [float(len(arrs))]
        for a in arrs:
            a = np.asarray(a)
            assert a.ndim == 1
            head += [0.0 if np.issubdtype(a.dtype, np.integer) else 1.0, float(a.size)]
        bufs.append(np.concatenate([np.asarray(head)] + [np.asarray(a, dtype=np.float64) for a in arrs]))
    in_splits = [int(b.size) for b in bufs]
    t_in = torch.tensor(in_splits, dtype=torch.int64, device=dev)
    t_out = torch.empty(size, dtype=torch.int64, device=dev)
    dist.all_to_all_single(t_out, t_in)
    out_splits = [int(v) for v in t_out.cpu().tolist()]
    send = torch.as_tensor(np.concatenate(bufs) if sum(in_splits) else np.zeros(0), dtype=torch.float64, device=dev)
    recv = torch.empty(sum(out_splits), dtype=torch.float64, device=dev)
    dist.all_to_all_single(recv, send, out_splits, in_splits)
    recv = recv.cpu().numpy()
    res, pos = {}, 0
    for r in range(size):
        n = out_splits[r]
        if n == 0:
            continue
        b = recv[pos:pos + n]
        pos += n
        na = int(b[0])
        kinds = b[1:1 + 2 * na:2]
        lens = b[2:2 + 2 * na:2].astype(np.int64)
        off = 1 + 2 * na
        arrs = []
        for k in range(na):
            a = b[off:off + lens[k]]
            off += lens[k]
            arrs.append(np.rint(a).astype(np.int64) if kinds[k] == 0.0 else a.copy())
        res[r] = arrs
    return res


def all_reduce_sum_(t: torch.Tensor, comm: Comm):
    """In-place SUM over ranks of a small device/CPU tensor."""
    if comm.size == 1:
        return
    if comm.backend != "nccl" and t.is_cuda:
        c = t.cpu()
        dist.all_reduce(c)
        t.copy_(c)
    else:
        dist.all_reduce(t)


def guarded(fn):
    """Wrap a ctypes callback body: never let a Python exception cross the C ABI."""
    def inner(*a):
        try:
            fn(*a)
            return 0
        except Exception:            # noqa: BLE001
            traceback.print_exc()
            return 1
    return inner
