"""Uniform red refinement of tagged P1 simplex meshes on the GPU, and the transfer of nodal fields from a mesh to its refinement.

Replaces (setup only) the reference's src/CGx/utils/refine_mesh.py: ``dolfinx.mesh.refine`` + ``transfer_cell_meshtag`` /
``transfer_facet_meshtag``.  The children are NOT DOLFINx's (its Plaza refinement bisects longest edges; red refinement keeps the
parents' angles): tags, geometry and conformity are the contract, not the order of the cells.  The numbering, the child tables
and the diagonal rule are stated in include/knpemi_hip.h ("mesh refinement"); the kernels are csrc/knp_refine.inc.  Per level:

    knp_refine_edge_keys  ->  torch.unique (sort + deduplication of the 64-bit keys, on the device)  ->  one read-back of
    (validation flag, number of edges)  ->  knp_refine_vertices, knp_refine_cells, knp_refine_facets  ->  one read-back of the
    missing-edge counter when there are tagged facets.

Everything stays on the device between levels; the four arrays ``load_mesh`` hands over are copied to the host once, at the end.
Like ``Backend`` there is no CPU fallback: without a HIP device ``refine`` raises ``KnpError``.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from ._lib import KnpError

INT32_MAX = 2 ** 31 - 1


def _device():
    if not torch.cuda.is_available():
        raise KnpError("No HIP device visible: meshes are refined on the GPU only (csrc/knp_refine.inc); there is no CPU fallback.")
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    rc = getattr(_lib.load(), name)(*args)
    if rc != 0:
        raise KnpError(f"{name} failed ({rc}): " + ("bad argument" if rc == -1 else "the kernel launch failed" if rc == -2 else "error"))


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def check_levels(n):
    """``refine_levels`` of a config: a non-negative integer (``ValueError`` otherwise)"""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 0:
        raise ValueError(f"refine_levels must be a non-negative integer, got {n!r}")
    return int(n)


def refine_facets_device(dim, n_vertices, unique_keys, facets, values, fine_facets=None, fine_values=None):
    """The children of tagged facets on the device: ``(fine_facets [n * 2^(dim-1), dim], fine_values, n_missing)``; a facet with an
    edge that is not among ``unique_keys`` is counted in ``n_missing`` (read back here) and its rows of the outputs are not written."""
    dev = facets.device
    n, nch = facets.shape[0], 2 ** (dim - 1)
    if fine_facets is None:
        fine_facets = torch.empty((n * nch, dim), dtype=torch.int32, device=dev)
    if fine_values is None:
        fine_values = torch.empty(n * nch, dtype=torch.int32, device=dev)
    missing = torch.zeros(1, dtype=torch.int32, device=dev)
    _call("knp_refine_facets", dim, n, n_vertices, unique_keys.numel(), _ptr(unique_keys), _ptr(facets), _ptr(values), _ptr(fine_facets),
          _ptr(fine_values), missing.data_ptr(), _stream())
    return fine_facets, fine_values, int(missing.item())


def prolong_device(edge_vertices, n_vertices, stacked, out=None):
    """One launch of knp_refine_prolong: ``stacked`` [n_fields, n_vertices] float64 (rows contiguous) -> [n_fields, n_vertices + n_edges]"""
    nf, ne = stacked.shape[0], edge_vertices.shape[0]
    if stacked.dtype != torch.float64 or stacked.dim() != 2 or stacked.shape[1] != n_vertices or stacked.stride(1) != 1:
        raise ValueError(f"prolongation: float64 rows of {n_vertices} values expected, got {tuple(stacked.shape)} {stacked.dtype}")
    if out is None:
        out = torch.empty((nf, n_vertices + ne), dtype=torch.float64, device=stacked.device)
    elif out.shape != (nf, n_vertices + ne) or out.dtype != torch.float64 or out.stride(1) != 1 or out.device != stacked.device:
        raise ValueError(f"prolongation: out must be float64 [{nf}, {n_vertices + ne}] on the device of the input")
    _call("knp_refine_prolong", nf, n_vertices, ne, _ptr(edge_vertices), _ptr(stacked), stacked.stride(0) if nf > 1 else n_vertices,
          _ptr(out), out.stride(0) if nf > 1 else n_vertices + ne, _stream())
    return out


@dataclass
class RefinedMesh:
    """The fine mesh in ``load_mesh``'s form and the record of how it came about."""
    coords: np.ndarray                 # (n_v, dim) float64
    cells: np.ndarray                  # (n_c, dim+1) int32
    cell_tags: np.ndarray              # (n_c,) int32
    facet_tags: object                 # (facet vertices [n, dim] int64, values int64), "intra" or None: as passed, refined
    levels: int
    dim: int
    n_coarse_vertices: list = field(default_factory=list)     # per level: vertices of the mesh that level refined
    n_coarse_cells: list = field(default_factory=list)
    edge_vertices: list = field(default_factory=list)         # per level: int32 [n_edges, 2] ON THE DEVICE, (a, b) of fine vertex nv + e
    diagonal: list = field(default_factory=list)              # per level: uint8 [n_coarse_cells] (3D), None in 2D

    def parent_cell(self, level=None):
        """parent (a cell of level ``level - 1``) of every cell of level ``level`` (1 .. levels, default the last)"""
        level = self.levels if level is None else int(level)
        if not 1 <= level <= self.levels:
            raise ValueError(f"level {level} of a mesh refined {self.levels} times")
        return np.arange(self.n_coarse_cells[level - 1] * 2 ** self.dim, dtype=np.int64) // 2 ** self.dim

    def prolong(self, arrays, out=None):
        """Device tensors in coarse global numbering -> in fine global numbering, through all levels: a list of 1-D float64 tensors
        (returns a list) or one tensor [n_fields, n_coarse] (returns [n_fields, n_fine]).  Enqueued on the current stream; nothing is
        copied to the host.  ``out``: a float64 device tensor [n_fields, n_fine] for the last level."""
        as_list = isinstance(arrays, (list, tuple))
        f = torch.stack([a.reshape(-1) for a in arrays]) if as_list else (arrays if arrays.dim() == 2 else arrays.reshape(1, -1))
        if self.levels == 0:
            f = f.clone() if out is None else out.copy_(f)
        for lv in range(self.levels):
            f = prolong_device(self.edge_vertices[lv], self.n_coarse_vertices[lv], f, out if lv == self.levels - 1 else None)
        if as_list:
            return list(f.unbind(0))
        return f if arrays.dim() == 2 else f.reshape(-1)

    def restrict(self, arrays):
        """injection: the values at the coarse vertices, ``a[:n_coarse]``"""
        nv = self.n_coarse_vertices[0] if self.levels else self.coords.shape[0]
        if isinstance(arrays, (list, tuple)):
            return [a[..., :nv] for a in arrays]
        return arrays[..., :nv]


def refine(coords, cells, cell_tags, facet_tags=None, levels=1):
    """Red refinement, ``levels`` times, of the mesh ``load_mesh`` returned (its first four values)."""
    levels = check_levels(levels)
    dev = _device()
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    cells = np.asarray(cells)
    if coords.ndim != 2 or coords.shape[1] not in (2, 3) or cells.ndim != 2 or cells.shape[1] != coords.shape[1] + 1:
        raise ValueError(f"refine: triangles in 2D or tetrahedra in 3D expected, got coords {coords.shape}, cells {cells.shape}")
    dim = coords.shape[1]
    if cells.size and (cells.min() < -INT32_MAX or cells.max() > INT32_MAX):
        raise ValueError("refine: a cell has a vertex index out of range")
    tagged = facet_tags is not None and not isinstance(facet_tags, str)
    x = torch.tensor(coords, device=dev)
    c = torch.tensor(np.ascontiguousarray(cells, dtype=np.int32), device=dev)
    t = torch.tensor(np.ascontiguousarray(cell_tags, dtype=np.int32), device=dev)
    if t.shape != (c.shape[0],):
        raise ValueError(f"refine: {t.numel()} cell tags for {c.shape[0]} cells")
    if tagged:
        fv_host = np.asarray(facet_tags[0]).reshape(-1, dim)
        if fv_host.size and (fv_host.min() < -INT32_MAX or fv_host.max() > INT32_MAX):
            raise ValueError("refine: a tagged facet has a vertex index out of range")
        fv = torch.tensor(np.ascontiguousarray(fv_host, dtype=np.int32), device=dev)
        fval_dtype = np.asarray(facet_tags[1]).dtype
        fvals = torch.tensor(np.ascontiguousarray(facet_tags[1], dtype=np.int32).reshape(-1), device=dev)
        if fvals.shape[0] != fv.shape[0]:
            raise ValueError(f"refine: {fvals.shape[0]} facet tags for {fv.shape[0]} facets")
    rec = RefinedMesh(None, None, None, facet_tags, levels, dim)
    nch, nedge = 2 ** dim, (dim + 1) * dim // 2
    for _ in range(levels):
        nv, nc = x.shape[0], c.shape[0]
        if nv * nv >= 2 ** 63 or nc * nch > INT32_MAX or (tagged and fv.shape[0] * 2 ** (dim - 1) > INT32_MAX):
            raise ValueError(f"refine: the fine mesh would have more than 2^31 - 1 cells or facets ({nc} cells, {nv} vertices)")
        keys = torch.empty(nc * nedge, dtype=torch.int64, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _call("knp_refine_edge_keys", dim + 1, nc, nv, _ptr(c), _ptr(keys), flag.data_ptr(), _stream())
        ukeys = torch.unique(keys)                                            # sorted; the one piece that is torch's
        ne = ukeys.numel()
        if int(flag.item()):
            raise ValueError("refine: a cell has a vertex index out of range or the same vertex twice; nothing was refined")
        if nv + ne > INT32_MAX:
            raise ValueError(f"refine: the fine mesh would have {nv + ne} vertices, more than 2^31 - 1")
        fx = torch.empty((nv + ne, dim), dtype=torch.float64, device=dev)
        ev = torch.empty((ne, 2), dtype=torch.int32, device=dev)
        _call("knp_refine_vertices", dim, nv, ne, _ptr(ukeys), _ptr(x), _ptr(fx), _ptr(ev), _stream())
        fc = torch.empty((nc * nch, dim + 1), dtype=torch.int32, device=dev)
        ft = torch.empty(nc * nch, dtype=torch.int32, device=dev)
        diag = torch.empty(nc, dtype=torch.uint8, device=dev) if dim == 3 else None
        _call("knp_refine_cells", dim, nc, nv, ne, _ptr(ukeys), _ptr(c), _ptr(t), _ptr(x), _ptr(fc), _ptr(ft), _ptr(diag), _stream())
        if tagged:
            fv, fvals, missing = refine_facets_device(dim, nv, ukeys, fv, fvals)
            if missing:
                raise ValueError(f"refine: {missing} tagged facets have an edge that no cell has (or a vertex out of range); "
                                 "they are not facets of this mesh")
        rec.n_coarse_vertices.append(nv)
        rec.n_coarse_cells.append(nc)
        rec.edge_vertices.append(ev)
        rec.diagonal.append(diag.cpu().numpy() if diag is not None else None)
        x, c, t = fx, fc, ft
    rec.coords, rec.cells, rec.cell_tags = x.cpu().numpy(), c.cpu().numpy(), t.cpu().numpy()
    if tagged:
        rec.facet_tags = (fv.cpu().numpy().astype(np.int64), fvals.cpu().numpy().astype(fval_dtype if fval_dtype.kind in "iu" else np.int64))
    return rec


def _state_functions(problem):
    """name -> Function of everything ``transfer_state`` carries, in groups (one prolongation launch per group and level)"""
    p = problem
    wh = [f for side in p.wh for f in (side if isinstance(side, (list, tuple)) else [side])]
    groups = [("wh", {f"{i}:{f.name}": f for i, f in enumerate(wh)})]
    groups.append(("phi_m_prev", {"phi_m": p.phi_m_prev} if hasattr(getattr(p, "phi_m_prev", None), "x") else {}))
    groups.append(("gates", {nm: getattr(p, nm) for nm in ("n", "m", "h") if hasattr(getattr(p, nm, None), "x")}))
    states = {}
    for m in getattr(p, "ionic_models", []):
        for st in getattr(m, "states", []):
            states[st.name] = st.function
    groups.append(("states", states))
    return groups


def transfer_state(coarse_problem, fine_problem):
    """Copies the state of ``coarse_problem`` (the solution functions ``wh``, ``phi_m_prev``, the HH gates and every state a
    mechanism declared) into ``fine_problem``, which was built with ``refine_levels`` from the same files: P1 interpolation, exact
    at the coarse vertices and the mean of the two parents at the new ones.  Both problems' ``local_mesh.l2g`` are honoured, so either
    may run with ``vertex_order: morton``.  One rank only."""
    cp, fp = coarse_problem, fine_problem
    if cp.comm.size != 1 or fp.comm.size != 1:
        raise NotImplementedError("transfer_state runs on one rank (like the samplers and the functionals)")
    rec = getattr(fp, "refinement", None)
    if rec is None or rec.levels == 0:
        raise ValueError("transfer_state: the fine problem was not built with refine_levels > 0")
    if getattr(cp, "refinement", None) is not None and cp.refinement.levels:
        raise ValueError("transfer_state: the coarse problem must be the unrefined one")
    nvc, nvf = cp.local_mesh.coords.shape[0], fp.local_mesh.coords.shape[0]
    if rec.n_coarse_vertices[0] != nvc or rec.coords.shape[0] != nvf:
        raise ValueError(f"transfer_state: the fine problem refines a mesh of {rec.n_coarse_vertices[0]} vertices, the coarse problem has {nvc}")
    dev = fp.mesh.device
    to_global = torch.as_tensor(np.argsort(cp.local_mesh.l2g), dtype=torch.long, device=dev)      # coarse local index of global vertex g
    to_local = torch.as_tensor(np.asarray(fp.local_mesh.l2g), dtype=torch.long, device=dev)       # fine global vertex of local index i
    for (what, cg), (_, fg) in zip(_state_functions(cp), _state_functions(fp)):
        if sorted(cg) != sorted(fg):
            raise ValueError(f"transfer_state: the two problems do not carry the same {what}: {sorted(cg)} on the coarse mesh, "
                             f"{sorted(fg)} on the fine one")
        if not cg:
            continue
        names = list(cg)
        fine = rec.prolong(torch.stack([cg[nm].x.array for nm in names])[:, to_global])
        for k, nm in enumerate(names):
            fg[nm].x.array[:] = fine[k][to_local]


def refine_files(mesh_dir, mesh_file, facets_file, levels=1):
    """What the reference's ``refine_mesh.py mesh_dir mesh_file facets_file`` does: reads the tagged mesh, refines it and writes
    ``<mesh_file without .xdmf>_refined.xdmf`` (+ .h5) into ``mesh_dir`` with the grids "mesh", "ct" and "ft".  Returns the path."""
    from . import xdmf
    coords, cells, tags, ft = xdmf.read_mesh_and_tags(mesh_dir + mesh_file, mesh_dir + facets_file)
    r = refine(coords, cells, tags, ft, levels)
    stem = mesh_file[:-5] if mesh_file.endswith(".xdmf") else mesh_file
    out = mesh_dir + stem + "_refined.xdmf"
    facets, fvals = r.facet_tags if r.facet_tags is not None else (None, None)
    xdmf.write_mesh_and_tags(out, r.coords, r.cells, r.cell_tags, facets, fvals)
    return out


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Refine a tagged XDMF mesh uniformly (red refinement) and write <mesh>_refined.xdmf")
    ap.add_argument("mesh_dir")
    ap.add_argument("mesh_file")
    ap.add_argument("facets_file")
    ap.add_argument("--levels", type=int, default=1)
    a = ap.parse_args(argv)
    print("Wrote " + refine_files(a.mesh_dir, a.mesh_file, a.facets_file, a.levels), flush=True)
