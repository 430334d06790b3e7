"""Clipped cell surfaces, slices / iso-surfaces and isolines as geometry, cut out of the unstructured mesh on the device
(csrc/knp_surface.inc, ``knp_surface_*`` of include/knpemi_hip.h, which states the definitions and the tables).

Replaces, for runs of this project, what every plotting script of the reference does to a checkpoint with pyvista: ``threshold`` on the
cell tag and ``clip`` with a plane (utils/plot_slices.py, plot_slice_membrane.py, plot_slices_geometries.py, plot_geometries.py,
plot_geometry.py).  A ``GridSampler`` blurs a membrane that is one element thick; a surface is exact on the mesh and takes every
nodal value from the side of the membrane its element lies on.

A surface is built once (``LevelSetSurface.build``: count -> scan -> emit -> sort + deduplication of the 64-bit vertex keys -> decode
-> remap; the scan and the sort are torch's, as in cgx_hip/refine.py, everything else is HIP) and then evaluates any number of nodal
fields per call with one gather kernel, into a device tensor, without a host copy or a synchronisation.  A build reads back one count
of its own, the number of elements; ``torch.unique`` sizes its result itself.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import KnpError

FEATURE = "level-set surfaces (LevelSetSurface / ClipSurface / IsoSurface / clip_surfaces)"
MAX_SURFACE_BYTES = 2 ** 30                    # largest plan, and largest record buffer, of one surface
INT32_MAX = 2 ** 31 - 1
SurfaceVertices = namedtuple("SurfaceVertices", "a b w side")


def _call(name, *args):
    rc = getattr(_lib.load(), name)(*args)
    if rc != 0:
        raise KnpError(f"{name} failed ({rc}): " + ("bad argument" if rc == -1 else "the kernel launch failed" if rc == -2 else "error"))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def launch_info():
    """the launch geometry of the last ``knp_surface_*`` call that launched a kernel: ``_lib.SURFACE_INFO`` -> int"""
    out = (C.c_int32 * len(_lib.SURFACE_INFO))()
    _call("knp_surface_get_info", out, len(_lib.SURFACE_INFO))
    return dict(zip(_lib.SURFACE_INFO, (int(v) for v in out)))


def _one_rank(problem):
    if problem.comm.size > 1:
        raise NotImplementedError(f"{FEATURE} runs on one rank: a surface cuts this rank's owned cells only and the merge of the "
                                  "pieces over ranks is not implemented")


def _device(source):
    dev = getattr(getattr(source, "mesh", None), "device", None)
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    if torch.device(dev).type != "cuda":
        raise KnpError("No HIP device visible: surfaces are cut on the GPU only (csrc/knp_surface.inc); there is no CPU fallback.")
    return torch.device(dev)


def _nodal(f):
    return f.x.array if hasattr(f, "x") else f


def outward_facets(coords, cells, cell, local_facet):
    """vertex ids [n, d] of facet ``local_facet`` (opposite that local vertex) of every listed cell, in an order whose normal points
    out of the cell: 3D (v1 - v0) x (v2 - v0) away from the opposite vertex, 2D the cell to the left of v0 -> v1"""
    cells = np.asarray(cells)
    nv = cells.shape[1]
    loc = np.array([[a for a in range(nv) if a != lf] for lf in range(nv)])
    cv = cells[cell]
    fv = np.take_along_axis(cv, loc[local_facet], axis=1).astype(np.int64)
    opp = np.take_along_axis(cv, np.asarray(local_facet)[:, None], axis=1)[:, 0]
    X, xo = coords[fv], coords[opp]
    if nv == 4:
        out = np.einsum("ij,ij->i", np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), X[:, 0] - xo)
    else:
        e, d = X[:, 1] - X[:, 0], xo - X[:, 0]
        out = e[:, 0] * d[:, 1] - e[:, 1] * d[:, 0]
    flip = out < 0
    fv[flip, -2], fv[flip, -1] = fv[flip, -1].copy(), fv[flip, -2].copy()
    return fv


def kept_boundary(coords, cells, kept, facets=None):
    """(boundary facets [n, d] oriented out of their kept cell, that cell's index) of the set of cells ``kept`` (a mask): the facets
    with exactly one kept neighbour, ascending in ``mesh.build_facets``' order.  ``facets``: that function's result, to reuse it."""
    from . import mesh as meshmod
    _, c0, l0, c1, l1 = meshmod.build_facets(np.asarray(cells)) if facets is None else facets
    k0 = kept[c0]
    k1 = np.zeros_like(k0)
    k1[c1 >= 0] = kept[c1[c1 >= 0]]
    sel = np.nonzero(k0 ^ k1)[0]
    cell = np.where(k0[sel], c0[sel], c1[sel])
    lf = np.where(k0[sel], l0[sel], l1[sel])
    return outward_facets(np.asarray(coords), cells, cell, lf), cell


class LevelSetSurface:
    """The level-set cut of ``items`` [n, 3 | 4] (vertex ids into the source's vertices).  ``source``: a problem (its
    ``local_mesh.coords``) or a coordinate array [n_vertices, dim]; ``item_side`` (0 intracellular, 1 extracellular; default 0) and
    ``item_ref`` (the tag an element carries; default 0) per item; ``bfacets`` [m, npi - 1] with ``bfacet_item`` [m]: boundary facets,
    oriented out of the item they belong to, which are clipped to the inside and added to the cut faces.

    After ``build(s, iso)``: ``n_elements``, ``elements`` [n, npi - 1] (output vertex numbers), ``element_item``, ``element_tag``,
    ``element_kind`` (0 cut, 1 boundary), ``n_vertices``, ``vertices`` (a, b, w, side) and ``xyz`` [n_vertices, dim] -- all device
    tensors.  A call evaluates nodal fields at the output vertices."""

    def __init__(self, source, items, item_side=None, item_ref=None, bfacets=None, bfacet_item=None):
        coords = source.local_mesh.coords if hasattr(source, "local_mesh") else source
        if hasattr(source, "comm"):
            _one_rank(source)
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        items = np.asarray(items)
        if coords.ndim != 2 or coords.shape[1] not in (2, 3) or coords.shape[0] < 1:
            raise ValueError(f"a surface needs vertex coordinates [n, 2 | 3], got {coords.shape}")
        dim = coords.shape[1]
        if items.ndim != 2 or items.shape[1] not in (3, 4) or items.shape[1] > dim + 1:
            raise ValueError(f"items are triangles (2D cells, 3D membrane facets) or tetrahedra (3D cells), got {items.shape} in {dim}D")
        n, npi = items.shape
        nb = 0 if bfacets is None else len(bfacets)
        if coords.shape[0] > INT32_MAX or n + nb > INT32_MAX:
            raise ValueError("a surface takes at most 2^31 - 1 vertices, and as many items and boundary facets together")
        self.device = dev = _device(source)
        self.dim, self.npi, self.npe, self.n_items, self.n_bfacets, self.n_mesh_vertices = dim, npi, npi - 1, n, nb, coords.shape[0]
        i32 = lambda a, shape: torch.as_tensor(np.ascontiguousarray(np.asarray(a).reshape(shape), dtype=np.int32), device=dev)
        self._x = torch.as_tensor(coords, device=dev)
        self._items = i32(items, (n, npi))
        side = np.zeros(n, dtype=np.uint8) if item_side is None else np.ascontiguousarray(item_side, dtype=np.uint8).reshape(n)
        if side.size and side.max() > 1:
            raise ValueError("item_side is 0 (intracellular) or 1 (extracellular)")
        self._side = torch.as_tensor(side, device=dev)
        self._ref = i32(np.zeros(n) if item_ref is None else item_ref, (n,))
        if nb:
            if bfacet_item is None or len(bfacet_item) != nb:
                raise ValueError("every boundary facet needs the index of its item")
            self._bf, self._bitem = i32(bfacets, (nb, npi - 1)), i32(bfacet_item, (nb,))
        else:
            self._bf = self._bitem = None
        self._counts = torch.empty(n + nb, dtype=torch.int32, device=dev)
        self.n_elements = self.n_vertices = None

    # ---- the plan
    def _level_function(self, s):
        s = _nodal(s)
        if not isinstance(s, torch.Tensor):
            s = torch.as_tensor(np.ascontiguousarray(s, dtype=np.float64), device=self.device)
        if s.dtype != torch.float64 or not s.is_cuda or not s.is_contiguous() or s.numel() != self.n_mesh_vertices:
            raise ValueError("the level function is a Function or a contiguous float64 device tensor with one value per vertex")
        return s

    def build(self, s, iso=0.0):
        """cut by the level ``s == iso`` of the nodal ``s``, keeping ``s >= iso``; reads back one count (the number of elements)"""
        s, iso, dev = self._level_function(s), float(iso), self.device
        n, nb, npe = self.n_items, self.n_bfacets, self.npe
        st = _stream()
        total = 0
        if n + nb:
            _call("knp_surface_count", self.npi, n, self.n_mesh_vertices, _ptr(self._items), nb, _ptr(self._bf), _ptr(self._bitem), s.data_ptr(),
                  iso, self._counts.data_ptr(), st)
            ends = torch.cumsum(self._counts, 0, dtype=torch.int64)
            total = int(ends[-1].item())                                     # the one read-back of a build
        # before anything of that size is allocated: the keys of the build (8 per element vertex), the elements, and at most one
        # output vertex per element vertex
        worst = total * (8 * npe + 9 + 4 * npe) + total * npe * (25 + 8 * self.dim)
        if total > INT32_MAX or worst > MAX_SURFACE_BYTES:
            raise ValueError(f"{FEATURE}: {total} elements may need a plan of {worst} bytes, more than the {MAX_SURFACE_BYTES} allowed "
                             "for one surface: cut fewer cells")
        keys = torch.empty(total * npe, dtype=torch.int64, device=dev)
        self.element_item = torch.empty(total, dtype=torch.int32, device=dev)
        self.element_tag = torch.empty(total, dtype=torch.int32, device=dev)
        self.element_kind = torch.empty(total, dtype=torch.uint8, device=dev)
        if total:
            offsets = ends - self._counts
            _call("knp_surface_emit", self.dim, self.npi, n, self.n_mesh_vertices, _ptr(self._items), _ptr(self._side), _ptr(self._ref), nb,
                  _ptr(self._bf), _ptr(self._bitem), s.data_ptr(), iso, self._x.data_ptr(), offsets.data_ptr(), total, keys.data_ptr(),
                  self.element_item.data_ptr(), self.element_tag.data_ptr(), self.element_kind.data_ptr(), st)
        ukeys = torch.unique(keys)                                           # sorted; the one piece that is torch's
        nout = ukeys.numel()
        self.keys = ukeys
        a, b = (torch.empty(nout, dtype=torch.int32, device=dev) for _ in range(2))
        w = torch.empty(nout, dtype=torch.float64, device=dev)
        side = torch.empty(nout, dtype=torch.uint8, device=dev)
        self.xyz = torch.empty((nout, self.dim), dtype=torch.float64, device=dev)
        self.elements = torch.empty((total, npe), dtype=torch.int32, device=dev)
        if total:
            _call("knp_surface_vertices", self.dim, self.n_mesh_vertices, nout, ukeys.data_ptr(), s.data_ptr(), iso, self._x.data_ptr(),
                  a.data_ptr(), b.data_ptr(), w.data_ptr(), side.data_ptr(), self.xyz.data_ptr(), st)
            _call("knp_surface_remap", total * npe, nout, keys.data_ptr(), ukeys.data_ptr(), self.elements.data_ptr(), st)
        self.vertices = SurfaceVertices(a, b, w, side)
        self.n_elements, self.n_vertices, self.iso, self.s = total, nout, iso, s
        return self

    @property
    def plan_bytes(self):
        """device memory of the built plan: 25 + 8 dim bytes per output vertex (key, a, b, w, side, position), 9 + 4 (npi - 1) per
        element (item, tag, kind, vertex numbers)"""
        self._built()
        return self.n_vertices * (25 + 8 * self.dim) + self.n_elements * (9 + 4 * self.npe)

    def _built(self):
        if self.n_elements is None:
            raise KnpError("the surface has not been built: call build(s, iso) first")

    # ---- the per-record kernel
    def __call__(self, functions_i, functions_e=None, out=None):
        """values[f, vertex] on the device: ``functions_i[f]`` at the output vertices of intracellular elements, ``functions_e[f]`` at
        those of extracellular ones, (1 - w) F[a] + w F[b] each; NaN where the vertex's side has no function.  Each list holds Functions
        or device tensors [n_vertices of the mesh]; one of the lists may be None.  One launch: no host copy, no synchronisation.
        ``out``: a contiguous float64 device tensor of n_fields * n_vertices entries, else a new one [n_fields, n_vertices]."""
        self._built()
        if functions_i is None and functions_e is None:
            raise ValueError("no fields to evaluate")
        nf = len(functions_i if functions_i is not None else functions_e)
        if nf > _lib.KNP_SURFACE_MAX_FIELDS:
            raise ValueError(f"at most {_lib.KNP_SURFACE_MAX_FIELDS} fields per call")
        tables = []
        for fs in (functions_i, functions_e):
            if fs is None:
                tables.append(None)
                continue
            if len(fs) != nf:
                raise ValueError("functions_i and functions_e must list the same number of fields")
            ptrs = []
            for f in fs:
                t = None if f is None else _nodal(f)
                if t is not None and (t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.numel() != self.n_mesh_vertices):
                    raise ValueError("a field is a Function or a contiguous float64 device tensor with one value per mesh vertex")
                ptrs.append(None if t is None else t.data_ptr())
            tables.append((C.c_void_p * max(nf, 1))(*ptrs))
        if out is None:
            out = torch.empty((nf, self.n_vertices), dtype=torch.float64, device=self.device)
        if not (out.is_contiguous() and out.dtype == torch.float64 and out.is_cuda and out.numel() == nf * self.n_vertices):
            raise ValueError(f"out must be a contiguous float64 device tensor of {nf} x {self.n_vertices} entries")
        v = self.vertices
        _call("knp_surface_gather", nf, self.n_vertices, _ptr(v.a), _ptr(v.b), _ptr(v.w), _ptr(v.side), tables[0], tables[1], _ptr(out), _stream())
        return out

    # ---- what the geometry measures
    def measure(self):
        """device tensor [n_elements]: area of every triangle / length of every segment (one launch, not waited for)"""
        self._built()
        m = torch.empty(self.n_elements, dtype=torch.float64, device=self.device)
        _call("knp_surface_measure", self.dim, self.npe, self.n_elements, self.n_vertices, _ptr(self.elements), _ptr(self.xyz), _ptr(m), _stream())
        return m

    def area(self):
        """total area (length of a set of segments); one launch and one read-back"""
        return float(self.measure().sum().item())

    # ---- files
    def write(self, path, fields=None):
        """One XDMF/HDF5 snapshot ``<path>.xdmf`` / ``<path>.h5`` (a trailing .xdmf is dropped): the grid ``surface`` with the cell
        attributes ``tag``, ``kind`` and ``item``; ``fields``: name -> values [n_vertices] (device or host) as node attributes."""
        self._built()
        stem = path[:-5] if str(path).endswith(".xdmf") else str(path)
        w = SurfaceWriter(stem + ".xdmf", stem + ".h5", self, extra_cell={"item": self.element_item.cpu().numpy()})
        w.write(0.0, {nm: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for nm, v in (fields or {}).items()})
        w.close()
        return stem + ".xdmf"


class SurfaceWriter:
    """``surface_<name>.xdmf`` / ``.h5``: geometry, topology and the cell attributes ``tag`` and ``kind`` are stored once; the document
    is a temporal collection of uniform grids ``step_<k>`` that refer to them and carry the record's node attributes.  After every
    record the .xdmf is a complete document; the .h5 becomes readable at ``close()``."""
    _TAIL = ['    </Grid>', '  </Domain>', '</Xdmf>', '']

    def __init__(self, xname, hname, S, extra_cell=None):
        from .hdf5_write import Hdf5Writer
        self.xname, self.h5 = xname, os.path.basename(hname)
        self.dim, self.npe, self.n_el, self.n_pts = S.dim, S.npe, S.n_elements, S.n_vertices
        self.w = Hdf5Writer(hname)
        self.w.write("/Mesh/surface/geometry", S.xyz.cpu().numpy())
        self.w.write("/Mesh/surface/topology", S.elements.cpu().numpy().astype(np.int64))
        self.cell = {"tag": S.element_tag.cpu().numpy().astype(np.int32), "kind": S.element_kind.cpu().numpy().astype(np.int32)}
        self.cell.update({k: np.asarray(v, dtype=np.int32) for k, v in (extra_cell or {}).items()})
        for nm, a in self.cell.items():
            self.w.write(f"/Mesh/surface/{nm}", a.reshape(-1, 1))
        self.records = 0
        head = "\n".join(['<?xml version="1.0"?>', '<!DOCTYPE Xdmf SYSTEM "Xdmf.dtd" []>', '<Xdmf Version="3.0">', '  <Domain>',
                          '    <Grid Name="surface" GridType="Collection" CollectionType="Temporal">', ''])
        with open(self.xname, "w") as f:
            f.write(head)
            self.pos = f.tell()
            f.write("\n".join(self._TAIL))

    def _item(self, rows, cols, kind, prec, where):
        return f'          <DataItem Dimensions="{rows} {cols}" NumberType="{kind}" Precision="{prec}" Format="HDF">{self.h5}:{where}</DataItem>'

    def write(self, t, data):
        """one record at time ``t``: name -> host values [n_vertices]"""
        k = self.records
        body = [f'      <Grid Name="step_{k}" GridType="Uniform">', f'        <Time Value="{float(t)!r}" />',
                f'        <Topology TopologyType="{"Triangle" if self.npe == 3 else "Polyline"}" NumberOfElements="{self.n_el}" NodesPerElement="{self.npe}">',
                self._item(self.n_el, self.npe, "Int", 8, "/Mesh/surface/topology"), '        </Topology>',
                f'        <Geometry GeometryType="{"XY" if self.dim == 2 else "XYZ"}">',
                self._item(self.n_pts, self.dim, "Float", 8, "/Mesh/surface/geometry"), '        </Geometry>']
        for nm in self.cell:
            body += [f'        <Attribute Name="{nm}" AttributeType="Scalar" Center="Cell">',
                     self._item(self.n_el, 1, "Int", 4, f"/Mesh/surface/{nm}"), '        </Attribute>']
        for nm, a in data.items():
            self.w.write(f"/Function/{nm}/{k}", np.asarray(a, dtype=np.float64).reshape(self.n_pts, 1))
            body += [f'        <Attribute Name="{nm}" AttributeType="Scalar" Center="Node">',
                     self._item(self.n_pts, 1, "Float", 8, f"/Function/{nm}/{k}"), '        </Attribute>']
        body += ['      </Grid>']
        with open(self.xname, "r+") as f:
            f.seek(self.pos)
            f.write("\n".join(body) + "\n")
            self.pos = f.tell()
            f.write("\n".join(self._TAIL))
            f.truncate()
        self.records += 1

    def close(self):
        if self.w is not None:
            self.w.close()
            self.w = None


class ClipSurface(LevelSetSurface):
    """The boundary of {cells tagged ``tags``} intersected with the half-space n . (x - origin) >= 0, cut open along the plane: what
    the reference's ``threshold`` + ``clip`` draws.  ``tags``: cell tags (default: every intracellular tag), or ``side`` 0 / 1 for all
    tags of a side; ``origin`` / ``normal`` in metres (the problem's coordinates).  ``boundary=True`` adds the clipped boundary of the
    kept set -- the facets with exactly one kept neighbour, found once per tag set by NumPy from ``mesh.build_facets`` --,
    ``boundary=False`` gives the exact slice alone.  ``item_cell`` maps ``element_item`` to the mesh's cells.  Built on construction
    (one read-back); ``move(origin, normal)`` cuts again."""

    def __init__(self, problem, tags=None, side=None, origin=None, normal=None, boundary=True):
        _one_rank(problem)
        lm = problem.local_mesh
        dim = lm.coords.shape[1]
        if tags is not None and side is not None:
            raise ValueError("give tags or side, not both")
        if side is not None and side not in (0, 1):
            raise ValueError("side must be 0 (intracellular) or 1 (extracellular)")
        if tags is None:
            tags = problem.extra_tag if side == 1 else problem.intra_tags
        tags = tuple(int(t) for t in (tags if isinstance(tags, (list, tuple, np.ndarray, range)) else [tags]))
        known = {int(t) for t in problem.intra_tags} | {int(t) for t in problem.extra_tag}
        if not tags or len(set(tags)) != len(tags) or set(tags) - known:
            raise ValueError(f"tags {list(tags)}: listed once each, out of the problem's cell tags {sorted(known)}")
        nco = int(lm.n_cells_owned)
        cells, ctags = np.asarray(lm.cells)[:nco], np.asarray(lm.cell_tags)[:nco]
        kept = np.isin(ctags, tags)
        self.tags, self.boundary, self.problem = tags, bool(boundary), problem
        self.item_cell = np.nonzero(kept)[0]
        bf = bitem = None
        if boundary:
            cache = problem.__dict__.setdefault("_surface_boundaries", {})       # once per tag set
            if tags not in cache:
                facets = cache.get("facets") or cache.setdefault("facets", _build_facets(cells))
                fv, cell = kept_boundary(lm.coords, cells, kept, facets)
                to_item = np.full(nco, -1, dtype=np.int64)
                to_item[self.item_cell] = np.arange(len(self.item_cell))
                cache[tags] = (fv, to_item[cell])
            bf, bitem = cache[tags]
        super().__init__(problem, cells[kept], np.asarray(problem.cell_side)[:nco][kept], ctags[kept], bf, bitem)
        self._s = torch.empty(self.n_mesh_vertices, dtype=torch.float64, device=self.device)
        self.move(np.zeros(dim) if origin is None else origin, normal)

    def move(self, origin, normal):
        """cut with another plane (one launch for s = n . (x - origin) on the device, then a build: one read-back)"""
        dim = self.dim
        o = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).ravel()[:dim])
        if normal is None:
            raise ValueError("a clip needs the plane's normal")
        nrm = np.ascontiguousarray(np.asarray(normal, dtype=np.float64).ravel()[:dim])
        if o.shape[0] != dim or nrm.shape[0] != dim or not np.all(np.isfinite(o)) or not np.all(np.isfinite(nrm)) or not np.abs(nrm).sum() > 0:
            raise ValueError(f"origin and normal need {dim} finite components and the normal must not be the zero vector")
        self.origin, self.normal = o, nrm
        _call("knp_surface_plane", dim, self.n_mesh_vertices, self._x.data_ptr(), o.ctypes.data_as(_lib.f64p), nrm.ctypes.data_as(_lib.f64p),
              self._s.data_ptr(), _stream())
        return self.build(self._s, 0.0)

    @property
    def element_cell(self):
        """mesh cell of every element (device tensor, int64)"""
        return torch.as_tensor(self.item_cell, device=self.device)[self.element_item.long()]


def _build_facets(cells):
    from . import mesh as meshmod
    return meshmod.build_facets(np.asarray(cells))


class IsoSurface(LevelSetSurface):
    """The iso-surface ``function == iso`` through the cells tagged ``tags``, exact on the mesh (cut faces only; its normals point
    toward decreasing values).  ``function_i`` cuts intracellular cells, ``function_e`` extracellular ones; ``tags`` defaults to every
    tag of the side whose function is given and must lie on one side -- a level through both sides is two surfaces, because a
    membrane vertex has a value per side.  ``update(iso=None)`` rebuilds from the function's current values: one read-back, like the
    construction."""

    def __init__(self, problem, function_i=None, function_e=None, iso=0.0, tags=None):
        _one_rank(problem)
        if function_i is None and function_e is None:
            raise ValueError("an iso-surface needs a function")
        lm = problem.local_mesh
        intra, extra = tuple(int(t) for t in problem.intra_tags), tuple(int(t) for t in problem.extra_tag)
        if tags is None:
            if function_i is not None and function_e is not None:
                raise ValueError("two functions were given: name the tags (of one side) whose cells are cut")
            tags = intra if function_i is not None else extra
        tags = tuple(int(t) for t in (tags if isinstance(tags, (list, tuple, np.ndarray, range)) else [tags]))
        sides = {0 if t in intra else 1 if t in extra else -1 for t in tags}
        if not tags or len(sides) != 1 or -1 in sides:
            raise ValueError(f"tags {list(tags)} must be cell tags of one side (intracellular {list(intra)}, extracellular {list(extra)})")
        side = sides.pop()
        self.function = function_i if side == 0 else function_e
        if self.function is None:
            raise ValueError("the tags lie on the side whose function was not given")
        nco = int(lm.n_cells_owned)
        cells, ctags = np.asarray(lm.cells)[:nco], np.asarray(lm.cell_tags)[:nco]
        kept = np.isin(ctags, tags)
        self.tags, self.problem, self.item_cell = tags, problem, np.nonzero(kept)[0]
        super().__init__(problem, cells[kept], np.full(int(kept.sum()), side, dtype=np.uint8), ctags[kept])
        self.update(iso)

    def update(self, iso=None):
        """rebuild from the function's current values (and another level): one read-back"""
        return self.build(self.function, self.iso if iso is None else iso)


# ------------------------------------------------------------------------------------------------ recording during a run
def parse_clip_surfaces(out_cfg, problem, save_interval, n_steps, known_fields):
    """``clip_surfaces`` / ``surface_interval`` of ``solver.output``: (entries, interval).  Each entry: ``name``, ``tags`` or ``side``,
    ``origin`` and ``normal`` (the config gives mesh units, like sample_grids; the entries hold metres), ``boundary`` (default true),
    ``fields`` (default: all of ``known_fields``).  Absent or empty: ([], interval) and nothing is allocated or launched."""
    surfs = out_cfg.get("clip_surfaces") or []
    interval = int(out_cfg.get("surface_interval", save_interval))
    if interval < 1:
        raise ValueError("surface_interval must be at least 1")
    if not isinstance(surfs, (list, tuple)):
        raise ValueError("clip_surfaces must be a list of entries")
    dim, factor = problem.local_mesh.coords.shape[1], float(problem.mesh_conversion_factor)
    entries, seen = [], set()
    for k, g in enumerate(surfs):
        what = f"clip_surfaces[{k}]"
        if not isinstance(g, dict) or "name" not in g:
            raise ValueError(f"{what}: an entry is a mapping with a name, origin and normal")
        name = str(g["name"])
        what += f" ('{name}')"
        if name in seen:
            raise ValueError(f"{what}: the name is used twice")
        seen.add(name)
        unknown = set(g) - {"name", "tags", "side", "origin", "normal", "boundary", "fields"}
        if unknown:
            raise ValueError(f"{what}: unknown key(s) {sorted(unknown)}")
        for key in ("origin", "normal"):
            if key not in g:
                raise ValueError(f"{what}: missing key '{key}'")
        try:
            origin = np.asarray(g["origin"], dtype=np.float64).ravel()
            normal = np.asarray(g["normal"], dtype=np.float64).ravel()
        except (TypeError, ValueError) as e:
            raise ValueError(f"{what}: origin and normal must be numbers ({e})") from None
        if origin.shape[0] < dim or normal.shape[0] < dim or not np.abs(normal[:dim]).sum() > 0:
            raise ValueError(f"{what}: origin and normal need {dim} components and the normal must not be the zero vector")
        if "tags" in g and "side" in g:
            raise ValueError(f"{what}: give tags or side, not both")
        fields = list(g.get("fields", known_fields))
        bad = [f for f in fields if f not in known_fields]
        if bad or not fields or len(set(fields)) != len(fields):
            raise ValueError(f"{what}: unknown, repeated or no field name(s) {bad or fields}: choose from {list(known_fields)}")
        entries.append({"name": name, "tags": g.get("tags"), "side": g.get("side"), "origin": origin[:dim] * factor, "normal": normal[:dim],
                        "boundary": bool(g.get("boundary", True)), "fields": fields})
    return entries, interval


def named_functions(problem, fields=None):
    """(names, functions_i, functions_e) a surface records: ``fields`` None or a list of names -- the merged ``Na, K, Cl, phi`` of a
    KNP-EMI problem, ``phi`` of an EMI problem -- or a mapping name -> (function_i, function_e)"""
    if isinstance(fields, dict):
        names = [str(k) for k in fields]
        pairs = [tuple(v) if isinstance(v, (list, tuple)) else (v, None) for v in fields.values()]
        if not names or any(len(p) != 2 or (p[0] is None and p[1] is None) for p in pairs):
            raise ValueError("fields maps a name to a pair (function_i, function_e), one of which may be None")
        return names, [p[0] for p in pairs], [p[1] for p in pairs]
    if hasattr(problem, "ion_list"):
        from .sampling import merged_functions
        return merged_functions(problem, fields)
    names = ["phi"] if fields is None else list(fields)
    if names != ["phi"]:
        raise ValueError(f"unknown field name(s) {names}: an EMI problem has 'phi' (or give a mapping name -> (function_i, function_e))")
    return names, [problem.wh[0]], [problem.wh[1]]


class SurfaceRecorder:
    """What ``add_surface`` / ``clip_surfaces`` keep per surface: a preallocated device tensor [records, fields, vertices]; a record is
    one gather launch into its row, ``save()`` reads the tensor back once and writes surface_<name>.xdmf / .h5."""

    def __init__(self, name, S, names, f_i, f_e, interval, n_steps, out_dir):
        S._built()
        self.name, self.S, self.names, self.f_i, self.f_e, self.interval = name, S, list(names), f_i, f_e, int(interval)
        self.out_dir, self.t, self.saved = out_dir, [], False
        n_rec = n_steps // self.interval + 1
        nbytes = 8 * n_rec * len(self.names) * S.n_vertices
        if nbytes > MAX_SURFACE_BYTES:
            raise ValueError(f"surface '{name}': {n_rec} records of {len(self.names)} fields on {S.n_vertices} vertices take {nbytes} bytes, "
                             f"more than the {MAX_SURFACE_BYTES} allowed for one surface: raise the interval (now {self.interval})")
        self.buf = torch.zeros((n_rec, len(self.names), S.n_vertices), dtype=torch.float64, device=S.device)

    def record(self, i, t):
        """state after timestep ``i`` at time ``t``, if a record is due"""
        if i % self.interval or i // self.interval >= self.buf.shape[0]:
            return
        self.S(self.f_i, self.f_e, out=self.buf[i // self.interval])
        self.t.append(float(t))

    def save(self):
        if self.saved:
            return
        self.saved = True
        os.makedirs(self.out_dir, exist_ok=True)
        stem = os.path.join(self.out_dir, "surface_" + self.name)
        w = SurfaceWriter(stem + ".xdmf", stem + ".h5", self.S)
        vals = self.buf[:len(self.t)].cpu().numpy()
        for k, t in enumerate(self.t):
            w.write(t, {nm: vals[k, j] for j, nm in enumerate(self.names)})
        w.close()


def check_add_surface(solver, name, S, fields, interval, existing):
    """the checks ``add_surface`` shares between the solvers; returns (name, S, fields, interval)"""
    name = str(name)
    if not name or any(name == e[0] for e in existing) or os.sep in name:
        raise ValueError(f"a surface needs a name of its own (got '{name}')")
    if not isinstance(S, LevelSetSurface) or S.n_elements is None:
        raise ValueError("add_surface() takes a built LevelSetSurface (ClipSurface, IsoSurface)")
    if getattr(S, "problem", solver.problem) is not solver.problem:
        raise ValueError("add_surface() takes a surface of this solver's problem")
    interval = int(solver.save_interval if interval is None else interval)
    if interval < 1:
        raise ValueError("interval must be at least 1")
    named_functions(solver.problem, fields)
    return name, S, fields, interval
