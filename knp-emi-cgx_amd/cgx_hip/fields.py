"""Fields of user expressions on the device: one value per cell (``CellField``) or per membrane facet (``FacetField``), and their
measure-weighted averages onto the vertices (csrc/knp_fields.inc; ``knp_functional_eval_items``,
``knp_membrane_functional_eval_items`` and ``knp_project_*`` of include/knpemi_hip.h).  What the reference gets by projecting or
interpolating a UFL expression: the current density ``-sigma * grad(phi)``, an ion flux, a charge density, the channel current of an
ion on every membrane facet.

A field takes the expressions of a functional (cgx_hip/functionals.py: ``compile_functional`` / ``compile_membrane_functional``, with
their side rules, tag rules and refusals) and evaluates them with the functional's own kernel; instead of the integral per tag it
keeps the mean of every item, ``sum_q q_w[q] f(x_q)``.  The measures are attributes (``volume`` / ``area``), so an integral is one
multiply away.  A gradient of a P1 function is constant on a cell and no nodal Function; ``to_nodes`` averages the item values onto
the vertices, every item weighted with its measure, which gives Functions that the samplers, the checkpoints and the XDMF writer take.

``FieldsWriter`` is the ``fields.xdmf`` / ``fields.h5`` pair of ``SolverKNPEMI.add_field``; it takes host arrays and needs no device.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib, fem
from .diagnostics import cell_volumes
from .functionals import _Functional, compile_functional, compile_membrane_functional, field_roles, membrane_field_roles

CELL_FEATURE = "cell fields (CellField / cell_field / add_field)"
FACET_FEATURE = "facet fields (FacetField / facet_field / add_field)"
PROJECT_INFO = ("lanes", "longest", "n_split", "n_units", "split")      # the slots of knp_project_get_info, in its order


class Projection:
    """A plan of ``knp_project_create``: item values [n_items, n_out] on the device -> their measure-weighted vertex averages
    [n_out, n_vertices].  ``info()`` names what an application runs (``PROJECT_INFO``)."""

    def __init__(self, backend, item_vertices, measure):
        self.backend = backend
        iv = np.ascontiguousarray(item_vertices, dtype=np.int32)
        ms = np.ascontiguousarray(measure, dtype=np.float64)
        self.n_items, self.nv = iv.shape
        if ms.shape != (self.n_items,):
            raise ValueError("one measure per item")
        pid = C.c_int32(-1)
        backend.check(backend.lib.knp_project_create(backend.ctx, self.n_items, self.nv, iv.ctypes.data_as(_lib.i32p) if iv.size else None,
                                                     ms.ctypes.data_as(_lib.f64p) if ms.size else None, C.byref(pid)))
        self.id = int(pid.value)

    def info(self):
        be = self.backend
        v = np.zeros(len(PROJECT_INFO), dtype=np.int32)
        be.check(be.lib.knp_project_get_info(be.ctx, self.id, v.ctypes.data_as(_lib.i32p), len(v)))
        return dict(zip(PROJECT_INFO, (int(x) for x in v)))

    def __call__(self, values, n_out, n_vertices, fill=float("nan"), out=None):
        """``values``: a contiguous float64 device tensor of n_items * n_out entries.  Enqueued: no host copy, no synchronisation."""
        be = self.backend
        if self.id < 0:
            raise _lib.KnpError("the projection is closed")
        if not (values.is_contiguous() and values.dtype == torch.float64 and values.is_cuda and values.numel() == self.n_items * n_out):
            raise ValueError(f"values must be a contiguous float64 device tensor of {self.n_items} x {n_out} entries")
        if out is None:
            out = torch.empty((n_out, n_vertices), dtype=torch.float64, device=be.device)
        be.check(be.lib.knp_project_apply(be.ctx, self.id, C.c_void_p(values.data_ptr()) if self.n_items else None, n_out, float(fill),
                                          C.c_void_p(out.data_ptr())))
        return out

    def close(self):
        be, pid = self.backend, self.id
        self.id = -1
        if pid >= 0 and getattr(be, "ctx", None):
            be.lib.knp_project_destroy(be.ctx, pid)

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass


class _Field(_Functional):
    """What the two kinds of field share on top of ``_Functional``: every plan has one row that lists all its items, ascending, and a
    call returns the items' means instead of the rows' integrals."""

    def _plan(self, prog, items, q_pts, q_w):
        items = np.ascontiguousarray(items, dtype=np.int32)
        self._first.append(sum(self._count))
        self._count.append(len(items))
        self._create(prog, 1, np.array([0, len(items)], dtype=np.int32), items, q_pts, q_w)

    def _open(self, problem):
        super()._open(problem)
        self._first, self._count, self._proj = [], [], None

    @property
    def n_items(self):
        return sum(self._count)

    def __call__(self, out=None):
        """The means per listed item, [n_items, n_out] on the device; the constants and the tensors' addresses are read anew.
        Enqueued: no host copy, no synchronisation.  ``out``: a contiguous float64 device tensor of that size, else a new one."""
        be = self.backend
        if self.n_plans and not self.plans:
            raise _lib.KnpError("the field is closed")
        shape = (self.n_items, self.n_out)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=be.device)
        if not (out.is_contiguous() and out.dtype == torch.float64 and out.is_cuda and out.numel() == shape[0] * shape[1]):
            raise ValueError(f"out must be a contiguous float64 device tensor of {shape[0]} x {shape[1]} entries")
        for plan, first, count in zip(self.plans, self._first, self._count):
            if not count:
                continue
            f = self._fields(plan.spec)
            consts = plan.spec.constants()
            if consts.size:
                be.check(getattr(be.lib, self.ABI + "_set_constants")(be.ctx, plan.id, consts.shape[0], consts.ctypes.data_as(_lib.f64p)))
            be.check(getattr(be.lib, self.ABI + "_eval_items")(be.ctx, plan.id, C.byref(f), C.c_void_p(out.data_ptr() + 8 * first * self.n_out)))
        return out.view(shape)

    def value(self):
        """the means per listed item as NumPy [n_items, n_out] (one read-back)"""
        return self().cpu().numpy()

    def close(self):
        for pr in (getattr(self, "_proj", None) or []):
            if pr is not None:
                pr.close()
        self._proj = None
        super().close()

    def _named(self, tensors, suffix):
        """one ``fem.Function`` per output of a projection [n_out, n_vertices]"""
        fns = []
        for j in range(self.n_out):
            fn = fem.Function(self.problem.V, f"{self.name}{suffix}" + (f"_{j}" if self.n_out > 1 else ""))
            fn.x.array.copy_(tensors[j])
            fns.append(fn)
        return fns


class CellField(_Field):
    """Per owned cell of the chosen tags, the mean of ``expr_i`` (intracellular cells) or ``expr_e`` (extracellular cells) under a
    rule exact to polynomial ``degree``: expressions, sides, ``tags`` and refusals are ``VolumeFunctional``'s.  One plan per side, the
    side's cells ascending.  ``cells`` / ``cell_tag`` / ``side`` / ``volume``: per row of the result, the intracellular cells first.
    A call returns the device tensor [n_listed, n_out]."""
    ABI, ITEMS = "knp_functional", "cells"
    FEATURE = CELL_FEATURE
    roles = staticmethod(field_roles)

    def __init__(self, problem, expr_i=None, expr_e=None, tags=None, degree=1, name="field"):
        spec = self.spec = compile_functional(problem, expr_i, expr_e, tags, degree)
        self.n_out, self.degree, self.tags, self.name = spec.n_out, spec.degree, spec.tags, str(name)
        lm = problem.local_mesh
        nco = int(lm.n_cells_owned)
        self.n_cells = nco
        self._open(problem)
        per_side = []
        for sp in spec.sides:
            cells = np.sort(np.asarray(sp.cells, dtype=np.int64))
            per_side.append((sp.side, cells))
            self._plan(sp.spec, cells, spec.q_bary, spec.q_w)
        self._sides = [s for s, _ in per_side]
        self.cells = np.concatenate([c for _, c in per_side]) if per_side else np.zeros(0, dtype=np.int64)
        self.side = np.concatenate([np.full(len(c), s, dtype=np.int64) for s, c in per_side]) if per_side else np.zeros(0, dtype=np.int64)
        self.cell_tag = np.asarray(lm.cell_tags[:nco], dtype=np.int64)[self.cells]
        self.volume = cell_volumes(lm.coords, lm.cells[:nco][self.cells])
        self._cells_dev = torch.as_tensor(self.cells, dtype=torch.int64, device=self.backend.device)

    def full(self, fill=float("nan"), values=None):
        """[n_cells_owned, n_out] in mesh cell order (``fill`` on the cells that are not listed), so that ``F.full()[sampler.cell]``
        is the field at a sampler's points; ``values``: the result of an earlier call, else the field is evaluated"""
        values = self() if values is None else values
        out = torch.full((self.n_cells, self.n_out), float(fill), dtype=torch.float64, device=self.backend.device)
        out.index_copy_(0, self._cells_dev, values)
        return out

    def to_nodes(self, fill=float("nan"), values=None):
        """(intracellular, extracellular) projections, each [n_out, n_vertices] on the device: per vertex the volume-weighted average
        of the listed cells of that side around it, ``fill`` where there is none.  A membrane vertex has a value on both."""
        lm = self.problem.local_mesh
        values = self() if values is None else values
        if self._proj is None:
            cells = np.asarray(lm.cells)
            self._proj = [Projection(self.backend, cells[self.cells[a:a + n]], self.volume[a:a + n]) for a, n in zip(self._first, self._count)]
        out = [torch.full((self.n_out, self.n_vertices), float(fill), dtype=torch.float64, device=self.backend.device) for _ in range(2)]
        for s, pr, a, n in zip(self._sides, self._proj, self._first, self._count):
            pr(values[a:a + n], self.n_out, self.n_vertices, fill, out=out[s])
        return out[0], out[1]

    def functions(self, fill=float("nan")):
        """the projections as ``fem.Function``s, (intracellular list, extracellular list) with one Function per output: what
        ``FieldSampler(...)(functions_i, functions_e)`` takes"""
        ti, te = self.to_nodes(fill)
        return self._named(ti, "_i"), self._named(te, "_e")


class FacetField(_Field):
    """Per membrane facet of the chosen tags, the mean of ``expr`` under a facet rule exact to polynomial ``degree``: expressions
    (restrictions, ``fem.FacetNormal``, ``fem.NormalDerivative``), ``tags`` and refusals are ``MembraneFunctional``'s.  One plan, the
    facets ascending.  ``facets`` (indices into the problem's gamma list) / ``facet_tag`` / ``area`` / ``vertices`` [n, dim]: per row
    of the result.  A call returns the device tensor [n_listed, n_out]."""
    ABI, ITEMS = "knp_membrane_functional", "facets"
    FEATURE = FACET_FEATURE
    roles = staticmethod(membrane_field_roles)

    def __init__(self, problem, expr, tags=None, degree=1, name="field"):
        spec = self.spec = compile_membrane_functional(problem, expr, tags, degree)
        self.n_out, self.degree, self.tags, self.groups, self.name = spec.n_out, spec.degree, spec.tags, spec.groups, str(name)
        self._open(problem)
        self.facets = np.sort(np.asarray(spec.facets, dtype=np.int64))
        self._plan(spec.spec, self.facets, spec.q_pts, spec.q_w)
        self.facet_tag = np.asarray(problem.gamma_facet_tags, dtype=np.int64)[self.facets]
        self.area = np.asarray(problem._fmeas, dtype=np.float64)[self.facets]
        self.vertices = np.asarray(problem._fv, dtype=np.int64)[self.facets].reshape(len(self.facets), -1)

    def to_nodes(self, fill=float("nan"), values=None):
        """[n_out, n_vertices] on the device: per vertex the area-weighted average of the listed facets around it, ``fill`` away from
        the listed membranes"""
        values = self() if values is None else values
        if self._proj is None:
            self._proj = [Projection(self.backend, self.vertices, self.area)]
        return self._proj[0](values, self.n_out, self.n_vertices, fill)

    def functions(self, fill=float("nan")):
        """the projection as ``fem.Function``s, one per output"""
        return self._named(self.to_nodes(fill), "")


# ------------------------------------------------------------------------------------------ fields.xdmf / fields.h5
class FieldsWriter:
    """``fields.xdmf`` / ``fields.h5`` of ``SolverKNPEMI.add_field``, from host arrays.  The document is a temporal collection; every
    record is a spatial collection of the grid ``mesh`` (the cells, with the cell fields as ``Center="Cell"`` attributes and the nodal
    ones as ``Center="Node"``) and, where facet fields are due, one grid per facet list over the same geometry (``membrane``, then
    ``membrane_2``, ...: ``Polyline`` with 2 nodes in 2D, ``Triangle`` in 3D).  A field of ``dim`` outputs is one ``Vector`` attribute,
    padded to 3 components in 2D; one output is a ``Scalar``; any other count is written as scalars ``<name>_<j>``.  After every record the
    .xdmf is a complete document: the new text goes where the closing tags began, followed by the closing tags again.

    ``entries``: dicts with ``name``, ``kind`` ('cell' | 'node' | 'facet' | 'facet_node'), ``n_out`` and, for a facet field,
    ``vertices`` [n, dim]."""
    _TAIL = ['    </Grid>', '  </Domain>', '</Xdmf>', '']

    def __init__(self, xname, hname, coords, cells, entries):
        from .hdf5_write import Hdf5Writer
        coords = np.asarray(coords, dtype=np.float64)
        cells = np.asarray(cells, dtype=np.int64)
        self.dim, self.n_pts, self.n_cells = coords.shape[1], len(coords), len(cells)
        self.xname, self.h5 = xname, os.path.basename(hname)
        self.w = Hdf5Writer(hname)
        self.w.write("/Mesh/mesh/geometry", coords)
        self.w.write("/Mesh/mesh/topology", cells)
        self.entries, self.count, self.grids = {}, {}, []
        for e in entries:
            e = dict(e)
            if e["name"] in self.entries or not 1 <= int(e["n_out"]) <= 3 or e["kind"] not in ("cell", "node", "facet", "facet_node"):
                raise ValueError(f"field '{e['name']}': a name of its own, 1..3 outputs and a known kind")
            if e["kind"] == "facet":
                fv = np.asarray(e["vertices"], dtype=np.int64).reshape(-1, self.dim)
                for g in self.grids:
                    if g["fv"].shape == fv.shape and np.array_equal(g["fv"], fv):
                        break
                else:
                    g = {"name": "membrane" if not self.grids else f"membrane_{len(self.grids) + 1}", "fv": fv}
                    self.w.write(f"/Mesh/{g['name']}/topology", fv)
                    self.grids.append(g)
                e["grid"] = g["name"]
            self.entries[e["name"]] = e
            self.count[e["name"]] = 0
        self.records = 0
        head = "\n".join(['<?xml version="1.0"?>', '<!DOCTYPE Xdmf SYSTEM "Xdmf.dtd" []>', '<Xdmf Version="3.0">', '  <Domain>',
                          '    <Grid Name="fields" GridType="Collection" CollectionType="Temporal">', ''])
        with open(self.xname, "w") as f:
            f.write(head)
            self.pos = f.tell()
            f.write("\n".join(self._TAIL))

    def _geometry(self):
        return [f'          <Geometry GeometryType="{"XY" if self.dim == 2 else "XYZ"}">',
                f'            <DataItem Dimensions="{self.n_pts} {self.dim}" NumberType="Float" Precision="8" Format="HDF">{self.h5}:/Mesh/mesh/geometry</DataItem>',
                f'          </Geometry>']

    def _topology(self, grid, ttype, n, nodes):
        return [f'          <Topology TopologyType="{ttype}" NumberOfElements="{n}" NodesPerElement="{nodes}">',
                f'            <DataItem Dimensions="{n} {nodes}" NumberType="Int" Precision="8" Format="HDF">{self.h5}:/Mesh/{grid}/topology</DataItem>',
                f'          </Topology>']

    def _attributes(self, name, arr, n_rows, center, suffix=""):
        """writes the datasets of one field's record and returns its Attribute lines; ``arr`` [n_rows, n_out]"""
        arr = np.asarray(arr, dtype=np.float64).reshape(n_rows, -1)
        k, n_out = self.count[name], arr.shape[1]
        label = name + suffix
        if n_out == self.dim:
            cols = [(label, "Vector", np.concatenate([arr, np.zeros((n_rows, 3 - n_out))], axis=1))]
        elif n_out == 1:
            cols = [(label, "Scalar", arr)]
        else:
            cols = [(f"{label}_{j}", "Scalar", arr[:, j:j + 1]) for j in range(n_out)]
        lines = []
        for nm, atype, a in cols:
            self.w.write(f"/Field/{nm}/{k}", np.ascontiguousarray(a))
            lines += [f'          <Attribute Name="{nm}" AttributeType="{atype}" Center="{center}">',
                      f'            <DataItem Dimensions="{n_rows} {a.shape[1]}" NumberType="Float" Precision="8" Format="HDF">{self.h5}:/Field/{nm}/{k}</DataItem>',
                      f'          </Attribute>']
        return lines

    def write(self, t, data):
        """one record at time ``t``.  ``data``: name -> array; a 'cell' field [n_cells, n_out], a 'node' field the pair of
        [n_out, n_vertices] projections (written as ``<name>_i`` / ``<name>_e``), a 'facet' field [n_facets, n_out], a 'facet_node'
        field [n_out, n_vertices]"""
        if not data:
            return
        mesh, facet = [], {}
        for name, arr in data.items():
            e = self.entries[name]
            if e["kind"] == "cell":
                mesh += self._attributes(name, arr, self.n_cells, "Cell")
            elif e["kind"] == "node":
                for sfx, a in zip(("_i", "_e"), arr):
                    mesh += self._attributes(name, np.asarray(a).T, self.n_pts, "Node", sfx)
            elif e["kind"] == "facet_node":
                mesh += self._attributes(name, np.asarray(arr).T, self.n_pts, "Node")
            else:
                facet.setdefault(e["grid"], []).extend(self._attributes(name, arr, len(arr), "Cell"))
            self.count[name] += 1
        body = [f'      <Grid Name="step_{self.records}" GridType="Collection" CollectionType="Spatial">', f'        <Time Value="{float(t)!r}" />',
                '        <Grid Name="mesh" GridType="Uniform">']
        body += self._topology("mesh", "Triangle" if self.dim == 2 else "Tetrahedron", self.n_cells, self.dim + 1) + self._geometry() + mesh
        body += ['        </Grid>']
        for g in self.grids:
            if g["name"] in facet:
                body += [f'        <Grid Name="{g["name"]}" GridType="Uniform">']
                body += self._topology(g["name"], "Polyline" if self.dim == 2 else "Triangle", len(g["fv"]), self.dim) + self._geometry()
                body += facet[g["name"]] + ['        </Grid>']
        body += ['      </Grid>']
        with open(self.xname, "r+") as f:
            f.seek(self.pos)
            f.write("\n".join(body) + "\n")
            self.pos = f.tell()
            f.write("\n".join(self._TAIL))
            f.truncate()
        self.records += 1

    def close(self):
        """fields.h5 becomes readable here (its metadata and superblock are written at close)"""
        if self.w is not None:
            self.w.close()
            self.w = None


def writer_entry(name, F, nodal):
    """the ``FieldsWriter`` entry of an ``add_field`` call"""
    if isinstance(F, FacetField):
        return {"name": name, "kind": "facet_node" if nodal else "facet", "n_out": F.n_out, "vertices": F.vertices}
    return {"name": name, "kind": "node" if nodal else "cell", "n_out": F.n_out}


def record_arrays(F, nodal):
    """what ``FieldsWriter.write`` takes for the field ``F`` now, as host arrays (one evaluation, one read-back)"""
    if isinstance(F, FacetField):
        return (F.to_nodes() if nodal else F()).cpu().numpy()
    if nodal:
        return tuple(t.cpu().numpy() for t in F.to_nodes())
    return F.full().cpu().numpy()
