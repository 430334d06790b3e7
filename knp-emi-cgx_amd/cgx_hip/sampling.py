"""Sampling of the solution at arbitrary points -- grids, slices, probe lines -- with the point location and the interpolation on the
device (csrc/knp_sample.inc, ``knp_sample_*`` of include/knpemi_hip.h).

Replaces, for runs of this project, the slices the reference cuts out of its ADIOS2 checkpoints with pyvista (utils/plot_slices.py,
plot_slice_membrane.py, plot_slices_geometries.py): a ``GridSampler`` is the slice, the arrays it returns are what those scripts plot
(the merged fields and, as ``cell_tag``, their "Domain ID" layer).

A sampler locates its points once (``FieldSampler.__init__``: NumPy sorts the points into bins, two kernels find cell and weights per
point) and then evaluates any number of nodal fields per call with one gather kernel, into a device tensor, without a host copy or
a synchronisation.  The rule of location is that of ``output._barycentric``: a cell contains a point when all its barycentric weights
are >= -1e-9, the lowest cell index among the containing cells wins, the weights are clipped to [0, 1] and renormalised.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

FEATURE = "field sampling on grids and slices (FieldSampler / GridSampler / sample_grids)"
MERGED_FIELDS = ("Na", "K", "Cl", "phi")      # the _i function inside intracellular cells, the _e function inside extracellular ones
MAX_GRID_BYTES = 2 ** 30                      # largest record buffer of one sample_grids entry


def bin_points(pts, per_bin=2.0):
    """Sort the points [n, dim] into a uniform lattice of bins over their bounding box, about ``per_bin`` points per bin on average:
    ``origin`` [dim], ``size`` [dim], ``shape`` [dim], ``bin_ptr`` [n_bins + 1] and ``bin_pts`` [n] (the points of bin b are
    ``bin_pts[bin_ptr[b]:bin_ptr[b + 1]]``; bins row-major).  The bin of a point along axis k is
    ``clip(floor((p_k - origin_k) / size_k), 0, shape_k - 1)``, the formula knp_sample_plan_create verifies.  An axis along which all
    points coincide (a slice normal to it) gets one bin of the smallest width the origin's magnitude allows."""
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    n, dim = pts.shape
    origin = pts.min(axis=0)
    ext = pts.max(axis=0) - origin
    wide = ext > 0
    shape = np.ones(dim, dtype=np.int64)
    if wide.any():
        m = int(wide.sum())
        h = (float(np.prod(ext[wide])) / max(n / per_bin, 1.0)) ** (1.0 / m)
        while True:
            shape[wide] = np.maximum(np.ceil(ext[wide] / h), 1).astype(np.int64)
            if int(np.prod(shape)) <= 4 * n + 64:
                break
            h *= 1.26
    tiny = np.finfo(np.float64).tiny
    size = np.where(wide, np.maximum(ext / shape, tiny), np.maximum(np.spacing(np.abs(origin)), tiny))
    idx = np.clip(np.floor((pts - origin) / size), 0, shape - 1).astype(np.int64)
    lin = np.ravel_multi_index(tuple(idx.T), tuple(int(s) for s in shape))
    order = np.argsort(lin, kind="stable")
    n_bins = int(np.prod(shape))
    bin_ptr = np.zeros(n_bins + 1, dtype=np.int64)
    np.cumsum(np.bincount(lin, minlength=n_bins), out=bin_ptr[1:])
    return {"origin": origin, "size": size, "shape": shape.astype(np.int32), "bin_ptr": bin_ptr.astype(np.int32),
            "bin_pts": order.astype(np.int32)}


def grid_points(origin, axes, shape):
    """The lattice ``origin + sum_k t_k axes[k]``, ``t_k = linspace(0, 1, shape[k])`` (end points included): [*shape, dim]"""
    origin = np.asarray(origin, dtype=np.float64)
    axes = np.atleast_2d(np.asarray(axes, dtype=np.float64))
    shape = tuple(int(s) for s in np.atleast_1d(shape))
    if not 1 <= len(axes) <= 3 or len(axes) != len(shape):
        raise ValueError(f"a grid takes one to three axes and one point count per axis (got {len(axes)} axes, shape {list(shape)})")
    if axes.shape[1] != origin.shape[0]:
        raise ValueError("the grid's axes must have as many components as its origin")
    if min(shape) < 2:
        raise ValueError("a grid needs at least two points per axis (the end points)")
    if not np.all(np.abs(axes).sum(axis=1) > 0):
        raise ValueError("a grid axis must not be the zero vector")
    xyz = np.broadcast_to(origin, shape + origin.shape).copy()
    for k, (a, s) in enumerate(zip(axes, shape)):
        t = np.linspace(0.0, 1.0, s).reshape((1,) * k + (s,) + (1,) * (len(shape) - k - 1) + (1,))
        xyz += t * a
    return xyz


def _backend(problem):
    if problem.comm.size > 1:
        raise NotImplementedError(f"{FEATURE} runs on one rank: a plan searches this rank's owned cells only and the merge over ranks "
                                  "(lowest rank that found the point) is not implemented")
    be = getattr(problem, "backend", None)
    if be is None:
        if not hasattr(problem, "ion_list"):      # ProblemEMI creates its context in setup_bilinear_form()
            raise _lib.KnpError("the problem has no library context yet (ProblemEMI: call setup_bilinear_form() first)")
        be = problem.create_backend()
    return be


def _ptrs(fields, n):
    if fields is None:
        return None
    if len(fields) != n:
        raise ValueError("functions_i and functions_e must list the same number of fields")
    return (C.c_void_p * n)(*[None if f is None else f.data_ptr() for f in fields])


class FieldSampler:
    """P1 evaluation of nodal fields at fixed ``points`` [n, dim] in metres.  ``side``: 0 search intracellular cells only, 1
    extracellular only, None any cell.  ``cell`` (local cell index, -1 where no cell contains the point), ``cell_tag`` (-1 there),
    ``weights`` [n, dim + 1] and ``found`` are NumPy arrays in the order of ``points``."""

    def __init__(self, problem, points, side=None):
        be = _backend(problem)
        lm = problem.local_mesh
        dim = lm.coords.shape[1]
        pts = np.atleast_2d(np.asarray(points, dtype=np.float64))
        if pts.ndim != 2 or pts.shape[0] == 0 or pts.shape[1] < dim:
            raise ValueError(f"points must be a non-empty [n, {dim}] array")
        if side not in (None, 0, 1):
            raise ValueError("side must be None, 0 (intracellular) or 1 (extracellular)")
        pts = np.ascontiguousarray(pts[:, :dim])
        self.backend, self.points, self.side, self.n_points, self.dim = be, pts, side, pts.shape[0], dim
        self.n_vertices = lm.coords.shape[0]
        self.plan = None
        b = self.bins = bin_points(pts)
        plan = C.c_int32(-1)
        origin, size = np.ascontiguousarray(b["origin"]), np.ascontiguousarray(b["size"])
        be.check(be.lib.knp_sample_plan_create(be.ctx, self.n_points, pts.ctypes.data_as(_lib.f64p), -1 if side is None else int(side),
                                               len(b["bin_ptr"]) - 1, b["bin_ptr"].ctypes.data_as(_lib.i32p),
                                               b["bin_pts"].ctypes.data_as(_lib.i32p), origin.ctypes.data_as(_lib.f64p),
                                               size.ctypes.data_as(_lib.f64p), b["shape"].ctypes.data_as(_lib.i32p), C.byref(plan)))
        self.plan = int(plan.value)
        cell = np.empty(self.n_points, dtype=np.int32)
        w = np.empty((self.n_points, dim + 1), dtype=np.float64)
        be.check(be.lib.knp_sample_plan_get(be.ctx, self.plan, cell.ctypes.data_as(_lib.i32p), w.ctypes.data_as(_lib.f64p)))
        self.cell, self.weights, self.found = cell.astype(np.int64), w, cell >= 0
        tags = np.asarray(lm.cell_tags, dtype=np.int32)
        self.cell_tag = np.where(self.found, tags[np.maximum(cell, 0)], -1).astype(np.int32)

    def close(self):
        """free the plan's device memory (also done when the sampler or its problem's context goes away)"""
        be, plan = getattr(self, "backend", None), getattr(self, "plan", None)
        self.plan = None
        if plan is not None and be is not None and getattr(be, "ctx", None):
            be.lib.knp_sample_plan_destroy(be.ctx, plan)

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass

    def _check(self, f):
        t = f.x.array if hasattr(f, "x") else f
        if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.numel() != self.n_vertices:
            raise ValueError("a sampled field is a Function or a contiguous float64 device tensor with one value per local vertex")

    def __call__(self, functions_i, functions_e=None, out=None, fill=float("nan")):
        """values[f, point] on the device: ``functions_i[f]`` where the point's cell is intracellular, ``functions_e[f]`` where it is
        extracellular, ``fill`` where no cell contains the point.  Each list holds Functions or device tensors [n_vertices]; the list
        of a side that no located point needs may be None.  Enqueued: no host copy, no synchronisation.  ``out``: a contiguous float64
        device tensor of n_fields * n_points entries, else a new one of shape [n_fields, n_points]."""
        if self.plan is None:
            raise _lib.KnpError("the sampler is closed")
        if functions_i is None and functions_e is None:
            raise ValueError("no fields to sample")
        nf = len(functions_i if functions_i is not None else functions_e)
        for fs in (functions_i, functions_e):
            for f in (fs or ()):
                if f is not None:
                    self._check(f)
        be = self.backend
        if out is None:
            out = torch.empty((nf, self.n_points), dtype=torch.float64, device=be.device)
        if not (out.is_contiguous() and out.dtype == torch.float64 and out.is_cuda and out.numel() == nf * self.n_points):
            raise ValueError(f"out must be a contiguous float64 device tensor of {nf} x {self.n_points} entries")
        be.check(be.lib.knp_sample(be.ctx, self.plan, nf, _ptrs(functions_i, nf), _ptrs(functions_e, nf), float(fill),
                                   C.c_void_p(out.data_ptr())))
        return out


class GridSampler(FieldSampler):
    """A ``FieldSampler`` on the lattice ``origin + sum_k t_k axes[k]`` (metres): ``axes`` one, two or three edge vectors, ``shape``
    the points per axis, end points included.  ``xyz`` is [*shape, dim]; ``cell``, ``cell_tag``, ``found`` are [*shape], ``weights``
    [*shape, dim + 1], and a call returns [n_fields, *shape]."""

    def __init__(self, problem, origin, axes, shape, side=None):
        dim = problem.local_mesh.coords.shape[1]
        origin = np.asarray(origin, dtype=np.float64).ravel()[:dim]
        axes = np.atleast_2d(np.asarray(axes, dtype=np.float64))[:, :dim]
        self.xyz = grid_points(origin, axes, shape)
        self.shape = self.xyz.shape[:-1]
        super().__init__(problem, self.xyz.reshape(-1, dim), side)
        self.cell, self.cell_tag, self.found = (a.reshape(self.shape) for a in (self.cell, self.cell_tag, self.found))
        self.weights = self.weights.reshape(self.shape + (dim + 1,))

    def __call__(self, functions_i, functions_e=None, out=None, fill=float("nan")):
        return super().__call__(functions_i, functions_e, out, fill).view((-1,) + self.shape)


def merged_functions(problem, fields=None):
    """(names, functions_i, functions_e) of the merged fields of a KNP-EMI problem: ``fields`` a subset of ``MERGED_FIELDS`` (default
    all) -- ion k is ``wh[side][k]``, ``phi`` the potential ``wh[side][N_ions]``"""
    names = list(MERGED_FIELDS if fields is None else fields)
    index = {ion["name"]: k for k, ion in enumerate(problem.ion_list)}
    index["phi"] = problem.N_ions
    bad = [nm for nm in names if nm not in index]
    if bad:
        raise ValueError(f"unknown field name(s) {bad}: choose from {list(index)}")
    return names, [problem.wh[0][index[nm]] for nm in names], [problem.wh[1][index[nm]] for nm in names]
