"""Linear forms of user expressions on the device: ``int f v dx(tag)`` and ``int g v dS(tag)`` against the P1 test functions, one
number per vertex (csrc/knp_fields.inc; ``knp_functional_eval_load``, ``knp_membrane_functional_eval_load``, ``knp_scatter_*`` and
``knp_rhs_add_load`` of include/knpemi_hip.h).  What the reference gets from ``dfx.fem.assemble_vector(dfx.fem.form(f * v * dx))``,
and what it adds to the right-hand side of a step with ``L += dt * inner(ion['f_i'], vki) * dxi`` (KNPEMIx_problem.py:613-614).

A form takes the expressions of a functional (cgx_hip/functionals.py: ``compile_functional`` / ``compile_membrane_functional``, with
their side rules, tag rules and refusals) and evaluates them with the functional's own kernel; instead of the integral per tag the
kernel keeps, per item and local vertex a, ``meas sum_q q_w[q] lambda_a(q) f(x_q)``, and a gather without atomics adds those onto the
vertices: the same inputs give the same bits on every call.  Nothing is copied to the host and nothing waits for the device;
time-dependent Constants are read anew at every call.

``Source`` is what ``ProblemKNPEMI.add_source`` / ``add_membrane_source`` return: a form with one output that
``SolverKNPEMI.assemble()`` adds, times dt, to the rows of one unknown behind ``knp_assemble_rhs``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .fields import PROJECT_INFO
from .functionals import _Functional, compile_functional, compile_membrane_functional, field_roles, membrane_field_roles

VOLUME_FEATURE = "volume linear forms (VolumeLinearForm / assemble_vector / add_source)"
MEMBRANE_FEATURE = "membrane linear forms (MembraneLinearForm / assemble_vector_membrane / add_membrane_source)"
FIELDS = {"Na": 0, "K": 1, "Cl": 2, "phi": 3}      # the unknown of a node a source goes to: DoF = 4 * node + field


class Scatter:
    """A plan of ``knp_scatter_create``: element vectors [n_items, nv, n_out] on the device -> their sums per vertex
    [n_out, n_vertices], 0 where no item holds the vertex.  ``info()`` names what an application runs (``fields.PROJECT_INFO``)."""

    def __init__(self, backend, item_vertices):
        self.backend = backend
        iv = np.ascontiguousarray(item_vertices, dtype=np.int32)
        self.n_items, self.nv = iv.shape
        sid = C.c_int32(-1)
        backend.check(backend.lib.knp_scatter_create(backend.ctx, self.n_items, self.nv, iv.ctypes.data_as(_lib.i32p) if iv.size else None,
                                                     C.byref(sid)))
        self.id = int(sid.value)

    def info(self):
        be = self.backend
        v = np.zeros(len(PROJECT_INFO), dtype=np.int32)
        be.check(be.lib.knp_scatter_get_info(be.ctx, self.id, v.ctypes.data_as(_lib.i32p), len(v)))
        return dict(zip(PROJECT_INFO, (int(x) for x in v)))

    def __call__(self, values, n_out, out):
        """``values``: a contiguous float64 device tensor of n_items * nv * n_out entries; ``out``: one of n_out * n_vertices.
        Enqueued: no host copy, no synchronisation."""
        be = self.backend
        if self.id < 0:
            raise _lib.KnpError("the scatter plan is closed")
        if not (values.is_contiguous() and values.dtype == torch.float64 and values.is_cuda and values.numel() == self.n_items * self.nv * n_out):
            raise ValueError(f"values must be a contiguous float64 device tensor of {self.n_items} x {self.nv} x {n_out} entries")
        be.check(be.lib.knp_scatter_apply(be.ctx, self.id, C.c_void_p(values.data_ptr()) if self.n_items else None, n_out,
                                          C.c_void_p(out.data_ptr())))
        return out

    def close(self):
        be, sid = self.backend, self.id
        self.id = -1
        if sid >= 0 and getattr(be, "ctx", None):
            be.lib.knp_scatter_destroy(be.ctx, sid)

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass


class _LinearForm(_Functional):
    """What the two kinds of form share on top of ``_Functional``: every plan has one row that lists all its items, ascending, a
    buffer for their element vectors and a ``Scatter`` over their vertices; ``_row`` says which row of the result a plan fills."""

    def _open(self, problem):
        super()._open(problem)
        self._row, self._loads, self._scatter = [], [], []

    def _plan(self, row, prog, items, item_vertices, q_pts, q_w):
        items = np.ascontiguousarray(items, dtype=np.int32)
        self._create(prog, 1, np.array([0, len(items)], dtype=np.int32), items, q_pts, q_w)
        iv = np.asarray(item_vertices, dtype=np.int32).reshape(len(items), -1)
        self._row.append(row)
        self._loads.append(torch.zeros(max(iv.size * self.n_out, 1), dtype=torch.float64, device=self.backend.device))
        self._scatter.append(Scatter(self.backend, iv))

    def _assemble(self, out):
        """one load launch and one gather per plan into the rows ``out[row]``, each [n_out, n_vertices]"""
        be = self.backend
        if self.n_plans and not self.plans:
            raise _lib.KnpError("the linear form is closed")
        for plan, row, loads, sc in zip(self.plans, self._row, self._loads, self._scatter):
            f = self._fields(plan.spec)
            consts = plan.spec.constants()
            if consts.size:
                be.check(getattr(be.lib, self.ABI + "_set_constants")(be.ctx, plan.id, consts.shape[0], consts.ctypes.data_as(_lib.f64p)))
            be.check(getattr(be.lib, self.ABI + "_eval_load")(be.ctx, plan.id, C.byref(f), C.c_void_p(loads.data_ptr())))
            sc(loads[:sc.n_items * sc.nv * self.n_out], self.n_out, out[row])

    def _out(self, out, shape):
        n = int(np.prod(shape))
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=self.backend.device)
        if not (out.is_contiguous() and out.dtype == torch.float64 and out.is_cuda and out.numel() == n):
            raise ValueError(f"out must be a contiguous float64 device tensor of {' x '.join(str(s) for s in shape)} entries")
        return out.view(shape)

    def value(self):
        """the vector as NumPy (one read-back)"""
        return self().cpu().numpy()

    def close(self):
        for sc in getattr(self, "_scatter", []):
            sc.close()
        self._scatter, self._loads = [], []
        super().close()


class VolumeLinearForm(_LinearForm):
    """Per vertex v with its P1 function phi_v, ``int integrand_i phi_v dx`` over the listed intracellular cells and
    ``int integrand_e phi_v dx`` over the listed extracellular ones, with a rule exact to polynomial ``degree``, the test
    function counted in (a P1 Function at ``degree=2`` gives the mass matrix times it): expressions, sides, ``tags`` and refusals are ``VolumeFunctional``'s.  A call returns the device tensor [2, n_out, n_vertices]:
    row 0 the intracellular side, row 1 the extracellular one, 0 where a vertex has no listed cell of that side.  Per side one load
    launch (knp_functional_eval_load) and one gather (knp_scatter_apply)."""
    ABI, ITEMS = "knp_functional", "cells"
    FEATURE = VOLUME_FEATURE
    roles = staticmethod(field_roles)

    def __init__(self, problem, integrand_i=None, integrand_e=None, tags=None, degree=2, _spec=None):
        spec = self.spec = _spec if _spec is not None else compile_functional(problem, integrand_i, integrand_e, tags, degree)
        self.n_out, self.degree, self.tags = spec.n_out, spec.degree, spec.tags
        self._open(problem)
        cells = np.asarray(problem.local_mesh.cells)
        self.cells = [np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)]      # per side, the listed cells, ascending
        for sp in spec.sides:
            self.cells[sp.side] = np.sort(np.asarray(sp.cells, dtype=np.int64))
            self._plan(sp.side, sp.spec, self.cells[sp.side], cells[self.cells[sp.side]], spec.q_bary, spec.q_w)

    def __call__(self, out=None):
        """[2, n_out, n_vertices] on the device; the constants and the tensors' addresses are read anew.  Enqueued: no host copy,
        no synchronisation.  ``out``: a contiguous float64 device tensor of that size, else a new one."""
        out = self._out(out, (2, self.n_out, self.n_vertices))
        for s in range(2):
            if s not in self._row:
                out[s].zero_()
        self._assemble(out)
        return out


class MembraneLinearForm(_LinearForm):
    """Per vertex v, ``int integrand phi_v dS`` over the listed membrane facets with a facet rule exact to polynomial ``degree``,
    the test function counted in: expressions (restrictions, ``fem.FacetNormal``, ``fem.NormalDerivative``), ``tags`` (pooled groups too) and
    refusals are ``MembraneFunctional``'s.  A call returns the device tensor [n_out, n_vertices], 0 away from the listed membranes.
    One load launch (knp_membrane_functional_eval_load) and one gather."""
    ABI, ITEMS = "knp_membrane_functional", "facets"
    FEATURE = MEMBRANE_FEATURE
    roles = staticmethod(membrane_field_roles)

    def __init__(self, problem, integrand=None, tags=None, degree=10, _spec=None):
        spec = self.spec = _spec if _spec is not None else compile_membrane_functional(problem, integrand, tags, degree)
        self.n_out, self.degree, self.tags, self.groups = spec.n_out, spec.degree, spec.tags, spec.groups
        self._open(problem)
        self.facets = np.sort(np.asarray(spec.facets, dtype=np.int64))
        self.vertices = np.asarray(problem._fv, dtype=np.int64)[self.facets].reshape(len(self.facets), -1)
        self._plan(0, spec.spec, self.facets, self.vertices, spec.q_pts, spec.q_w)

    def __call__(self, out=None):
        """[n_out, n_vertices] on the device; enqueued like a volume form's call"""
        out = self._out(out, (self.n_out, self.n_vertices))
        self._assemble(out.view(1, self.n_out, self.n_vertices))
        return out


def _value_once(F):
    try:
        return F.value()
    finally:
        F.close()


def assemble_vector(problem, integrand_i=None, integrand_e=None, tags=None, degree=2):
    """what ``assemble_vector`` of both problem classes does: one form, one evaluation, NumPy [2, n_out, n_vertices]"""
    return _value_once(VolumeLinearForm(problem, integrand_i, integrand_e, tags, degree))


def assemble_vector_membrane(problem, integrand, tags=None, degree=10):
    """what ``assemble_vector_membrane`` of both problem classes does: one form, one evaluation, NumPy [n_out, n_vertices]"""
    return _value_once(MembraneLinearForm(problem, integrand, tags, degree))


# ------------------------------------------------------------------------------------------ sources of a step
def field_index(field):
    """'Na' | 'K' | 'Cl' | 'phi' or 0..3 -> the unknown's index within a node"""
    if isinstance(field, str):
        if field not in FIELDS:
            raise ValueError(f"unknown field '{field}': a source goes to one of {list(FIELDS)} (or 0..3)")
        return FIELDS[field]
    if isinstance(field, (int, np.integer)) and not isinstance(field, bool) and 0 <= int(field) <= 3:
        return int(field)
    raise ValueError(f"unknown field {field!r}: a source goes to one of {list(FIELDS)} (or 0..3)")


def _one_output(spec):
    if not spec.single or spec.n_out != 1:
        raise ValueError("a source is one expression per side: register one source per unknown")


def _sources(problem):
    """the problem's list of registered sources, in the order they are applied"""
    return problem.__dict__.setdefault("_sources", [])


class Source:
    """A registered source of a step: ``form`` (one output), the unknown ``field`` (0..3) and the ``sides`` whose rows it goes to.
    ``enabled = False`` leaves it out of the next assemblies; ``remove()`` takes it off the problem and frees its plans."""

    def __init__(self, problem, form, field, sides):
        self.problem, self.form, self.field, self.sides, self.enabled = problem, form, field, tuple(sides), True
        # the row of its own buffer that the form's plan of a side fills: a volume form has one per side, a membrane form one in all
        self._row = {s: (s if isinstance(form, VolumeLinearForm) else 0) for s in self.sides}
        self._vec = torch.zeros((max(self._row.values(), default=0) + 1, 1, form.n_vertices), dtype=torch.float64, device=form.backend.device)

    def apply(self, b, scale):
        """b[4 node + field] += scale * (the form's vector now) on the nodes of ``sides``: per side one load launch, one gather and
        one knp_rhs_add_load, all enqueued on the library's stream"""
        be = self.form.backend
        self.form._assemble(self._vec)      # the plans' rows only: a side without a plan is neither written nor read
        for s in self.sides:
            be.check(be.lib.knp_rhs_add_load(be.ctx, self.field, s, float(scale), C.c_void_p(self._vec[self._row[s]].data_ptr()),
                                             C.c_void_p(b.data_ptr())))

    def remove(self):
        srcs = _sources(self.problem)
        if self in srcs:
            srcs.remove(self)
        self.enabled = False
        self.form.close()


def add_source(problem, field, expr_i=None, expr_e=None, tags=None, degree=2):
    """what ``ProblemKNPEMI.add_source`` does"""
    f = field_index(field)
    spec = compile_functional(problem, expr_i, expr_e, tags, degree)
    _one_output(spec)
    form = VolumeLinearForm(problem, _spec=spec)
    h = Source(problem, form, f, [sp.side for sp in spec.sides])
    _sources(problem).append(h)
    return h


def add_membrane_source(problem, field, side, expr, tags=None, degree=10):
    """what ``ProblemKNPEMI.add_membrane_source`` does"""
    f = field_index(field)
    if side not in ("i", "e"):
        raise ValueError(f"unknown side {side!r}: a membrane source goes to the rows of 'i' or 'e'")
    spec = compile_membrane_functional(problem, expr, tags, degree)
    _one_output(spec)
    form = MembraneLinearForm(problem, _spec=spec)
    h = Source(problem, form, f, [0 if side == "i" else 1])
    _sources(problem).append(h)
    return h


def apply_sources(problem, backend):
    """the enabled sources of ``problem``, times dt, onto ``backend.b`` (``SolverKNPEMI.assemble``, behind ``assemble_rhs``)"""
    dt = float(problem.dt.value)
    for h in _sources(problem):
        if h.enabled:
            h.apply(backend.b, dt)
