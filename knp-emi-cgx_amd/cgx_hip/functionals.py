"""Integrals of user expressions over cell tags on the device (csrc/knp_functional.inc, ``knp_functional_*`` of
include/knpemi_hip.h): the reference's ``dfx.fem.assemble_scalar(dfx.fem.form(<UFL expression> * dx(tag)))``.

An integrand is an expression of cgx_hip/fem.py: the problem's Functions (concentrations, potentials, ``phi_m_prev``, gates,
declared states) and the user's own, their derivatives (``fem.grad``, ``fem.inner``), Constants, coordinates, and every operation
the membrane-program compiler knows.  A ``VolumeFunctional`` compiles it once to the bytecode of the membrane programs, uploads
the cells of the chosen tags sorted by tag, and then evaluates it at the points of a simplex rule per call: one launch pair per
side, into a device tensor, without a host copy or a synchronisation.  Time-dependent Constants are read anew at every call.

``compile_functional`` is the host part (expression -> programs, tags -> cell lists, degree -> rule); it needs no device.

``MembraneFunctional`` is the same over membrane tags (csrc/knp_membrane_functional.inc, ``knp_membrane_functional_*``): the
reference's ``assemble_scalar(form(<UFL expression> * dS(tag)))``.  There an integrand may also hold restricted derivatives
(``fem.grad(f)[a]('+')``), the facet normal (``fem.FacetNormal``) and normal derivatives (``fem.NormalDerivative``, ``fem.dot``);
``compile_membrane_functional`` is its host part.
"""
from __future__ import annotations

import collections
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, fem
from .diagnostics import cell_volumes, tag_map

FEATURE = "volume functionals (VolumeFunctional / assemble_scalar / add_functional)"
MEMBRANE_FEATURE = "membrane functionals (MembraneFunctional / assemble_scalar_membrane / add_functional)"
MAX_OUTPUTS = 3


def quadrature(dim, degree):
    """The rule of a functional: ``mms.simplex_quadrature(dim, ceil((degree + 1) / 2))``, exact to ``degree`` -- barycentric points
    [n_q, dim + 1] and weights summing to one"""
    from .mms import simplex_quadrature
    if int(degree) != degree or degree < 0:
        raise ValueError("degree must be a non-negative integer")
    m = max(1, math.ceil((int(degree) + 1) / 2))
    if m ** dim > _lib.KNP_FUNCTIONAL_MAX_Q:
        raise ValueError(f"degree {degree} needs {m ** dim} quadrature points per cell, more than {_lib.KNP_FUNCTIONAL_MAX_Q}")
    pts, w = simplex_quadrature(dim, m)
    return np.ascontiguousarray(pts, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)


def field_roles(problem):
    """id(Function) -> role of the solution functions a functional's program reads directly: the first three functions of each
    side of a KNP-EMI problem are ``KI j`` / ``KE j``.  Everything else (potentials, phi_m, gates, states, user Functions, all
    functions of an EMI problem) takes an aux slot."""
    roles = {}
    if hasattr(problem, "ion_list"):
        for j in range(min(3, len(problem.wh[0]))):
            roles[id(problem.wh[0][j])] = ("KI", j)
            roles[id(problem.wh[1][j])] = ("KE", j)
    return roles


def _side_functions(problem, side):
    wh = problem.wh[side]
    return list(wh) if isinstance(wh, (list, tuple)) else [wh]


def _functions_of(e, found):
    e = fem.as_expr(e)
    if isinstance(e, fem.Function):
        found.append(e)
    elif isinstance(e, (fem.Derivative, fem.NormalDerivative)):
        found.append(e.function)
    elif isinstance(e, fem.Op):
        for a in e.args:
            _functions_of(a, found)
    return found


class SideProgram:
    """One side of a functional: its tags, the owned cells of those tags sorted by tag, the program and its bindings"""

    def __init__(self, side, tags, seg_ptr, cells, volume, spec):
        self.side, self.tags, self.seg_ptr, self.cells, self.volume, self.spec = side, tags, seg_ptr, cells, volume, spec


class FunctionalSpec:
    """What ``compile_functional`` returns: ``sides`` (a ``SideProgram`` per side that has tags), the rule ``q_bary`` / ``q_w``,
    ``n_out``, ``single`` (the integrand was one expression, not a list) and ``tags`` / ``side`` / ``volume`` per row of the result:
    the intracellular tags first, each side's in the order given."""


def compile_functional(problem, integrand_i=None, integrand_e=None, tags=None, degree=2):
    p = problem
    lm = p.local_mesh
    dim = lm.coords.shape[1]
    given = [integrand_i, integrand_e]
    if given[0] is None and given[1] is None:
        raise ValueError("a functional needs integrand_i, integrand_e or both")
    single = not any(isinstance(g, (list, tuple)) for g in given if g is not None)
    outs = [None if g is None else [fem.as_expr(e) for e in (g if isinstance(g, (list, tuple)) else [g])] for g in given]
    counts = {len(o) for o in outs if o is not None}
    if len(counts) != 1 or not 1 <= next(iter(counts)) <= MAX_OUTPUTS:
        raise ValueError(f"an integrand is one expression or a list of up to {MAX_OUTPUTS}, and both sides give the same number")
    n_out = counts.pop()
    side_tags = [[int(t) for t in p.intra_tags], [int(t) for t in np.ravel(p.extra_tag)]]
    if tags is None:
        chosen = [side_tags[s] if outs[s] is not None else [] for s in range(2)]
    else:
        tags = [int(t) for t in np.ravel(tags)]
        if len(set(tags)) != len(tags):
            raise ValueError("a tag is listed twice")
        chosen = [[], []]
        for t in tags:
            s = 0 if t in side_tags[0] else 1 if t in side_tags[1] else None
            if s is None:
                raise ValueError(f"unknown cell tag {t}: the problem has the intracellular tags {side_tags[0]} and the extracellular {side_tags[1]}")
            if outs[s] is None:
                raise ValueError(f"tag {t} is {'intra' if s == 0 else 'extra'}cellular and integrand_{'ie'[s]} is not given")
            chosen[s].append(t)
    roles = field_roles(p)
    other = [{id(f) for f in _side_functions(p, 1 - s)} for s in range(2)]
    spec = FunctionalSpec()
    spec.q_bary, spec.q_w = quadrature(dim, degree)
    spec.n_out, spec.single, spec.degree, spec.sides = n_out, single, int(degree), []
    nco = int(lm.n_cells_owned)
    vol = cell_volumes(lm.coords, lm.cells[:nco])
    for s in range(2):
        if outs[s] is None:
            continue
        for e in outs[s]:
            for f in _functions_of(e, []):
                if id(f) in other[s]:
                    raise ValueError(f"integrand_{'ie'[s]} reads '{f.name}', a solution function of the other side")
        if not chosen[s]:
            continue
        aux, derivs = [], []
        try:
            prog = fem.compile_program(outs[s], roles, aux, derivs)
        except fem.AuxSlotsExhausted:
            raise ValueError(f"integrand_{'ie'[s]} binds more than {_lib.KNP_MAX_AUX} fields and derivatives to aux slots") from None
        if len(prog.const_sources) > _lib.KNP_DIAG_MAX_CONSTS:
            raise ValueError(f"integrand_{'ie'[s]} has more than {_lib.KNP_DIAG_MAX_CONSTS} constants")
        tg = np.array(chosen[s], dtype=np.int64)
        seg_ptr, cells = tag_map(lm.cell_tags[:nco], tg)
        dense = np.repeat(np.arange(len(tg)), np.diff(seg_ptr))
        spec.sides.append(SideProgram(s, tg, seg_ptr, cells, np.bincount(dense, weights=vol[cells], minlength=len(tg)), prog))
    cat = lambda key, dt: np.concatenate([np.asarray(getattr(sp, key), dtype=dt) for sp in spec.sides]) if spec.sides else np.zeros(0, dtype=dt)
    spec.tags, spec.volume = cat("tags", np.int64), cat("volume", np.float64)
    spec.side = np.concatenate([np.full(len(sp.tags), sp.side, dtype=np.int64) for sp in spec.sides]) if spec.sides else np.zeros(0, dtype=np.int64)
    return spec


def _backend(problem, feature, items):
    if problem.comm.size > 1:
        raise NotImplementedError(f"{feature} run on one rank: a functional integrates this rank's owned {items} only and the sum over "
                                  "ranks is not implemented")
    be = getattr(problem, "backend", None)
    if be is None:
        if not hasattr(problem, "ion_list"):      # ProblemEMI creates its context in setup_bilinear_form()
            raise _lib.KnpError("the problem has no library context yet (ProblemEMI: call setup_bilinear_form() first)")
        be = problem.create_backend()
    return be


Plan = collections.namedtuple("Plan", "id spec first n_rows")      # a plan of the library, its fem.ProgramSpec and the rows it writes


class _Functional:
    """What the two kinds share.  A functional holds ``plans``: a volume functional one per side, a membrane functional one.  A kind
    names its entry points of the library (``ABI``), what it integrates over (``FEATURE``, ``ITEMS``) and its role map (``roles``);
    its constructor sets ``spec``, ``tags``, ``n_out`` and its own per-row attributes, calls ``_open`` and then ``_create`` per plan."""

    def _open(self, problem):
        self.problem, self.plans, self.n_plans = problem, [], 0
        self.backend = _backend(problem, self.FEATURE, self.ITEMS)
        self.n_vertices = problem.local_mesh.coords.shape[0]

    def _create(self, prog, n_rows, seg_ptr, items, q_pts, q_w):
        """one plan for the next ``n_rows`` rows: the items of every row (``seg_ptr`` into ``items``), the rule and the program"""
        be = self.backend
        i32, f64 = (lambda a: a.ctypes.data_as(_lib.i32p)), (lambda a: a.ctypes.data_as(_lib.f64p))
        code = np.ascontiguousarray(prog.code, dtype=np.int32)
        consts = prog.constants()
        modes = np.ascontiguousarray(prog.aux_derivs, dtype=np.int32)
        fid = C.c_int32(-1)
        be.check(getattr(be.lib, self.ABI + "_create")(be.ctx, n_rows, i32(seg_ptr), i32(items) if items.size else None, len(q_w), f64(q_pts),
                                                       f64(q_w), code.shape[0], i32(code), consts.shape[0], f64(consts) if consts.size else None,
                                                       modes.shape[0], i32(modes) if modes.size else None, self.n_out, C.byref(fid)))
        self.plans.append(Plan(int(fid.value), prog, sum(pl.n_rows for pl in self.plans), n_rows))
        self.n_plans = len(self.plans)
        self._fields(prog)      # refuses a Function that is not a nodal field of this mesh now, not at the first call

    def _fields(self, prog):
        """the ABI's struct of device pointers for one program, filled at every call: a Function whose ``x.array`` was bound to
        another tensor in between is read where it is now"""
        p = self.problem
        f = _lib.Fields()
        roles = self.roles(p)
        for fn in (list(p.wh[0]) + list(p.wh[1]) + [getattr(p, "phi_m_prev", None)] if roles else []):
            role = roles.get(id(fn))
            if role is None:
                continue
            if role[0] == "PHIM":
                f.phi_m = fn.data_ptr()
            else:
                (f.k_i if role[0] == "KI" else f.k_e)[role[1]] = fn.data_ptr()
        for k, fn in enumerate(prog.aux_functions):
            if fn is None:      # a normal component
                continue
            t = fn.x.array
            if t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or t.numel() != self.n_vertices:
                raise ValueError(f"'{fn.name}' is not a nodal field of this problem's mesh on the device")
            f.aux[k] = fn.data_ptr()
        return f

    def close(self):
        """free the plans' device memory (also done when the functional or its problem's context goes away)"""
        be, plans = getattr(self, "backend", None), getattr(self, "plans", [])
        self.plans = []
        if be is not None and getattr(be, "ctx", None):
            for plan in plans:
                getattr(be.lib, self.ABI + "_destroy")(be.ctx, plan.id)

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass

    def __call__(self, out=None):
        """The integrals per row, [n_tags, n_out] on the device; the constants and the tensors' addresses are read anew.  Enqueued:
        no host copy, no synchronisation.  ``out``: a contiguous float64 device tensor of that size (a row of a preallocated trace),
        else a new one."""
        be = self.backend
        if self.n_plans and not self.plans:
            raise _lib.KnpError("the functional is closed")
        shape = (len(self.tags), self.n_out)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=be.device)
        if not (out.is_contiguous() and out.dtype == torch.float64 and out.is_cuda and out.numel() == shape[0] * shape[1]):
            raise ValueError(f"out must be a contiguous float64 device tensor of {shape[0]} x {shape[1]} entries")
        for plan in self.plans:
            f = self._fields(plan.spec)
            consts = plan.spec.constants()
            if consts.size:
                be.check(getattr(be.lib, self.ABI + "_set_constants")(be.ctx, plan.id, consts.shape[0], consts.ctypes.data_as(_lib.f64p)))
            be.check(getattr(be.lib, self.ABI + "_eval")(be.ctx, plan.id, C.byref(f), C.c_void_p(out.data_ptr() + 8 * plan.first * self.n_out)))
        return out.view(shape)

    def value(self):
        """the integrals per row as NumPy [n_tags, n_out] (one read-back)"""
        return self().cpu().numpy()

    def total(self):
        """the sum over the rows, [n_out]"""
        return self.value().sum(axis=0)


def _total_once(F):
    """one evaluation of a new functional, the sum over its rows: a float where the integrand was one expression"""
    try:
        tot = F.total()
    finally:
        F.close()
    return float(tot[0]) if F.spec.single else tot


class VolumeFunctional(_Functional):
    """Per cell tag, the integral of ``integrand_i`` (intracellular tags) or ``integrand_e`` (extracellular tags) with a rule exact to
    polynomial ``degree``.  Each integrand is one expression or a list of up to three (both sides the same number); ``tags``: None
    for every cell tag of the sides that have an integrand.  ``tags`` / ``side`` / ``volume``: per row of the result -- the
    intracellular tags first, each side's in the order given.  A call returns the device tensor [n_tags, n_out]."""
    ABI, ITEMS = "knp_functional", "cells"
    FEATURE = FEATURE
    roles = staticmethod(field_roles)

    def __init__(self, problem, integrand_i=None, integrand_e=None, tags=None, degree=2):
        spec = self.spec = compile_functional(problem, integrand_i, integrand_e, tags, degree)
        self.tags, self.side, self.volume, self.n_out, self.degree = spec.tags, spec.side, spec.volume, spec.n_out, spec.degree
        self._open(problem)
        for sp in spec.sides:
            self._create(sp.spec, len(sp.tags), sp.seg_ptr, sp.cells, spec.q_bary, spec.q_w)


def assemble_scalar(problem, integrand_i=None, integrand_e=None, tags=None, degree=2):
    """what ``ProblemKNPEMI.assemble_scalar`` and ``ProblemEMI.assemble_scalar`` do: one functional, one evaluation, the sum over tags"""
    return _total_once(VolumeFunctional(problem, integrand_i, integrand_e, tags, degree))


# ------------------------------------------------------------------------------------------ membrane functionals
def membrane_field_roles(problem):
    """``field_roles`` and, on a KNP-EMI problem, ``phi_m_prev`` as ``PHIM``: the roles of the membrane programs"""
    roles = field_roles(problem)
    if roles and getattr(problem, "phi_m_prev", None) is not None:
        roles[id(problem.phi_m_prev)] = ("PHIM", 0)
    return roles


class MembraneFunctionalSpec:
    """What ``compile_membrane_functional`` returns: ``spec`` (the ``fem.ProgramSpec``; ``aux_derivs`` are the slot modes of
    knp_membrane_functional_create, ``aux_functions`` has None for a normal component), the rule ``q_pts`` / ``q_w``, ``n_out``,
    ``single``, and per row of the result ``groups`` (tuples of membrane tags), ``tags`` (each group's first tag) and ``area``, with
    the facet map ``seg_ptr`` / ``facets`` (indices into the problem's gamma list)."""


def compile_membrane_functional(problem, integrand, tags=None, degree=10):
    from .diagnostics import FacetGroupLayout
    from .mesh import facet_quadrature
    p = problem
    dim = p.local_mesh.coords.shape[1]
    single = not isinstance(integrand, (list, tuple))
    outs = [fem.as_expr(e) for e in ([integrand] if single else integrand)]
    if not 1 <= len(outs) <= MAX_OUTPUTS:
        raise ValueError(f"an integrand is one expression or a list of up to {MAX_OUTPUTS}")
    known = [int(t) for t in p.gamma_tags]
    groups = [(t,) for t in known] if tags is None else [tuple(int(t) for t in g) if isinstance(g, (list, tuple)) else (int(g),)
                                                        for g in tags]
    listed = [t for g in groups for t in g]
    if len(set(listed)) != len(listed):
        raise ValueError("a membrane tag is listed twice")
    for g in groups:
        if not g:
            raise ValueError("an empty group of membrane tags")
        for t in g:
            if t not in known:
                raise ValueError(f"unknown membrane tag {t}: the problem has the membrane tags {known}")
    if int(degree) != degree or degree < 0:
        raise ValueError("degree must be a non-negative integer")
    n_q = (int(degree) // 2 + 1) ** (dim - 1)
    if n_q > _lib.KNP_FUNCTIONAL_MAX_Q:
        raise ValueError(f"degree {degree} needs {n_q} quadrature points per facet, more than {_lib.KNP_FUNCTIONAL_MAX_Q}")
    sides = {id(f): s for s in range(2) for f in _side_functions(p, s)}
    aux, modes = [], []
    try:
        prog = fem.compile_program(outs, membrane_field_roles(p), aux, modes, facet_sides=sides)
    except fem.AuxSlotsExhausted:
        raise ValueError(f"the integrand binds more than {_lib.KNP_MAX_AUX} fields, derivatives and normal components to aux slots") from None
    if len(prog.const_sources) > _lib.KNP_DIAG_MAX_CONSTS:
        raise ValueError(f"the integrand has more than {_lib.KNP_DIAG_MAX_CONSTS} constants")
    lay = FacetGroupLayout(p, groups)
    spec = MembraneFunctionalSpec()
    q_pts, q_w = facet_quadrature(dim, int(degree))
    spec.q_pts, spec.q_w = np.ascontiguousarray(q_pts, dtype=np.float64), np.ascontiguousarray(q_w, dtype=np.float64)
    spec.spec, spec.n_out, spec.single, spec.degree = prog, len(outs), single, int(degree)
    spec.groups, spec.tags, spec.area, spec.seg_ptr, spec.facets = lay.groups, lay.tags, lay.area, lay.seg_ptr, lay.facets
    return spec


class MembraneFunctional(_Functional):
    """Per membrane tag, the integral of ``integrand`` over that tag's facets with a facet rule exact to polynomial ``degree`` (10:
    the problem's own ``q_pts``).  The integrand is one expression or a list of up to three; besides what a volume functional
    takes it may hold ``fem.grad(f)[a]('+' | '-')``, ``fem.FacetNormal(mesh)[a]('+' | '-')``, ``fem.NormalDerivative(f, side)`` and
    ``fem.dot``: '+' is the intracellular cell of a facet, '-' the extracellular one.  ``tags``: None for every tag of
    ``problem.gamma_tags``, each on its own, or a list whose entries are tags or tuples of tags pooled into one row.  ``groups`` /
    ``tags`` (each row's first tag) / ``area``: per row of the result.  A call returns the device tensor [n_tags, n_out]."""

    ABI, ITEMS = "knp_membrane_functional", "facets"
    FEATURE = MEMBRANE_FEATURE
    roles = staticmethod(membrane_field_roles)

    def __init__(self, problem, integrand, tags=None, degree=10):
        spec = self.spec = compile_membrane_functional(problem, integrand, tags, degree)
        self.tags, self.groups, self.area, self.n_out, self.degree = spec.tags, spec.groups, spec.area, spec.n_out, spec.degree
        self._open(problem)
        self._create(spec.spec, len(spec.tags), spec.seg_ptr, spec.facets, spec.q_pts, spec.q_w)


def assemble_scalar_membrane(problem, integrand, tags=None, degree=10):
    """what ``assemble_scalar_membrane`` of both problem classes does: one functional, one evaluation, the sum over the rows"""
    return _total_once(MembraneFunctional(problem, integrand, tags, degree))
