"""Per-tag diagnostics of a run: ion amounts, charge, volume and membrane area per cell tag (reference
KNPEMIx_problem.py:807-843, ``print_conservation``), the stimulus-current trace (KNPEMIx_solver.py:578-585, 604-610, 855-857), the
trans-membrane ion fluxes per membrane tag (utils/calc_fluxes.py; KNPEMIx_solver.py:626-627, 641-643) and the membrane potential
per membrane tag (what utils/plot_membrane_potentials.py:48-128 reads per cell from the reference's checkpoints).

The tag maps and the time-invariant measures are built here, on the host, once; the integrals of the fields are HIP kernels
(csrc/knp_diagnostics.inc, ``knp_diag_*``) that run on the library's stream and write device buffers.  Reading a result is the
only synchronisation, and the time loop never reads one unless the problem prints every step.
"""
from __future__ import annotations

import math

import numpy as np

from . import fem

# valences the reference hard-codes in the charge of print_conservation (KNPEMIx_problem.py:840)
CHARGE_VALENCES = (1.0, 1.0, -1.0)


def tag_map(item_tags, tag_values):
    """Items (cells or facets) sorted by the dense index of their tag in ``tag_values``: returns ``seg_ptr`` [n_tags + 1] and
    ``items`` (positions in ``item_tags``), int32.  Items whose tag is not listed are left out; the sort is stable."""
    tag_values = np.asarray(tag_values, dtype=np.int64)
    item_tags = np.asarray(item_tags, dtype=np.int64)
    if len(np.unique(tag_values)) != len(tag_values):
        raise ValueError("tag values must be distinct")
    order = np.argsort(tag_values, kind="stable")
    pos = np.searchsorted(tag_values[order], item_tags)
    pos = np.minimum(pos, max(len(tag_values) - 1, 0))
    known = (tag_values[order][pos] == item_tags) if len(tag_values) else np.zeros(len(item_tags), bool)
    dense = np.where(known, order[pos] if len(tag_values) else 0, -1)
    sel = np.nonzero(dense >= 0)[0]
    items = sel[np.argsort(dense[sel], kind="stable")].astype(np.int32)
    counts = np.bincount(dense[sel], minlength=len(tag_values))
    seg_ptr = np.zeros(len(tag_values) + 1, dtype=np.int32)
    np.cumsum(counts, out=seg_ptr[1:])
    return seg_ptr, items


def cell_volumes(coords, cells):
    d = coords.shape[1]
    X = coords[cells]
    return np.abs(np.linalg.det(X[:, 1:, :] - X[:, :1, :])) / math.factorial(d)


def owned_facets(problem):
    """Membrane facets this rank counts: the owner of the facet's first vertex (rule of ``integrate_over_membrane``)."""
    lm = problem.local_mesh
    if not len(problem._fv):
        return np.zeros(0, dtype=bool)
    return problem._fv[:, 0] < lm.n_vertices_owned


def facet_group_map(problem, groups):
    """This rank's membrane facets (``owned_facets``) whose membrane tag is in ``groups[t]``, sorted by t: ``seg_ptr``
    [len(groups) + 1] and ``facets`` (indices into the mesh's gamma list), int32.  A facet goes to the first group that lists its
    tag; a group none of whose tags has an owned facet keeps an empty segment."""
    p = problem
    own = np.nonzero(owned_facets(p))[0]
    ftags = np.asarray(p.gamma_facet_tags)[own]
    first = {}                                # membrane tag -> the first group that lists it (one pass: a group per cell is usual)
    for t, tags in enumerate(groups):
        for tag in tags:
            first.setdefault(int(tag), t)
    keys = np.array(sorted(first), dtype=np.int64)
    vals = np.array([first[k] for k in keys], dtype=np.int64)
    group_of = np.full(len(own), -1, dtype=np.int64)
    if len(keys) and len(own):
        pos = np.minimum(np.searchsorted(keys, ftags), len(keys) - 1)
        hit = keys[pos] == ftags
        group_of[hit] = vals[pos[hit]]
    seg_ptr, items = tag_map(group_of, np.arange(len(groups)))
    return seg_ptr, np.ascontiguousarray(own[items], dtype=np.int32)


def stimulus_box(problem):
    """The stimulus region as an open box ``(lo, hi)``, two float64 [3] in metres with -inf / +inf on the axes it leaves free
    (the mask of the flux forms, utils/calc_fluxes.py:36-68); None without a ``stimulus_region``."""
    p = problem
    if not getattr(p, "stimulus_region", False):
        return None
    lo, hi = np.full(3, -np.inf), np.full(3, np.inf)
    if p.multiple_stimulus_directions:
        pairs = [(ax, p.stimulus_region_range[i]) for i, ax in enumerate(p.stimulus_region_directions)]
    else:
        pairs = [(p.stimulus_region_direction, p.stimulus_region_range)]
    for ax, rng in pairs:                     # a product of indicator functions: an axis listed twice keeps the intersection
        lo[ax], hi[ax] = max(lo[ax], float(rng[0])), min(hi[ax], float(rng[1]))
    return lo, hi


def flux_coefficients(problem):
    """``D_k`` and ``z_k / psi`` of the flux forms as they are now (both sides use the ion's ``Di``, utils/calc_fluxes.py:79)"""
    p = problem
    psi = float(p.psi.value)
    D = np.array([float(ion["Di"].value) for ion in p.ion_list], dtype=np.float64)
    zp = np.array([float(ion["z"].value) / psi for ion in p.ion_list], dtype=np.float64)
    return D, zp


def facet_areas(problem, seg_ptr, facets):
    """area of every segment of a facet map (this rank's part)"""
    dense = np.repeat(np.arange(len(seg_ptr) - 1), np.diff(seg_ptr))
    return np.bincount(dense, weights=problem._fmeas[facets], minlength=len(seg_ptr) - 1).astype(np.float64)


class FacetGroupLayout:
    """Facet groups of a membrane reduction (fluxes, membrane potential, membrane integral) on this rank: ``groups`` (tuples of
    membrane tags), ``tags`` (each group's first tag), the facet map (``facet_group_map``) and ``area``, this rank's part of
    A_t = sum_F |F| per group."""

    def __init__(self, problem, groups):
        self.groups = tuple(tuple(int(t) for t in g) for g in groups)
        self.tags = np.array([g[0] if g else -1 for g in self.groups], dtype=np.int64)
        self.seg_ptr, self.facets = facet_group_map(problem, self.groups)
        self.area = facet_areas(problem, self.seg_ptr, self.facets)

    @property
    def n_groups(self):
        return len(self.groups)


def reduce_membrane_potential(parts, areas):
    """Per-rank device results ``parts`` ([n, 3] = integral, min, max each; [..., n, 3] for traces) and per-rank ``areas`` [n],
    reduced in rank order by sum / min / max: returns the area [n] and (mean, min, max) in the shape of one part.  A group without
    a facet on any rank has area 0 and NaN for all three."""
    area = np.sum(areas, axis=0)
    I = np.sum([q[..., 0] for q in parts], axis=0)
    lo = np.min([q[..., 1] for q in parts], axis=0)
    hi = np.max([q[..., 2] for q in parts], axis=0)
    none = area == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(none, np.nan, I / area)
    return area, np.stack([mean, np.where(none, np.nan, lo), np.where(none, np.nan, hi)], axis=-1)


def threshold_crossings(trace, times, threshold):
    """Upward crossings of ``threshold`` per column of ``trace`` [records, n] sampled at ``times`` [records]: a crossing lies
    between records i and i + 1 when trace[i] < threshold <= trace[i + 1].  Returns ``count`` [n] (int64) and ``first`` [n], the
    linearly interpolated time of the first one (the sample's own time when it equals the threshold), NaN where there is none.
    Applied to ``phi_m_tags.npy[:, :, 0]`` it gives the activation time of every cell."""
    v = np.asarray(trace, dtype=np.float64)
    t = np.asarray(times, dtype=np.float64)
    if v.ndim == 1:
        v = v[:, None]
    if v.ndim != 2 or t.shape != (v.shape[0],):
        raise ValueError("trace must be [records, n] and times [records]")
    n = v.shape[1]
    count = np.zeros(n, dtype=np.int64)
    first = np.full(n, np.nan)
    if v.shape[0] < 2:
        return count, first
    up = (v[:-1] < threshold) & (v[1:] >= threshold)
    count = up.sum(axis=0).astype(np.int64)
    cols = np.nonzero(count > 0)[0]
    i = np.argmax(up[:, cols], axis=0)
    a, b = v[i, cols], v[i + 1, cols]
    first[cols] = t[i] + (threshold - a) / (b - a) * (t[i + 1] - t[i])
    return count, first


class BudgetLayout:
    """The cell tags of a problem (ics tags, then ecs tags), their side, and on this rank: the owned cells sorted by tag, the
    volume of every tag and the membrane area of every tag (facets whose membrane tag equals the cell tag, the reference's
    ``dS(tag)``).  Volumes and areas are this rank's parts; ``ProblemKNPEMI.ion_budget`` sums them over the ranks."""

    def __init__(self, problem):
        p = problem
        lm = p.local_mesh
        intra = [int(t) for t in p.intra_tags]
        extra = [int(t) for t in np.ravel(p.extra_tag)]
        self.tags = np.array(intra + extra, dtype=np.int64)
        self.side = np.array([0] * len(intra) + [1] * len(extra), dtype=np.int64)
        nco = int(lm.n_cells_owned)
        self.seg_ptr, self.cells = tag_map(lm.cell_tags[:nco], self.tags)
        vol = cell_volumes(lm.coords, lm.cells[:nco])
        dense = np.repeat(np.arange(len(self.tags)), np.diff(self.seg_ptr))
        self.volume = np.bincount(dense, weights=vol[self.cells], minlength=len(self.tags))
        self.area = np.zeros(len(self.tags))
        own = owned_facets(p)
        if own.any():
            fptr, fitems = tag_map(np.asarray(p.gamma_facet_tags)[own], self.tags)
            fdense = np.repeat(np.arange(len(self.tags)), np.diff(fptr))
            self.area = np.bincount(fdense, weights=p._fmeas[own][fitems], minlength=len(self.tags))

    @property
    def n_tags(self):
        return len(self.tags)


def membrane_program(problem, expr):
    """Compile one membrane expression with the field roles of the mechanism programs (output 0).  It may only read the
    auxiliary fields the mechanism programs already read: the assembly's field table stays as it is."""
    p = problem
    roles = {}
    for j in range(p.N_ions):
        roles[id(p.wh[0][j])] = ("KI", j)
        roles[id(p.wh[1][j])] = ("KE", j)
    roles[id(p.phi_m_prev)] = ("PHIM", 0)
    aux = list(getattr(p, "aux_functions", []))
    n0 = len(aux)
    spec = fem.compile_program([expr], roles, aux)
    if len(aux) != n0:
        raise ValueError("a diagnostic expression reads a nodal field that no membrane mechanism reads")
    return spec
