"""Activation map of a run: per membrane vertex the time phi_m first (and last) rose through a threshold, the time it fell back,
its peak and its steepest upstroke; per membrane facet the conduction velocity of the front; per membrane tag a summary.  What
the reference would read from checkpoints of every field at every step (utils/plot_membrane_potentials*.py), recorded on the
device while the run goes: one kernel launch per ``update()`` (knp_activation_step, csrc/knp_activation.inc), no host copy and no
synchronisation before ``result()``.

Definitions (include/knpemi_hip.h has them in full).  Over the interval [t0, t1] between two updates, with v0 / v1 the vertex's phi_m
at its ends and h = t1 - t0: an upward crossing iff v0 < threshold <= v1 (the rule of ``diagnostics.threshold_crossings``), at
t0 + (threshold - v0)/(v1 - v0) h; the repolarisation is the first v0 >= repolarisation_threshold > v1 after an upward crossing;
the peak is the first largest phi_m seen since ``arm()``, the steepest upstroke the largest (v1 - v0)/h, dated at the interval's
middle.  The velocity on a facet comes from the surface gradient g of the P1 interpolant of the activation time: speed 1/|g|,
direction g/|g|; a facet with a vertex that never fired, or with g = 0, has none (NaN).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import fem
from .diagnostics import FacetGroupLayout

# rows of ``ActivationMap.state`` and columns of ``result()`` / activation.npy
STATE_ROWS = ("t_first", "t_last_up", "t_repol", "v_peak", "t_peak", "dvdt_max", "t_dvdt")
RESULT_COLUMNS = ("t_act", "t_last", "t_repol", "apd", "v_peak", "t_peak", "dvdt_max", "t_dvdt", "count")
TAG_COLUMNS = ("tag", "area", "activated_area", "t_first", "t_last", "mean_speed", "valid_area")
FILES = ("activation.npy", "activation_vertices.npy", "activation_xyz.npy", "activation_velocity.npy", "activation_facets.npy",
         "activation_tags.npy")


def parse_activation_key(out_cfg, gamma_tags):
    """``save_activation`` of ``solver.output``: None (absent or False: nothing is allocated or launched) or the keyword arguments of
    ``ActivationMap``.  True: every membrane tag at threshold 0 V; a mapping may give ``threshold`` [V], ``repolarisation_threshold``
    [V] (default: the threshold) and ``tags``.  The solver does not know a membrane model's resting value, so the default threshold
    is 0 V; -0.02 V is common."""
    key = out_cfg.get("save_activation", False)
    if key is False or key is None:
        return None
    if key is True:
        key = {}
    if not isinstance(key, dict) or set(key) - {"threshold", "repolarisation_threshold", "tags"}:
        raise ValueError("save_activation must be true or a mapping with the keys threshold, repolarisation_threshold and tags")
    thr = float(key.get("threshold", 0.0))
    rep = key.get("repolarisation_threshold", None)
    rep = thr if rep is None else float(rep)
    if not (np.isfinite(thr) and np.isfinite(rep)):
        raise ValueError("save_activation: the thresholds must be finite")
    tags = key.get("tags", None)
    if tags is not None:
        tags = [int(t) for t in tags]
        if len(set(tags)) != len(tags):
            raise ValueError("save_activation lists a tag twice")
        unknown = sorted(set(tags) - {int(t) for t in gamma_tags})
        if unknown:
            raise ValueError(f"save_activation lists the tag(s) {unknown}, which are not membrane tags of the problem")
    return {"threshold": thr, "repolarisation_threshold": rep, "tags": tags}


class ActivationMap:
    """Activation times, peaks and conduction velocity on the membranes tagged ``tags`` (default: every tag of ``gamma_tags``) of a
    ``ProblemKNPEMI`` (its ``phi_m_prev``) or a ``ProblemEMI`` (its ``phi_M``).  ``threshold`` / ``repolarisation_threshold`` in V
    (the latter defaults to the former).

    ``vertices`` (local ids of the unique vertices of the tags' owned facets, ascending), ``xyz`` [n, dim] in metres, ``facets``
    (indices into the mesh's gamma list, sorted by tag), ``facet_vertices`` [n_facets, d], ``facet_tag``, ``area`` (per facet);
    ``state`` [7, n] (``STATE_ROWS``) and ``count`` [n] are the device tensors the kernel works on."""

    def __init__(self, problem, threshold, repolarisation_threshold=None, tags=None):
        from .functionals import _backend
        p = problem
        if p.comm.size > 1:
            raise NotImplementedError("activation maps run on one rank: a map holds this rank's owned membrane facets only and the "
                                      "exchange of their shared vertices between ranks is not implemented")
        self.problem = p
        self.backend = be = _backend(p, "activation maps", "membrane facets")
        self.phi = p.phi_m_prev if hasattr(p, "phi_m_prev") else p.phi_M
        self.threshold = float(threshold)
        self.repolarisation_threshold = self.threshold if repolarisation_threshold is None else float(repolarisation_threshold)
        if not (np.isfinite(self.threshold) and np.isfinite(self.repolarisation_threshold)):
            raise ValueError("the thresholds must be finite")
        self.tags = tuple(int(t) for t in (p.gamma_tags if tags is None else tags))
        if len(set(self.tags)) != len(self.tags):
            raise ValueError("a tag is listed twice")
        lm = p.local_mesh
        lay = FacetGroupLayout(p, [(t,) for t in self.tags])
        self.facets = lay.facets
        self.facet_vertices = np.ascontiguousarray(p._fv[self.facets], dtype=np.int64).reshape(len(self.facets), p._fv.shape[1])
        self.facet_tag = np.asarray(p.gamma_facet_tags, dtype=np.int64)[self.facets]
        self.area = np.asarray(p._fmeas, dtype=np.float64)[self.facets]
        self.vertices = np.unique(self.facet_vertices).astype(np.int32)
        self.xyz = np.asarray(lm.coords, dtype=np.float64)[self.vertices]
        self.dim = int(np.asarray(lm.coords).shape[1])
        self.n_vertices_mesh = int(np.asarray(lm.coords).shape[0])
        dev = be.device
        n = len(self.vertices)
        self._vertex = torch.as_tensor(self.vertices, dtype=torch.int32, device=dev)
        self._vertex64 = self._vertex.to(torch.int64)
        self._facets = torch.as_tensor(self.facets, dtype=torch.int32, device=dev)
        self.v_last = torch.zeros(n, dtype=torch.float64, device=dev)
        self.state = torch.zeros((len(STATE_ROWS), n), dtype=torch.float64, device=dev)
        self.count = torch.zeros(n, dtype=torch.int32, device=dev)
        self._T = torch.full((self.n_vertices_mesh,), float("nan"), dtype=torch.float64, device=dev)
        self._functions = None
        self.arm()

    # ---- the detector
    def arm(self):
        """reset the state at the problem's current time and phi_m"""
        self.t = float(self.problem.t.value)
        self.backend.activation_arm(self._vertex, self.phi.x.array, self.t, self.v_last, self.state, self.count)

    def update(self):
        """one detector launch over the interval from the time of the last ``arm()`` / ``update()`` to the problem's current time;
        nothing at an unchanged time"""
        t1 = float(self.problem.t.value)
        if t1 == self.t:
            return
        self.backend.activation_step(self._vertex, self.phi.x.array, self.t, t1, self.threshold, self.repolarisation_threshold, self.v_last,
                                     self.state, self.count)
        self.t = t1

    def result(self):
        """NumPy arrays per listed vertex: ``t_act`` (first upward crossing), ``t_last`` (last one), ``t_repol``, ``apd`` = t_repol -
        t_act, ``v_peak``, ``t_peak``, ``dvdt_max``, ``t_dvdt``, ``count`` (int64).  NaN where there was no such event.  One read-back."""
        st = self.state.cpu().numpy()
        out = {"t_act": st[0].copy(), "t_last": st[1].copy(), "t_repol": st[2].copy(), "apd": st[2] - st[0], "v_peak": st[3].copy(),
               "t_peak": st[4].copy(), "dvdt_max": st[5].copy(), "t_dvdt": st[6].copy(), "count": self.count.cpu().numpy().astype(np.int64)}
        return out

    # ---- velocity and summary
    def activation_time(self):
        """the nodal activation time on the device [n_vertices of the mesh]: NaN where a vertex did not fire or is not listed"""
        self._T.fill_(float("nan"))
        if len(self.vertices):
            self._T.index_copy_(0, self._vertex64, self.state[0])
        return self._T

    def velocity(self, T=None):
        """device tensor [n_facets, 1 + dim]: speed [m/s] and unit direction of the front on every facet of ``facets``, NaN on a facet
        with a vertex that did not fire or with a zero gradient.  ``T``: another nodal time field (device, [n_vertices of the mesh])
        than the activation time.  One launch, not waited for."""
        return self.backend.activation_velocity(self._facets, self.activation_time() if T is None else self._nodal(T))

    def _nodal(self, T):
        if not (isinstance(T, torch.Tensor) and T.dtype == torch.float64 and T.is_contiguous() and T.numel() == self.n_vertices_mesh
                and T.device == self._T.device):
            raise ValueError("a nodal time field is a contiguous float64 device tensor with one value per mesh vertex")
        return T

    def summary(self, groups=None, T=None):
        """the device rows of knp_diag_activation [n_groups, 5] and the layout of the groups: (valid area, area x speed, first time,
        last time, activated area) per group; not waited for.  The facet map of the groups lives in the library's context and the
        backend keeps the record of it: maps on one problem may alternate, each call sets the groups it needs."""
        groups = tuple((int(g),) if np.isscalar(g) else tuple(int(t) for t in g) for g in (self.tags if groups is None else groups))
        return self.backend.activation_summary(groups, self.activation_time() if T is None else self._nodal(T))

    def per_tag(self, groups=None):
        """Per group (default: every tag of the map on its own; a tuple of tags pools them, as in ``MembraneFunctional``): ``tag`` (the
        group's first), ``area``, ``activated_area`` (sum |F|/d per fired vertex of F), ``t_first`` / ``t_last`` (earliest / latest
        activation time), ``mean_speed`` = sum |F| speed / ``valid_area``, ``valid_area`` (facets that have a velocity).  NaN where a
        group has nothing.  One launch pair and one read-back."""
        out, lay = self.summary(groups)
        r = out.cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            speed = np.where(r[:, 0] > 0.0, r[:, 1] / r[:, 0], np.nan)
        none = ~np.isfinite(r[:, 2])
        return {"tag": lay.tags.copy(), "area": lay.area.copy(), "activated_area": r[:, 4].copy(), "t_first": np.where(none, np.nan, r[:, 2]),
                "t_last": np.where(none, np.nan, r[:, 3]), "mean_speed": speed, "valid_area": r[:, 0].copy()}

    def functions(self):
        """``fem.Function``s ``activation_time``, ``peak`` and ``repolarisation_time`` of the state as it is now: nodal, NaN away from
        the listed membranes (for ``FieldSampler``, checkpoints and field output).  The same three objects at every call."""
        if self._functions is None:
            V = getattr(self.problem, "V", None) or fem.FunctionSpace(self.problem.mesh)
            self._functions = {nm: fem.Function(V, nm) for nm in ("activation_time", "peak", "repolarisation_time")}
        for nm, row in (("activation_time", 0), ("peak", 3), ("repolarisation_time", 2)):
            a = self._functions[nm].x.array
            a.fill_(float("nan"))
            if len(self.vertices):
                a.index_copy_(0, self._vertex64, self.state[row])
        return self._functions

    def isochrones(self, levels):
        """Contour lines of the activation time on the map's membrane facets, exact on the mesh (cgx_hip/surfaces.py): per level a
        dict with ``level``, ``xyz`` [n, 3] in metres, ``segments`` [m, 2] (indices into ``xyz``), ``facet`` [m] (index into
        ``facets``), ``tag`` [m] and ``length`` [m].  Seen from the side a facet's stored normal points to, the part that fired at or
        after the level lies to the left of a segment.  A facet with a vertex that did not fire (NaN) is skipped.  3D only: the
        contour of a 2D mesh's membrane (a set of edges) would be points, and a 2D membrane raises ``ValueError``.  One build -- one
        read-back of a count -- and one copy of the result per level."""
        from .surfaces import LevelSetSurface
        if self.dim != 3:
            raise ValueError("isochrones are lines on the membrane surface of a 3D mesh; on a 2D mesh the membrane is a set of edges")
        levels = [float(v) for v in np.atleast_1d(levels)]
        if not all(np.isfinite(levels)):
            raise ValueError("isochrone levels must be finite")
        if getattr(self, "_isolines", None) is None:
            self._isolines = LevelSetSurface(self.problem, self.facet_vertices, np.zeros(len(self.facets), dtype=np.uint8), self.facet_tag)
        S, T, out = self._isolines, self.activation_time(), []
        for lv in levels:
            S.build(T, lv)
            item = S.element_item.cpu().numpy().astype(np.int64)
            out.append({"level": lv, "xyz": S.xyz.cpu().numpy(), "segments": S.elements.cpu().numpy().astype(np.int64), "facet": item,
                        "tag": S.element_tag.cpu().numpy().astype(np.int64), "length": S.measure().cpu().numpy()})
        return out

    # ---- files
    def save(self, out_dir):
        """activation.npy [n, 9] (``RESULT_COLUMNS``), activation_vertices.npy [n] local vertex ids, activation_xyz.npy [n, dim] in m,
        activation_velocity.npy [n_facets, 1 + dim] (speed in m/s, unit direction), activation_facets.npy [n_facets, d + 1] (the
        facet's vertex ids, then its tag), activation_tags.npy [n_tags, 7] (``TAG_COLUMNS``).  Two read-backs."""
        os.makedirs(out_dir, exist_ok=True)
        vel = self.velocity()
        tags = self.per_tag()
        res = self.result()
        join = lambda name: os.path.join(out_dir, name)
        np.save(join("activation.npy"), np.stack([np.asarray(res[k], dtype=np.float64) for k in RESULT_COLUMNS], axis=1))
        np.save(join("activation_vertices.npy"), self.vertices.astype(np.int64))
        np.save(join("activation_xyz.npy"), self.xyz)
        np.save(join("activation_velocity.npy"), vel.cpu().numpy())
        np.save(join("activation_facets.npy"), np.concatenate([self.facet_vertices, self.facet_tag[:, None]], axis=1))
        np.save(join("activation_tags.npy"), np.stack([np.asarray(tags[k], dtype=np.float64) for k in TAG_COLUMNS], axis=1))
