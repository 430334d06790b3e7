"""Run artefacts of the reference's solver that need no I/O library: probe-point evaluation, membrane traces, ``.npy``
exports and nodal-field checkpoints.

Mirrors reference
  src/CGx/utils/mixed_dim_problem.py:277-287    ``point_evaluation`` config key (points scaled by mesh_conversion_factor)
  src/CGx/utils/mixed_dim_problem.py:496-632    membrane measurement vertex closest to the mesh centre (``png_dof``, owner rank)
  src/CGx/utils/mixed_dim_problem.py:744-804    default ``gamma_points`` (measurement vertex, or a vertex inside the stimulus region)
  src/CGx/KNPEMI/KNPEMIx_solver.py:551-643      init_png_savefile / save_png / init_data / save_data
  src/CGx/KNPEMI/KNPEMIx_solver.py:799-821      checkpoints of the 2(N+1) solution functions every ``save_interval`` steps
  src/CGx/KNPEMI/KNPEMIx_solver.py:833-866      export_data: file names of the ``.npy`` artefacts
  src/CGx/KNPEMI/KNPEMIx_solver.py:578-610      stimulus current integrated over the stimulus membranes at every record (stimulus.npy)
  utils/plot_membrane_potentials.py:48-128      phi_m, n, m, h of chosen cells at each cell's membrane vertex closest to the mesh centre
The reference evaluates with scifem.evaluate_function (P1 interpolation in the cell containing the point) and checkpoints with
adios4dolfinx; here the interpolation weights are found once on the host and each evaluation is one tiny device gather, and a
checkpoint is an ``.npz`` of the nodal arrays per rank (with the local-to-global vertex map).
"""
from __future__ import annotations

import os

import numpy as np
import torch


def _barycentric(coords, cells, pts, tol=1e-9):
    """For every point the first cell (lowest index) that contains it: returns (cell index or -1, weights (n_pts, d+1))."""
    d = coords.shape[1]
    X0 = coords[cells[:, 0]]                                            # (nc, d)
    T = np.stack([coords[cells[:, a + 1]] - X0 for a in range(d)], axis=2)   # (nc, d, d): columns = edge vectors
    lo = coords[cells].min(axis=1)
    hi = coords[cells].max(axis=1)
    scale = float((hi - lo).max()) if len(cells) else 1.0
    out_c = np.full(len(pts), -1, dtype=np.int64)
    out_w = np.zeros((len(pts), d + 1))
    for k, p in enumerate(pts):
        cand = np.nonzero(np.all((lo <= p + tol * scale) & (hi >= p - tol * scale), axis=1))[0]
        if cand.size == 0:
            continue
        lam = np.linalg.solve(T[cand], (p - X0[cand])[:, :, None])[:, :, 0]     # (n_cand, d)
        w = np.concatenate([1.0 - lam.sum(axis=1, keepdims=True), lam], axis=1)
        ok = np.nonzero(np.all(w >= -tol, axis=1))[0]
        if ok.size:
            j = ok[0]
            out_c[k] = cand[j]
            out_w[k] = np.clip(w[j], 0.0, 1.0)
            out_w[k] /= out_w[k].sum()
    return out_c, out_w


class PointEvaluator:
    """P1 evaluation of nodal fields at fixed points.  ``side``: 0 search intracellular cells only, 1 extracellular only,
    None any cell (membrane points: the weight of the vertex opposite the facet is zero either way)."""

    def __init__(self, problem, points, side=None):
        p = problem
        lm = p.local_mesh
        pts = np.atleast_2d(np.asarray(points, dtype=np.float64))[:, :lm.coords.shape[1]]
        sel = np.arange(lm.n_cells_owned)
        if side is not None:
            sel = sel[p.cell_side[:lm.n_cells_owned] == side]
        c, w = _barycentric(lm.coords, lm.cells[sel], pts)
        found = c >= 0
        # the lowest rank that found a point evaluates it
        owners = p.comm.all_gather_object(found.tolist())
        owner = np.full(len(pts), -1, dtype=np.int64)
        for r in range(p.comm.size - 1, -1, -1):
            owner[np.asarray(owners[r], dtype=bool)] = r
        if (owner < 0).any():
            bad = pts[owner < 0] / getattr(p, "mesh_conversion_factor", 1.0)
            raise RuntimeError(f"point_evaluation: no {'cell' if side is None else ('intracellular', 'extracellular')[side] + ' cell'} "
                               f"contains the point(s) {bad.tolist()} (mesh units)")
        self.comm = p.comm
        self.n_points = len(pts)
        self.mine = np.nonzero(owner == p.comm.rank)[0]
        dev = p.mesh.device
        verts = lm.cells[sel[c[self.mine]]] if self.mine.size else np.zeros((0, lm.cells.shape[1]), dtype=np.int64)
        self.verts = torch.as_tensor(np.ascontiguousarray(verts, dtype=np.int64), device=dev)
        self.weights = torch.as_tensor(np.ascontiguousarray(w[self.mine]), dtype=torch.float64, device=dev)

    def __call__(self, functions):
        """values[f, point] of the given Functions (one device gather + one small copy per call)."""
        out = np.zeros((len(functions), self.n_points))
        if self.mine.size:
            stack = torch.stack([(f.x.array[self.verts] * self.weights).sum(dim=1) for f in functions])
            out[:, self.mine] = stack.cpu().numpy()
        if self.comm.size > 1:
            parts = self.comm.all_gather_object(out)
            out = np.sum(parts, axis=0)
        return out


def find_membrane_measurement_vertex(problem):
    """The membrane vertex (of the facets tagged ``membrane_data_tag``) closest to the centre of the mesh's bounding box:
    sets ``png_point``, ``png_dof`` (local vertex index on the owner), ``owner_rank_membrane_vertex`` and, when the config
    gave none, ``gamma_points`` (reference mixed_dim_problem.py:496-632, 744-804)."""
    p = problem
    lm = p.local_mesh
    mm = p.get_min_and_max_coordinates()
    d = lm.coords.shape[1]
    centre = np.array([(mm[2 * a] + mm[2 * a + 1]) / 2 for a in range(d)])
    tags = p.gamma_tags if p.MMS_test else (p.membrane_data_tag,)
    sel = np.isin(p.gamma_facet_tags, tags)
    gv = np.unique(p._fv[sel]) if sel.any() else np.zeros(0, dtype=np.int64)
    gv = gv[gv < lm.n_vertices_owned]
    if gv.size:
        dist = ((lm.coords[gv] - centre) ** 2).sum(axis=1)
        k = int(np.argmin(dist))
        mine = (float(dist[k]), p.comm.rank, int(gv[k]), lm.coords[gv[k]].tolist())
    else:
        mine = (np.inf, p.comm.rank, -1, None)
    best = min(p.comm.all_gather_object(mine), key=lambda t: (t[0], t[1]))
    if best[2] < 0:
        raise RuntimeError(f"no membrane facet carries membrane_data_tag {tags}")
    p.owner_rank_membrane_vertex = best[1]
    p.png_dof = best[2]
    p.png_point = np.array([best[3]])
    p.print("Phi m measurement point: ", p.png_point[0])
    if p.gamma_points is None:
        if not p.MMS_test and p.stimulus_region:
            x = lm.coords[gv] if gv.size else np.zeros((0, d))
            mask = np.ones(len(x), dtype=bool)
            if p.multiple_stimulus_directions:
                for i, ax in enumerate(p.stimulus_region_directions):
                    mask &= (x[:, ax] > p.stimulus_region_range[i][0]) & (x[:, ax] < p.stimulus_region_range[i][1])
            else:
                ax, rng = p.stimulus_region_direction, p.stimulus_region_range
                mask &= (x[:, ax] > rng[0]) & (x[:, ax] < rng[1])
            local = x[mask][0].tolist() if mask.any() else None
            pts = [q for q in p.comm.all_gather_object(local) if q is not None]
            p.gamma_points = np.array([pts[0]]) if pts else p.png_point
        else:
            p.gamma_points = p.png_point


def find_membrane_probe_vertices(problem, tags):
    """For every membrane tag in ``tags`` the owned vertex of that tag's facets closest to the centre of the mesh's bounding box,
    by the rule of ``find_membrane_measurement_vertex`` (smallest distance, then lowest rank; on a rank the lowest vertex index):
    for ``membrane_data_tag`` it is that function's ``png_dof`` and owner (not in an MMS test, where that function searches the
    facets of all ``gamma_tags`` at once).  Returns ``owner`` [n] (rank, -1 when no facet carries
    the tag), ``vertex`` [n] (local index on the owner) and ``xyz`` [n, dim] in metres (NaN without a vertex).  One gather."""
    p = problem
    lm = p.local_mesh
    mm = p.get_min_and_max_coordinates()
    d = lm.coords.shape[1]
    centre = np.array([(mm[2 * a] + mm[2 * a + 1]) / 2 for a in range(d)])
    ftags = np.asarray(p.gamma_facet_tags, dtype=np.int64)
    order = np.argsort(ftags, kind="stable")      # facets by tag, once: a tissue mesh has thousands of tags
    want = np.asarray([int(t) for t in tags], dtype=np.int64)
    lo, hi = np.searchsorted(ftags[order], want, side="left"), np.searchsorted(ftags[order], want, side="right")
    mine = []
    for t in range(len(want)):
        gv = np.unique(p._fv[order[lo[t]:hi[t]]]) if hi[t] > lo[t] else np.zeros(0, dtype=np.int64)
        gv = gv[gv < lm.n_vertices_owned]
        if gv.size:
            dist = ((lm.coords[gv] - centre) ** 2).sum(axis=1)
            k = int(np.argmin(dist))
            mine.append((float(dist[k]), p.comm.rank, int(gv[k]), lm.coords[gv[k]].tolist()))
        else:
            mine.append((np.inf, p.comm.rank, -1, None))
    parts = p.comm.all_gather_object(mine)
    n = len(mine)
    owner, vertex, xyz = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64), np.full((n, d), np.nan)
    for t in range(n):
        best = min((q[t] for q in parts), key=lambda c: (c[0], c[1]))
        if best[2] >= 0:
            owner[t], vertex[t], xyz[t] = best[1], best[2], best[3]
    return {"owner": owner, "vertex": vertex, "xyz": xyz}


def parse_membrane_potential_keys(out_cfg, gamma_tags):
    """``save_membrane_potentials`` / ``membrane_potential_interval`` of ``solver.output``: (tags or None, interval).  True: every
    membrane tag; a list of ints: those tags, in that order; absent or False: None (nothing is allocated or launched)."""
    key = out_cfg.get("save_membrane_potentials", False)
    interval = int(out_cfg.get("membrane_potential_interval", 1))
    if interval < 1:
        raise ValueError("membrane_potential_interval must be at least 1")
    if key is False or key is None:
        return None, interval
    if key is True:
        return [int(t) for t in gamma_tags], interval
    if isinstance(key, (list, tuple)) and all(isinstance(t, (int, np.integer)) and not isinstance(t, bool) for t in key):
        tags = [int(t) for t in key]
        if len(set(tags)) != len(tags):
            raise ValueError("save_membrane_potentials lists a tag twice")
        return tags, interval
    raise ValueError("save_membrane_potentials must be true or a list of membrane tags")


def parse_sample_grids(out_cfg, dim, factor, save_interval, n_steps):
    """``sample_grids`` / ``sample_interval`` of ``solver.output``: (entries, interval).  Each entry: ``name``, ``origin`` and ``axes``
    in metres (the config gives mesh units, like point_evaluation), ``shape``, ``fields``, ``records``.  Absent or empty: ([], interval)
    and nothing is allocated or launched.  Every invalid entry raises a ValueError that names it."""
    from .sampling import MAX_GRID_BYTES, MERGED_FIELDS
    grids = out_cfg.get("sample_grids") or []
    interval = int(out_cfg.get("sample_interval", save_interval))
    if interval < 1:
        raise ValueError("sample_interval must be at least 1")
    if not isinstance(grids, (list, tuple)):
        raise ValueError("sample_grids must be a list of entries")
    entries, seen = [], set()
    for k, g in enumerate(grids):
        what = f"sample_grids[{k}]"
        if not isinstance(g, dict) or "name" not in g:
            raise ValueError(f"{what}: an entry is a mapping with a name, origin, axes and shape")
        name = str(g["name"])
        what += f" ('{name}')"
        if name in seen:
            raise ValueError(f"{what}: the name is used twice")
        seen.add(name)
        for key in ("origin", "axes", "shape"):
            if key not in g:
                raise ValueError(f"{what}: missing key '{key}'")
        try:
            origin = np.asarray(g["origin"], dtype=np.float64).ravel()
            axes = np.atleast_2d(np.asarray(g["axes"], dtype=np.float64))
            shape = [int(s) for s in np.atleast_1d(g["shape"])]
        except (TypeError, ValueError) as e:
            raise ValueError(f"{what}: origin, axes and shape must be numbers ({e})") from None
        if origin.shape[0] < dim or axes.ndim != 2 or axes.shape[1] < dim:
            raise ValueError(f"{what}: origin and axes need {dim} components")
        if len(axes) != len(shape):
            raise ValueError(f"{what}: {len(axes)} axes but {len(shape)} entries in shape")
        if not 1 <= len(axes) <= 3:
            raise ValueError(f"{what}: one to three axes")
        if min(shape) < 2:
            raise ValueError(f"{what}: at least two points per axis (shape {shape})")
        if not np.all(np.abs(axes[:, :dim]).sum(axis=1) > 0):
            raise ValueError(f"{what}: an axis is the zero vector")
        fields = list(g.get("fields", MERGED_FIELDS))
        bad = [f for f in fields if f not in MERGED_FIELDS]
        if bad or not fields or len(set(fields)) != len(fields):
            raise ValueError(f"{what}: unknown, repeated or no field name(s) {bad or fields}: choose from {list(MERGED_FIELDS)}")
        records = n_steps // interval + 1
        nbytes = 8 * records * len(fields) * int(np.prod(shape))
        if nbytes > MAX_GRID_BYTES:
            raise ValueError(f"{what}: {records} records of {len(fields)} fields on {shape} points take {nbytes} bytes, more than the "
                             f"{MAX_GRID_BYTES} allowed for one grid: raise sample_interval (now {interval}) or coarsen the grid")
        entries.append({"name": name, "origin": origin[:dim] * factor, "axes": axes[:, :dim] * factor, "shape": tuple(shape),
                        "fields": fields, "records": records})
    return entries, interval


class RunOutput:
    """Everything ``SolverKNPEMI`` records besides the solve itself; one instance per solver."""

    def __init__(self, solver):
        self.s = solver
        p = solver.problem
        self.p = p
        self.prefix = p.output_dir
        self.traces = bool(solver.save_pngs or solver.save_dat)
        self.v_t, self.n_t, self.m_t, self.h_t = [], [], [], []
        self.ics_eval = self.ecs_eval = self.gamma_eval = None
        if self.traces or p.point_evaluation:
            os.makedirs(self.prefix, exist_ok=True)
            if not hasattr(p, "png_dof"):
                find_membrane_measurement_vertex(p)
        if p.point_evaluation:                                         # KNPEMIx_solver.py:612-626
            n = solver.time_steps + 1
            self.ics_eval = PointEvaluator(p, p.ics_points, side=0)
            self.ecs_eval = PointEvaluator(p, p.ecs_points, side=1)
            self.gamma_eval = PointEvaluator(p, p.gamma_points, side=None)
            solver.ics_point_values = np.zeros((n, p.num_variables, len(p.ics_points)))
            solver.ecs_point_values = np.zeros((n, p.num_variables, len(p.ecs_points)))
            solver.gamma_point_values = np.zeros((n, len(p.gamma_points)))
        if solver.save_cpoints:
            os.makedirs(os.path.join(self.prefix, "checkpoints"), exist_ok=True)
        # stimulus-current trace (KNPEMIx_solver.py:578-585): the expression as a diagnostic program, integrated over the stimulus
        # membranes on the device into one slot per record; read at export (or every step when the problem prints)
        self.stim = None
        if self.traces and hasattr(p, "stim_ufl_expr"):
            from .diagnostics import membrane_program
            be = solver.backend
            self.stim_spec = membrane_program(p, p.stim_ufl_expr)
            be.set_diag_program(self.stim_spec)
            be.set_facet_groups([p.stimulus_tags])
            self.stim = torch.zeros(solver.time_steps + 1, dtype=torch.float64, device=be.device)
        # ion amounts per cell tag every save_interval steps (output key save_ion_budget), one row of a preallocated device tensor each
        self.budget = None
        if getattr(solver, "save_ion_budget", False):
            os.makedirs(self.prefix, exist_ok=True)
            lay = solver.backend.budget_layout()
            n_rec = solver.time_steps // solver.save_interval + 1
            self.budget = torch.zeros((n_rec, lay.n_tags, 3), dtype=torch.float64, device=solver.backend.device)
        # molar ion fluxes across the membrane-data tag inside the stimulus region at every step (output key save_fluxes): the
        # reference's flux_values[time_steps + 1, 2 N_ions] (KNPEMIx_solver.py:626-627, 641-643), one row of a device tensor per record
        self.fluxes = None
        if getattr(solver, "save_fluxes", False):
            from .fluxes import FluxEvaluator
            os.makedirs(self.prefix, exist_ok=True)
            self.flux_eval = FluxEvaluator(p, [p.membrane_data_tag], mask=True)
            self.fluxes = torch.zeros((solver.time_steps + 1, 2 * p.N_ions), dtype=torch.float64, device=solver.backend.device)
        # membrane potential per membrane tag and at one probe vertex per tag (output key save_membrane_potentials): one row of
        # preallocated device tensors per record, read once in save_membrane_potentials()
        self.phim = None
        if getattr(solver, "membrane_potential_tags", None) is not None:
            os.makedirs(self.prefix, exist_ok=True)
            be = solver.backend
            tags = solver.membrane_potential_tags
            be.set_phim_groups([[t] for t in tags])
            self.phim_lay = be.phim_layout()
            n_rec = solver.time_steps // solver.membrane_potential_interval + 1
            self.phim = torch.zeros((n_rec, len(tags), 3), dtype=torch.float64, device=be.device)
            self.probes = find_membrane_probe_vertices(p, tags)
            self.probe_cols = np.nonzero(self.probes["owner"] == p.comm.rank)[0]
            self.probe_idx = torch.as_tensor(self.probes["vertex"][self.probe_cols], dtype=torch.int64, device=be.device)
            self.probe_fields = [p.phi_m_prev] + ([p.n, p.m, p.h] if hasattr(p, "n") else [])
            self.probe_rows = torch.zeros((len(self.probe_fields), n_rec, len(self.probe_cols)), dtype=torch.float64, device=be.device)
        # activation map (output key save_activation): armed here, on the state that record 0 sees, then one detector launch per
        # record; read once in save_activation()
        self.activation = None
        if getattr(solver, "save_activation", None) is not None:
            from .activation import ActivationMap
            os.makedirs(self.prefix, exist_ok=True)
            self.activation = ActivationMap(p, **solver.save_activation)
        # fields on grids and slices (output key sample_grids): per entry one located GridSampler and one preallocated device tensor
        # [records, fields, *shape]; a record is one gather launch, the tensors are read once in save_sample_grids()
        self.grids = []
        for g in getattr(solver, "sample_grids", None) or []:
            from .sampling import GridSampler, merged_functions
            os.makedirs(self.prefix, exist_ok=True)
            gs = GridSampler(p, g["origin"], g["axes"], g["shape"])
            _, f_i, f_e = merged_functions(p, g["fields"])
            buf = torch.zeros((g["records"], len(f_i)) + gs.shape, dtype=torch.float64, device=solver.backend.device)
            self.grids.append({"name": g["name"], "sampler": gs, "f_i": f_i, "f_e": f_e, "buf": buf, "t": []})
        # surfaces (output key clip_surfaces, SolverKNPEMI.add_surface): per surface one built plan and one preallocated device tensor
        # [records, fields, vertices]; a record is one gather launch, the tensors are read once in save_surfaces()
        self.surfaces = []
        if getattr(solver, "clip_surfaces", None) or getattr(solver, "surfaces", None):
            from .surfaces import ClipSurface, SurfaceRecorder, named_functions
            for g in solver.clip_surfaces:
                S = ClipSurface(p, g["tags"], g["side"], g["origin"], g["normal"], g["boundary"])
                self.surfaces.append(SurfaceRecorder(g["name"], S, *named_functions(p, g["fields"]), solver.surface_interval, solver.time_steps,
                                                     self.prefix))
            for name, S, fields, interval in solver.surfaces:
                self.surfaces.append(SurfaceRecorder(name, S, *named_functions(p, fields), interval, solver.time_steps, self.prefix))
        # volume functionals (SolverKNPEMI.add_functional): one row of a preallocated device tensor per record, read once in
        # save_functionals()
        self.functionals = []
        for name, F, interval in getattr(solver, "functionals", None) or []:
            os.makedirs(self.prefix, exist_ok=True)
            buf = torch.zeros((solver.time_steps // interval + 1, len(F.tags), F.n_out), dtype=torch.float64, device=solver.backend.device)
            self.functionals.append({"name": name, "F": F, "interval": interval, "buf": buf})
        # fields of user expressions (SolverKNPEMI.add_field): fields.xdmf / fields.h5, a pair of its own next to solution.*
        self.fields, self.fields_writer = list(getattr(solver, "fields", None) or []), None
        if self.fields:
            from .fields import FieldsWriter, writer_entry
            os.makedirs(self.prefix, exist_ok=True)
            lm = p.local_mesh
            xname, hname = self._xdmf_names("fields")
            self.fields_writer = FieldsWriter(xname, hname, lm.coords, np.asarray(lm.cells)[:int(lm.n_cells_owned)],
                                              [writer_entry(name, F, nodal) for name, F, _, nodal in self.fields])
        self.xdmf = None
        if getattr(solver, "save_xdmfs", False):
            os.makedirs(self.prefix, exist_ok=True)
            self.init_xdmf_savefile()

    # ---- KNPEMIx_solver.py:551-610
    def _trace_point(self):
        p = self.p
        if p.comm.rank != p.owner_rank_membrane_vertex:
            return
        d = p.png_dof
        self.v_t.append(1000.0 * float(p.phi_m_prev.x.array[d]))       # mV
        if hasattr(p, "n"):
            self.n_t.append(float(p.n.x.array[d]))
            self.m_t.append(float(p.m.x.array[d]))
            self.h_t.append(float(p.h.x.array[d]))

    def record(self, i):
        """state after timestep i (i = 0: initial data)"""
        s, p = self.s, self.p
        if self.traces:
            self._trace_point()
        if p.point_evaluation:                                         # KNPEMIx_solver.py:628-643
            s.ics_point_values[i] = self.ics_eval(p.wh[0])
            s.ecs_point_values[i] = self.ecs_eval(p.wh[1])
            s.gamma_point_values[i] = self.gamma_eval([p.phi_m_prev])[0]
        if self.stim is not None:                                      # KNPEMIx_solver.py:580-582, 604-610
            be = s.backend
            be.refresh_diag_constants(self.stim_spec)
            be.membrane_integral(self.stim[i:i + 1])
            if i > 0 and not getattr(p, "quiet", False):               # a read-back: only where the step timers are read anyway
                p.print(f"Total stimulus current: {p.comm.allreduce_sum(float(self.stim[i])):.2e}")
        if self.fluxes is not None:
            self.flux_eval.enqueue(self.fluxes[i])
        if self.budget is not None and (i % s.save_interval == 0):
            s.backend.ion_amounts(self.budget[i // s.save_interval])
        if self.phim is not None and (i % s.membrane_potential_interval == 0):
            r = i // s.membrane_potential_interval
            if s.backend.phim_layout() is not self.phim_lay:           # a membrane_potential(tags=...) call in between replaced the map
                s.backend.set_phim_groups(self.phim_lay.groups)
                self.phim_lay = s.backend.phim_layout()
            s.backend.membrane_potential(out=self.phim[r])
            if len(self.probe_cols):
                for k, fn in enumerate(self.probe_fields):
                    torch.index_select(fn.x.array, 0, self.probe_idx, out=self.probe_rows[k, r])
        if self.activation is not None and i > 0:
            self.activation.update()
        if self.grids and (i % s.sample_interval == 0):
            for g in self.grids:
                g["sampler"](g["f_i"], g["f_e"], out=g["buf"][i // s.sample_interval])
                g["t"].append(float(p.t.value))
        for g in self.functionals:
            if i % g["interval"] == 0:
                g["F"](out=g["buf"][i // g["interval"]])
        for r in self.surfaces:
            r.record(i, float(p.t.value))
        if self.fields_writer is not None:
            from .fields import record_arrays
            self.fields_writer.write(float(p.t.value), {name: record_arrays(F, nodal) for name, F, interval, nodal in self.fields
                                                        if i % interval == 0})
        if s.save_cpoints and (i % s.save_interval == 0):
            self.checkpoint(i)
        if self.xdmf is not None and i > 0 and (i % s.save_interval == 0):       # reference :471
            self.save_xdmf()

    # ---- KNPEMIx_solver.py:766-797, 824-831: subdomains.xdmf (mesh + cell tags) and solution.xdmf (time series of the 2(N+1)
    # nodal functions), heavy data in .h5 files next to them (cgx_hip/hdf5_write.py); one pair of files per rank
    def _xdmf_names(self, stem):
        p = self.p
        sfx = f"_rank{p.comm.rank}" if p.comm.size > 1 else ""
        return os.path.join(self.prefix, stem + sfx + ".xdmf"), os.path.join(self.prefix, stem + sfx + ".h5")

    def _mesh_items(self, h5name, n_cells, n_pts, dim):
        ttype = "Triangle" if dim == 2 else "Tetrahedron"
        return [f'      <Topology TopologyType="{ttype}" NumberOfElements="{n_cells}" NodesPerElement="{dim + 1}">',
                f'        <DataItem Dimensions="{n_cells} {dim + 1}" NumberType="Int" Precision="8" Format="HDF">{h5name}:/Mesh/mesh/topology</DataItem>',
                f'      </Topology>',
                f'      <Geometry GeometryType="{"XY" if dim == 2 else "XYZ"}">',
                f'        <DataItem Dimensions="{n_pts} {dim}" NumberType="Float" Precision="8" Format="HDF">{h5name}:/Mesh/mesh/geometry</DataItem>',
                f'      </Geometry>']

    def _tag_grid(self, h5name, n_cells, n_pts, dim):
        return ['    <Grid Name="ct" GridType="Uniform">'] + self._mesh_items(h5name, n_cells, n_pts, dim)[:3] + [
            f'      <Geometry GeometryType="{"XY" if dim == 2 else "XYZ"}">',
            f'        <DataItem Dimensions="{n_pts} {dim}" NumberType="Float" Precision="8" Format="HDF">{h5name}:/Mesh/mesh/geometry</DataItem>',
            f'      </Geometry>',
            f'      <Attribute Name="ct" AttributeType="Scalar" Center="Cell">',
            f'        <DataItem Dimensions="{n_cells} 1" NumberType="Int" Precision="4" Format="HDF">{h5name}:/MeshTags/ct/Values</DataItem>',
            f'      </Attribute>',
            f'    </Grid>']

    @staticmethod
    def _xdmf_text(body):
        return "\n".join(['<?xml version="1.0"?>', '<!DOCTYPE Xdmf SYSTEM "Xdmf.dtd" []>', '<Xdmf Version="3.0">', '  <Domain>'] + body + ['  </Domain>', '</Xdmf>', ''])

    def init_xdmf_savefile(self):
        from .hdf5_write import Hdf5Writer
        p = self.p
        lm = p.local_mesh
        coords = np.asarray(lm.coords, dtype=np.float64)
        cells = np.asarray(lm.cells, dtype=np.int64)
        tags = np.asarray(lm.cell_tags, dtype=np.int32).reshape(-1, 1)
        dim = cells.shape[1] - 1
        nc, npt = len(cells), len(coords)
        for stem in ("subdomains", "solution"):
            xname, hname = self._xdmf_names(stem)
            w = Hdf5Writer(hname)
            w.write("/Mesh/mesh/geometry", coords)
            w.write("/Mesh/mesh/topology", cells)
            w.write("/MeshTags/ct/topology", cells)
            w.write("/MeshTags/ct/Values", tags)
            base = os.path.basename(hname)
            head = ['    <Grid Name="mesh" GridType="Uniform">'] + self._mesh_items(base, nc, npt, dim) + ['    </Grid>'] + self._tag_grid(base, nc, npt, dim)
            if stem == "subdomains":
                w.close()
                with open(xname, "w") as f:
                    f.write(self._xdmf_text(head))
            else:
                self.xdmf = {"writer": w, "xname": xname, "h5": base, "head": head, "steps": [], "dims": (nc, npt, dim)}
        self.save_xdmf()                               # initial state, reference :787-790

    def save_xdmf(self):
        """the 2(N+1) solution functions at the current time (reference :792-797), appended to solution.h5"""
        if self.xdmf is None:
            return
        p = self.p
        X = self.xdmf
        k = len(X["steps"])
        names = []
        for idx in range(p.num_variables):
            for side in (0, 1):
                f = p.wh[side][idx]
                X["writer"].write(f"/Function/{f.name}/{k}", np.asarray(f.numpy(), dtype=np.float64).reshape(-1, 1))
                names.append(f.name)
        X["steps"].append((float(p.t.value), names))
        self._write_solution_xml()

    _XML_TAIL = ['    </Grid>', '  </Domain>', '</Xdmf>', '']

    def _write_solution_xml(self):
        """solution.xdmf is always a complete document: the text of the steps not yet written is put where the closing tags of
        the previous version began, followed by the closing tags again -- O(steps) text in total (regenerating the
        whole file at every save was O(steps^2))."""
        X = self.xdmf
        nc, npt, dim = X["dims"]
        if "xml_pos" not in X:
            head = self._xdmf_text(list(X["head"]) + ['    <Grid Name="solution" GridType="Collection" CollectionType="Temporal">'])
            head = head[:head.index("  </Domain>")]
            with open(X["xname"], "w") as f:
                f.write(head)
                X["xml_pos"] = f.tell()
                f.write("\n".join(self._XML_TAIL))
            X["xml_steps"] = 0
        body = []
        for k in range(X["xml_steps"], len(X["steps"])):
            t, names = X["steps"][k]
            body += [f'      <Grid Name="step_{k}" GridType="Uniform">', f'        <Time Value="{t!r}" />']
            body += ["  " + ln for ln in self._mesh_items(X["h5"], nc, npt, dim)]
            for nm in names:
                body += [f'        <Attribute Name="{nm}" AttributeType="Scalar" Center="Node">',
                         f'          <DataItem Dimensions="{npt} 1" NumberType="Float" Precision="8" Format="HDF">{X["h5"]}:/Function/{nm}/{k}</DataItem>',
                         f'        </Attribute>']
            body += ['      </Grid>']
        if not body:
            return
        with open(X["xname"], "r+") as f:
            f.seek(X["xml_pos"])
            f.write("\n".join(body) + "\n")
            X["xml_pos"] = f.tell()
            f.write("\n".join(self._XML_TAIL))
            f.truncate()
        X["xml_steps"] = len(X["steps"])

    def close_xdmf(self):
        if self.xdmf is not None:
            self.xdmf["writer"].close()                # the .h5 file becomes readable here (metadata + superblock)
            self._write_solution_xml()
            self.p.print("\nXDMF output saved in ", self.prefix)
            self.xdmf = None

    def close_fields(self):
        if self.fields_writer is not None:
            self.fields_writer.close()                 # the .h5 file becomes readable here; fields.xdmf is complete after every record
            self.fields_writer = None

    def checkpoint(self, i):
        """nodal values of the 2(N+1) solution functions (+ phi_m and the gating variables) of this rank's owned vertices"""
        p = self.p
        lm = p.local_mesh
        nvo = lm.n_vertices_owned
        data = {"t": float(p.t.value), "step": i, "l2g": lm.l2g[:nvo], "coords": lm.coords[:nvo]}
        for f in p.u_out_i + p.u_out_e:
            data[f.name] = f.numpy()[:nvo]
        data["phi_m"] = p.phi_m_prev.numpy()[:nvo]
        for nm in ("n", "m", "h"):
            if hasattr(p, nm):
                data[nm] = getattr(p, nm).numpy()[:nvo]
        for st in getattr(p, "state_variables", []):
            data[st.name] = st.function.numpy()[:nvo]
        np.savez(os.path.join(self.prefix, "checkpoints", f"step_{i:06d}_rank{p.comm.rank}.npz"), **data)

    # ---- KNPEMIx_solver.py:833-866 (same file names)
    def export(self):
        s, p = self.s, self.p
        out = p.output_dir
        if self.traces and p.comm.rank == p.owner_rank_membrane_vertex:
            np.save(out + "phi_m.npy", np.array(self.v_t))
            if hasattr(p, "n"):
                np.save(out + "n.npy", np.array(self.n_t))
                np.save(out + "m.npy", np.array(self.m_t))
                np.save(out + "h.npy", np.array(self.h_t))
        if p.comm.rank == 0:
            if p.point_evaluation:
                np.save(out + "gamma_point_values.npy", s.gamma_point_values)
                np.save(out + "ics_point_values.npy", s.ics_point_values)
                np.save(out + "ecs_point_values.npy", s.ecs_point_values)
            np.save(out + "assembly_time.npy", np.array(s.assembly_time))
            np.save(out + "solve_time.npy", np.array(s.solve_time))
            if not s.direct_solver:
                np.save(out + "iterations.npy", np.array(s.iterations))
        if self.stim is not None:                                      # KNPEMIx_solver.py:855-857
            stim = self._sum_ranks(self.stim.cpu().numpy())
            if p.comm.rank == 0:
                np.save(out + "stimulus.npy", stim)

    def _sum_ranks(self, a):
        """a summed over the ranks in rank order (the same bits for the same rank count)"""
        if self.p.comm.size == 1:
            return a
        return np.sum(self.p.comm.all_gather_object(a), axis=0)

    def save_ion_budget(self):
        """ion_budget.npy: [records, cell tags, (Na, K, Cl)] in mol at steps 0, save_interval, 2 save_interval, ...;
        ion_budget_tags.npy: per cell tag (tag, side 0 intra / 1 extra, volume [m^3], membrane area [m^2]).  One read-back."""
        p = self.p
        lay = self.s.backend.budget_layout()
        data = self._sum_ranks(self.budget.cpu().numpy())
        vol, area = self._sum_ranks(lay.volume), self._sum_ranks(lay.area)
        if p.comm.rank == 0:
            np.save(p.output_dir + "ion_budget.npy", data)
            np.save(p.output_dir + "ion_budget_tags.npy", np.stack([lay.tags, lay.side, vol, area], axis=1).astype(np.float64))

    def save_fluxes(self):
        """fluxes.npy: [time_steps + 1, (Na, K, Cl out of the intracellular side, Na, K, Cl out of the extracellular side)] in mol/s
        through the membrane-data tag inside the stimulus region, state after step i in row i.  One read-back."""
        data = self._sum_ranks(self.fluxes.cpu().numpy())
        if self.p.comm.rank == 0:
            np.save(self.p.output_dir + "fluxes.npy", data)

    def save_membrane_potentials(self):
        """phi_m_tags.npy: [records, tags, (mean, min, max)] in V at steps 0, interval, 2 interval, ...; phi_m_tags_index.npy: per tag
        (tag, area [m^(d-1)]); phi_m_points.npy: [records, tags] phi_m in V at each tag's probe vertex
        (``find_membrane_probe_vertices``), phi_m_points_xyz.npy: [tags, dim] its coordinates in m; gating_points.npy: [records, tags,
        (n, m, h)] there when the problem has gating variables.  A tag no facet carries has area 0 and NaN values.  One read-back."""
        from .diagnostics import reduce_membrane_potential
        p = self.p
        lay = self.phim_lay
        mine = (self.phim.cpu().numpy(), lay.area, self.probe_cols, self.probe_rows.cpu().numpy())
        parts = p.comm.all_gather_object(mine) if p.comm.size > 1 else [mine]
        if p.comm.rank != 0:
            return
        area, val = reduce_membrane_potential([q[0] for q in parts], [q[1] for q in parts])
        pts = np.full((len(self.probe_fields), self.phim.shape[0], len(lay.tags)), np.nan)
        for _, _, cols, rows in parts:
            pts[:, :, cols] = rows
        out = p.output_dir
        np.save(out + "phi_m_tags.npy", val)
        np.save(out + "phi_m_tags_index.npy", np.stack([lay.tags.astype(np.float64), area], axis=1))
        np.save(out + "phi_m_points.npy", pts[0])
        np.save(out + "phi_m_points_xyz.npy", self.probes["xyz"])
        if len(self.probe_fields) == 4:
            np.save(out + "gating_points.npy", np.ascontiguousarray(np.transpose(pts[1:], (1, 2, 0))))

    def save_activation(self):
        """the six activation*.npy files of ``ActivationMap.save``"""
        self.activation.save(self.p.output_dir)

    def save_sample_grids(self):
        """Per ``sample_grids`` entry: grid_<name>.npy [records, fields, *shape] (the merged fields: the _i function inside intracellular
        cells, the _e function inside extracellular ones, NaN outside the mesh) at steps 0, sample_interval, 2 sample_interval, ...;
        grid_<name>_tags.npy int32 [*shape], the cell tag per point, -1 outside; grid_<name>_xyz.npy [*shape, dim] in metres;
        grid_<name>_t.npy the recorded times [s].  One read-back per grid."""
        out = self.p.output_dir
        for g in self.grids:
            gs = g["sampler"]
            np.save(out + f"grid_{g['name']}.npy", g["buf"][:len(g["t"])].cpu().numpy())
            np.save(out + f"grid_{g['name']}_tags.npy", np.ascontiguousarray(gs.cell_tag, dtype=np.int32))
            np.save(out + f"grid_{g['name']}_xyz.npy", gs.xyz)
            np.save(out + f"grid_{g['name']}_t.npy", np.array(g["t"]))

    def save_surfaces(self):
        """surface_<name>.xdmf / .h5 per recorded surface (one read-back each; a second call writes nothing)"""
        for r in self.surfaces:
            r.save()

    def save_functionals(self):
        """Per ``add_functional`` entry: functional_<name>.npy [records, n_tags, n_out] at steps 0, interval, 2 interval, ...;
        functional_<name>_tags.npy: per row (tag, side 0 intra / 1 extra, volume), for a membrane functional (the row's first tag,
        side 2, area).  One read-back per functional."""
        out = self.p.output_dir
        for g in self.functionals:
            F = g["F"]
            np.save(out + f"functional_{g['name']}.npy", g["buf"].cpu().numpy())
            rows = [F.tags, F.side, F.volume] if hasattr(F, "side") else [F.tags, np.full(len(F.tags), 2), F.area]
            np.save(out + f"functional_{g['name']}_tags.npy", np.stack(rows, axis=1).astype(np.float64))

    def figures(self):
        """PNG plots of the traces (KNPEMIx_solver.py:645-764) when matplotlib is installed; the data are exported either way."""
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except Exception:      # noqa: BLE001
            self.p.print("matplotlib is not installed: PNG figures skipped, traces are in the .npy files")
            return
        s, p = self.s, self.p
        times = np.linspace(0, 1000 * s.time_steps * float(p.dt.value), s.time_steps + 1)
        if p.comm.rank == p.owner_rank_membrane_vertex and self.v_t:
            fig, ax = plt.subplots()
            ax.plot(times[:len(self.v_t)], np.array(self.v_t))
            ax.set_xlabel("Time [ms]"); ax.set_ylabel("Membrane potential [mV]")
            fig.savefig(self.prefix + "v.png")
            if self.n_t:
                fig, ax = plt.subplots()
                for arr, lab in ((self.n_t, "n"), (self.m_t, "m"), (self.h_t, "h")):
                    ax.plot(times[:len(arr)], np.array(arr), label=lab)
                ax.set_xlabel("Time [ms]"); ax.legend()
                fig.savefig(self.prefix + "gating.png")
        if p.comm.rank == 0:
            fig, ax = plt.subplots()
            ax.plot(s.assembly_time, label="assembly"); ax.plot(s.solve_time, label="solve")
            ax.set_xlabel("Timestep"); ax.set_ylabel("Time [s]"); ax.legend()
            fig.savefig(self.prefix + "timings.png")
            if not s.direct_solver:
                fig, ax = plt.subplots()
                ax.plot(s.iterations); ax.set_xlabel("Timestep"); ax.set_ylabel("Number of iterations")
                fig.savefig(self.prefix + "iterations.png")
