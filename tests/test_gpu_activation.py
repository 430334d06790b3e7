"""The activation map on the device (csrc/knp_activation.inc, cgx_hip/activation.py, output key ``save_activation``) against the
independent NumPy restatement of tests/activation_ref.py, on the meshes of tests/test_gpu_membrane_potential.py and one Delaunay
mesh of tests/irregular_meshes.py.

Tolerances (derived in tests/activation_ref.py): counts, peaks, peak times, the record of the steepest upstroke and every NaN pattern
are selections and equal the reference exactly; an interpolated time agrees within 8 * 2^-52 * max(|t1|, h) of its interval, a slope
within 4 * 2^-52 |s|; |g|^2 and the components of g within 1e-12 of their un-cancelled sums; area sums within 1e-12 of the sum (all
terms positive), the speed sum within 1e-12 of sum |F| speed (1 + gg_unc / (2 gg)); minima and maxima exactly."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import irregular_meshes as IM
from activation_ref import EPS, TOL, detector_ref, summary_ref, time_tol, velocity_ref
from parity_utils import ci_config, make_problem, tissue_config
from phim_ref import facet_vertices

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -3          # KNP_E_ARG, KNP_E_STATE of include/knpemi_hip.h
CASES = ["square16", "cube8", "tissue2d", "tissue3d_12_2", "delaunay3d_7"]
FACETS = {"square16": [32], "cube8": [192], "tissue2d": [16] * 9, "tissue3d_12_2": [192] * 8}
THR, THR_DOWN = 0.01, -0.005
FILES = ("activation.npy", "activation_vertices.npy", "activation_xyz.npy", "activation_velocity.npy", "activation_facets.npy",
         "activation_tags.npy")


def _write(fn, values):
    fn.x.array.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(fn.x.array.device))


def _problem(case, tmp_path):
    if case == "square16":
        cfg = ci_config(N=16, steps=1)
    elif case == "cube8":
        cfg = ci_config(N=8, steps=1, kind="cube")
    elif case == "tissue2d":
        cfg = tissue_config(2, 18, 3, steps=1)
    elif case == "tissue3d_12_2":
        cfg = tissue_config(3, 12, 2, steps=1)
    else:
        cfg = IM.config(tmp_path, case)
    p = make_problem(cfg, "ci")
    p.create_backend()
    return p


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- 1. the detector on traces the test writes ---------------------------------------------------------------------------------
def _traces(n, seed):
    """13 records at non-uniform times: random walks around the threshold, and in the first seven columns one trace per category"""
    rng = np.random.default_rng(seed)
    R = 13
    times = 0.002 + np.cumsum(rng.uniform(2e-5, 3e-4, R))
    tr = -0.02 + np.cumsum(rng.normal(0.0, 0.012, (R, n)), axis=0)
    ramp = np.linspace(-0.05, 0.045, R)                                              # passes THR between records 7 and 8
    tr[:, 0] = -0.06 + 0.001 * rng.uniform(size=R)                                   # never crossing
    tr[:, 1] = ramp                                                                  # crossing once, staying up
    tr[:, 2] = np.where((np.arange(R) // 2) % 2 == 0, -0.02, 0.03)                   # up at records 2, 6, 10: three crossings
    tr[:, 3] = ramp
    tr[7, 3] = THR                                                                   # landing exactly on the threshold
    tr[:7, 3] = np.minimum(tr[:7, 3], THR - 1e-3)
    tr[:, 4] = THR + np.linspace(0.0, 0.02, R)                                       # starting exactly on it, rising: no crossing
    tr[:, 5] = np.concatenate([np.linspace(-0.05, 0.03, 6), np.linspace(0.02, -0.04, R - 6)])      # up, then down through THR_DOWN
    tr[:, 6] = ramp
    tr[5, 6] = np.nan                                                                # a NaN at one vertex for one record
    return times, tr


@pytest.mark.parametrize("case", CASES)
def test_detector_matches_the_reference(case, tmp_path):
    from cgx_hip.activation import ActivationMap, RESULT_COLUMNS
    p = _problem(case, tmp_path)
    amap = ActivationMap(p, THR, THR_DOWN)
    n = len(amap.vertices)
    fv = facet_vertices(p)
    assert np.array_equal(amap.vertices, np.unique(fv)) and np.array_equal(np.sort(amap.facet_vertices, axis=1), np.sort(fv[amap.facets], axis=1))
    if case in FACETS:
        assert [int((amap.facet_tag == t).sum()) for t in amap.tags] == FACETS[case]
    if case == "tissue3d_12_2":
        assert n > 256 and n % 256 != 0                         # more than one block of the detector, with a ragged tail
    times, tr = _traces(n, 5)
    ref = detector_ref(tr, times, THR, THR_DOWN)
    # every category is there, by construction: checked on the reference before the GPU is asked
    c = ref["count"]
    assert c[0] == 0 and c[1] == 1 and c[2] == 3 and c[3] == 1 and ref["k_act"][3] == 7 and tr[7, 3] == THR and c[4] == 0 and tr[0, 4] == THR
    assert c[5] == 1 and np.isfinite(ref["t_repol"][5]) and np.isnan(tr[5, 6]) and c[6] == 1 and ref["k_act"][6] > 6
    assert (c == 0).any() and (c == 1).any() and (c >= 3).any() and np.isfinite(ref["t_repol"]).any() and np.isnan(ref["t_repol"][c > 0]).any()
    rng = np.random.default_rng(9)
    nv = p.local_mesh.coords.shape[0]

    def run():
        for k in range(len(times)):
            phi = rng.uniform(-0.1, 0.1, nv)                    # the vertices off the list hold anything
            phi[amap.vertices] = tr[k]
            _write(p.phi_m_prev, phi)
            p.t.value = float(times[k])
            if k == 0:
                amap.arm()
            else:
                amap.update()
                amap.update()                                   # at an unchanged time: nothing
        return amap.result()
    got = run()
    assert list(got) == list(RESULT_COLUMNS) and got["count"].dtype == np.int64
    assert np.array_equal(got["count"], ref["count"])
    for key in RESULT_COLUMNS[:-1]:
        assert np.array_equal(np.isnan(got[key]), np.isnan(ref[key])), key
    assert _bits(got["v_peak"]) == _bits(ref["v_peak"]) and _bits(got["t_peak"]) == _bits(ref["t_peak"])
    h = np.diff(times)
    worst = 0.0
    for key, rec in (("t_act", "k_act"), ("t_last", "k_last"), ("t_repol", "k_repol"), ("t_dvdt", "k_dvdt")):
        for j in np.nonzero(ref[rec] >= 0)[0]:
            k = ref[rec][j]
            tol = time_tol(times[k], h[k - 1])
            err = abs(got[key][j] - ref[key][j])
            worst = max(worst, err / tol)
            assert err <= tol, (key, j, got[key][j], ref[key][j])
    # the record of the steepest upstroke: the interval whose middle the recorded time is
    mid = times[:-1] + 0.5 * h
    has = ref["k_dvdt"] >= 0
    assert np.array_equal(np.argmin(np.abs(got["t_dvdt"][has, None] - mid[None, :]), axis=1) + 1, ref["k_dvdt"][has])
    err = np.abs(got["dvdt_max"][has] - ref["dvdt_max"][has])
    assert np.all(err <= 4.0 * EPS * np.abs(ref["dvdt_max"][has]))
    assert np.array_equal(got["dvdt_max"][~has], ref["dvdt_max"][~has])
    assert _bits(got["apd"]) == _bits(got["t_repol"] - got["t_act"])
    print(f"{case}: {n} vertices; largest time error / bound = {worst:.3f}; largest slope error / |s| = "
          f"{float(np.max(err / np.abs(ref['dvdt_max'][has]))) / EPS:.2f} ulp")
    # the same sequence again: the same bytes
    state, count = _bits(amap.state.cpu().numpy()), _bits(amap.count.cpu().numpy())
    rng = np.random.default_rng(9)
    run()
    assert _bits(amap.state.cpu().numpy()) == state and _bits(amap.count.cpu().numpy()) == count
    # arm() restores the armed state at the current time and phi_m
    amap.arm()
    st, now = amap.state.cpu().numpy(), p.phi_m_prev.numpy()[amap.vertices]
    assert np.isnan(st[[0, 1, 2, 6]]).all() and _bits(st[3]) == _bits(now) and np.all(st[4] == times[-1]) and np.all(st[5] == -np.inf)
    assert not amap.count.cpu().numpy().any() and _bits(amap.v_last.cpu().numpy()) == _bits(now)
    # the nodal functions: NaN away from the listed membranes
    amap.update()
    fns = amap.functions()
    off = np.setdiff1d(np.arange(nv), amap.vertices)
    assert sorted(fns) == ["activation_time", "peak", "repolarisation_time"]
    assert np.isnan(fns["peak"].numpy()[off]).all() and _bits(fns["peak"].numpy()[amap.vertices]) == _bits(now)


# ---- 2. velocity and the rows per group ----------------------------------------------------------------------------------------
def _time_field(p, amap, seed, blank_tag=None):
    """a plane wave plus a quadratic term over the mesh's extent, NaN on a random 10 % of the membrane vertices and on every vertex
    of the facets tagged ``blank_tag``"""
    rng = np.random.default_rng(seed)
    X = np.asarray(p.local_mesh.coords, dtype=np.float64)
    lo, span = X.min(axis=0), float((X.max(axis=0) - X.min(axis=0)).max())
    U = (X - lo) / span
    k = rng.uniform(0.5, 1.5, X.shape[1]) * 1e-3
    T = 2e-3 + U @ k + 4e-4 * (U[:, 0] - 0.3) ** 2 - 3e-4 * U[:, 0] * U[:, -1]
    T[rng.choice(amap.vertices, max(1, len(amap.vertices) // 10), replace=False)] = np.nan
    if blank_tag is not None:
        T[np.unique(amap.facet_vertices[amap.facet_tag == blank_tag])] = np.nan
    return T


@pytest.mark.parametrize("case", CASES)
def test_velocity_and_group_rows_match_the_reference(case, tmp_path):
    from cgx_hip.activation import ActivationMap
    p = _problem(case, tmp_path)
    amap = ActivationMap(p, THR)
    tags = list(amap.tags)
    dim = amap.dim
    blank = tags[1] if len(tags) >= 3 else None
    T = _time_field(p, amap, 21, blank)
    Td = torch.from_numpy(T).to(amap.state.device)
    X = np.asarray(p.local_mesh.coords, dtype=np.float64)
    fv = facet_vertices(p)
    ref = velocity_ref(X, fv[amap.facets], T)
    assert ref["valid"].any() and not ref["valid"].all()
    vel = amap.velocity(Td).cpu().numpy()
    assert vel.shape == (len(amap.facets), 1 + dim)
    ok = ref["valid"]
    assert np.array_equal(~np.isnan(vel[:, 0]), ok) and np.isnan(vel[~ok]).all() and np.isfinite(vel[ok]).all()
    gg = 1.0 / vel[ok, 0] ** 2
    r_gg = np.abs(gg - ref["gg"][ok]) / ref["gg_unc"][ok]
    g = vel[ok, 1:] / vel[ok, :1]
    r_g = np.abs(g - ref["g"][ok]) / np.maximum(ref["g_unc"][ok], 1e-300)
    print(f"{case}: {int(ok.sum())} of {len(ok)} facets valid; max | |g|^2 - ref | / un-cancelled = {r_gg.max():.3e}, components of g: {r_g.max():.3e}")
    assert np.all(r_gg <= TOL) and np.all(r_g <= TOL)
    assert np.all(np.abs(np.linalg.norm(vel[ok, 1:], axis=1) - 1.0) <= 1e-12)
    assert np.all(np.sum(vel[ok, 1:] * ref["direction"][ok], axis=1) > 0.0)
    assert _bits(amap.velocity(Td).cpu().numpy()) == _bits(vel)

    def check(groups, what):
        rows, cover, meas, S1 = summary_ref(X, fv, p.local_mesh.gamma_tags, T, groups)
        got, lay = amap.summary(groups, Td)
        got = got.cpu().numpy()
        assert got.shape == (len(groups), 5) and np.allclose(lay.area, [meas[c].sum() for c in cover], rtol=1e-13, atol=0)
        assert np.array_equal(got[:, 2], rows[:, 2]) and np.array_equal(got[:, 3], rows[:, 3]), what
        for col, S in ((0, rows[:, 0]), (1, S1), (4, rows[:, 4])):
            err = np.abs(got[:, col] - rows[:, col])
            print(f"{case} {what}: column {col} max error / scale = {float(np.max(err / np.maximum(S, 1e-300))):.3e}")
            assert np.all(err <= TOL * S), (what, col)
        assert _bits(amap.summary(groups, Td)[0].cpu().numpy()) == _bits(got)
        return got, rows, cover
    got, rows, cover = check([[t] for t in tags], "per tag")
    if blank is not None:                                        # a group whose vertices all carry NaN
        assert list(got[1]) == [0.0, 0.0, np.inf, -np.inf, 0.0] and len(cover[1]) > 0
    # pooled groups, an empty group in the middle, a tag that no facet carries
    groups = [tags[:2], [987654], tags[2:]] if len(tags) >= 3 else [[987654], tags, [424242]]
    got, rows, cover = check(groups, "pooled")
    empty = [t for t, c in enumerate(cover) if len(c) == 0]
    assert empty == ([1] if len(tags) >= 3 else [0, 2])
    for t in empty:
        assert list(got[t]) == [0.0, 0.0, np.inf, -np.inf, 0.0]
    # every time NaN: every group gives the identity, every facet is invalid
    none = torch.full_like(Td, float("nan"))
    got, _ = amap.summary(groups, none)
    assert np.array_equal(got.cpu().numpy(), np.tile([0.0, 0.0, np.inf, -np.inf, 0.0], (len(groups), 1)))
    assert np.isnan(amap.velocity(none).cpu().numpy()).all()
    # per_tag() of the map's own state (armed, nothing fired): NaN where a group has nothing
    out = amap.per_tag(groups)
    assert list(out["tag"]) == [g[0] for g in groups] and np.isnan(out["t_first"]).all() and np.isnan(out["mean_speed"]).all()
    assert np.all(out["area"][empty] == 0.0) and not out["valid_area"].any() and not out["activated_area"].any()


def test_two_maps_on_one_problem_alternate(tmp_path):
    """The summary's facet map lives in the context, one per problem: maps with different thresholds, tags and group counts take
    turns, and every call reduces its own times over its own groups into a tensor of its own size."""
    from cgx_hip.activation import ActivationMap
    p = _problem("tissue2d", tmp_path)
    tags = [int(t) for t in p.gamma_tags]
    A, B = ActivationMap(p, THR), ActivationMap(p, -0.03, tags=tags[2:6])
    assert len(A.vertices) > len(B.vertices) > 0
    X, fv, ftags = np.asarray(p.local_mesh.coords, dtype=np.float64), facet_vertices(p), p.local_mesh.gamma_tags
    nv = X.shape[0]
    rng = np.random.default_rng(3)
    times = 0.001 + np.cumsum(rng.uniform(1e-5, 1e-4, 6))
    phis = -0.05 + np.cumsum(rng.normal(0.004, 0.012, (6, nv)), axis=0)
    for k in range(6):
        _write(p.phi_m_prev, phis[k])
        p.t.value = float(times[k])
        for m in (A, B):
            m.arm() if k == 0 else m.update()
    refs = {}
    for name, m in (("A", A), ("B", B)):
        r = m.result()
        ref = detector_ref(phis[:, m.vertices], times, m.threshold)
        assert np.array_equal(r["count"], ref["count"]) and np.array_equal(np.isnan(r["t_act"]), np.isnan(ref["t_act"])) and (r["count"] > 0).any()
        T = np.full(nv, np.nan)
        T[m.vertices] = r["t_act"]
        refs[name] = T
    assert not np.array_equal(np.isnan(refs["A"]), np.isnan(refs["B"]))
    gA, gB = [[t] for t in tags], [tags[2:4], tags[4:6]]                 # nine groups and two

    def check(m, T, groups):
        rows, cover, meas, S1 = summary_ref(X, fv, ftags, T, groups if groups is not None else [[t] for t in m.tags])
        got = m.summary(groups)[0].cpu().numpy()
        assert got.shape == (len(rows), 5)
        assert np.array_equal(got[:, 2], rows[:, 2]) and np.array_equal(got[:, 3], rows[:, 3])
        for col, S in ((0, rows[:, 0]), (1, S1), (4, rows[:, 4])):
            assert np.all(np.abs(got[:, col] - rows[:, col]) <= TOL * S), col
        out = m.per_tag(groups)
        assert out["tag"].shape == (len(rows),) and np.array_equal(out["valid_area"], got[:, 0])
        return got
    first = check(A, refs["A"], gA)
    for _ in range(2):
        check(B, refs["B"], gB)
        assert _bits(check(A, refs["A"], gA)) == _bits(first)           # B's map in between leaves A's rows as they were
    assert p.backend._activation.groups == tuple(tuple(g) for g in gA)
    check(B, refs["B"], None)                                            # B's own default: its four tags
    assert p.backend._activation.n_groups == 4


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------
def _knp_solver(cfg, out_dir, **keys):
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    cfg = copy.deepcopy(cfg)
    cfg["output_dir"] = str(out_dir) + "/"
    cfg["solver"]["output"].update({"save_dat": True, **keys})
    p = make_problem(cfg, "ci")
    p.solver_config["view_ksp"] = False
    return SolverKNPEMI(p, solver_config=p.solver_config)


def _first_crossings(trace, times, thr):
    """``threshold_crossings`` and per column the time bound of its first crossing's interval"""
    from cgx_hip.diagnostics import threshold_crossings
    count, first = threshold_crossings(trace, times, thr)
    up = (trace[:-1] < thr) & (trace[1:] >= thr)
    i = np.argmax(up, axis=0)
    tol = np.array([time_tol(times[k + 1], times[k + 1] - times[k]) for k in i])
    return count, first, tol


def _midpoint_of_the_largest_rise(trace):
    rise = np.diff(trace, axis=0)
    i, j = np.unravel_index(np.nanargmax(rise), rise.shape)
    assert rise[i, j] > 0.0, "phi_m rises nowhere: the run cannot test an upward crossing"
    return 0.5 * (trace[i, j] + trace[i + 1, j])


def _check_files(d, n, n_f, dim, n_tags):
    a = {name: np.load(os.path.join(str(d), name)) for name in FILES}
    assert a["activation.npy"].shape == (n, 9) and a["activation_vertices.npy"].shape == (n,) and a["activation_xyz.npy"].shape == (n, dim)
    assert a["activation_velocity.npy"].shape == (n_f, 1 + dim) and a["activation_facets.npy"].shape == (n_f, dim + 1)
    assert a["activation_tags.npy"].shape == (n_tags, 7)
    return a


# The CI physics' own synaptic conductance (g_syn_bar = 1e-9 S over the 2 um membrane of the 16 x 16 square)
# drives a current hundreds of times below the leak currents (g_leak 0.1 to 0.3 S/m^2): measured on the MI355X, phi_m then only relaxes,
# from -70 mV by 0.58 mV in 20 steps, and its largest
# change in one interval is -2.8e-5 V -- it rises nowhere.  The run below keeps the CI config, Hodgkin-Huxley and its stimulus term
# and gives the stimulus a conductance that depolarises the membrane within the 20 steps; the test still fails if phi_m rises nowhere.
G_SYN_BAR = 2e-5


def test_knpemi_run_records_the_crossings_of_its_own_trace(tmp_path):
    steps = 20
    cfg = ci_config(N=16, steps=steps)
    cfg["stimulus"]["conductance"]["g_syn_bar"] = G_SYN_BAR
    # pass one: phi_m at the membrane vertices after every step
    s = _knp_solver(cfg, tmp_path / "a")
    s.prepare()
    p = s.problem
    verts = np.unique(p._fv)
    trace, times = [p.phi_m_prev.numpy()[verts].copy()], [float(p.t.value)]
    for i in range(1, steps + 1):
        s.step(i)
        trace.append(p.phi_m_prev.numpy()[verts].copy())
        times.append(float(p.t.value))
    s.finish()
    trace, times = np.array(trace), np.array(times)
    # the key off: none of the files, no tensors
    assert (tmp_path / "a" / "phi_m.npy").exists() and not any((tmp_path / "a" / f).exists() for f in FILES)
    assert s.output.activation is None and s.save_activation is None and s.backend._activation is None
    thr = _midpoint_of_the_largest_rise(trace)
    count, first, tol = _first_crossings(trace, times, thr)
    assert count.max() >= 1
    # pass two: the same run with the key
    s2 = _knp_solver(cfg, tmp_path / "b", save_activation={"threshold": float(thr)})
    s2.solve()
    amap = s2.output.activation
    assert np.array_equal(amap.vertices, verts)
    a = _check_files(tmp_path / "b", len(verts), len(p._fv), 2, len(p.gamma_tags))
    act = a["activation.npy"]
    print(f"threshold {thr:.6e} V: {int((count > 0).sum())} of {len(verts)} vertices cross; same trace in both passes: "
          f"{_bits(s2.problem.phi_m_prev.numpy()[verts]) == _bits(trace[-1])}")
    assert np.array_equal(act[:, 8], count) and np.array_equal(np.isnan(act[:, 0]), np.isnan(first))
    hit = count > 0
    assert np.all(np.abs(act[hit, 0] - first[hit]) <= tol[hit])
    ref = detector_ref(trace, times, thr)
    assert _bits(act[:, 4]) == _bits(ref["v_peak"]) and _bits(act[:, 5]) == _bits(ref["t_peak"])
    assert np.array_equal(a["activation_vertices.npy"], verts) and np.array_equal(a["activation_xyz.npy"], p.local_mesh.coords[verts])
    assert np.array_equal(a["activation_facets.npy"][:, :2], amap.facet_vertices) and np.array_equal(a["activation_facets.npy"][:, 2], amap.facet_tag)
    # the velocity and the rows per tag that were written are those of the reference on the recorded activation times
    T = np.full(p.local_mesh.coords.shape[0], np.nan)
    T[verts] = act[:, 0]
    vref = velocity_ref(p.local_mesh.coords, amap.facet_vertices, T)
    vel = a["activation_velocity.npy"]
    assert np.array_equal(~np.isnan(vel[:, 0]), vref["valid"])
    ok = vref["valid"]
    assert np.all(np.abs(1.0 / vel[ok, 0] ** 2 - vref["gg"][ok]) <= TOL * vref["gg_unc"][ok])
    rows = a["activation_tags.npy"]
    assert list(rows[:, 0]) == [float(t) for t in amap.tags] and rows[0, 3] == np.nanmin(act[:, 0]) and rows[0, 4] == np.nanmax(act[:, 0])


def _emi(tmp_path, steps, **attrs):
    from cgx_hip.emi_models import g_syn
    from cgx_hip.emi_problem import ProblemEMI
    from cgx_hip.emi_solver import SolverEMI
    cfg = {"problem_type": "EMI", "dt": 5e-5, "time_steps": steps, "C_M": 0.02, "sigma_i": 0.7, "sigma_e": 1.3, "quiet": True,
           "cell_tag_file": "square16.xdmf", "facet_tag_file": "square16.xdmf", "mesh_conversion_factor": 1e-6,
           "ics_tags": [1], "ecs_tags": [2], "membrane_tags": [4], "output_dir": str(tmp_path) + os.sep}
    p = ProblemEMI(cfg)
    p.add_ionic_model("HH", stim_fun=g_syn)
    p.init_ionic_model()

    class S(SolverEMI):
        pass
    for k, v in attrs.items():
        setattr(S, k, v)
    return S(p, use_direct_solver=True)


def test_emi_single_steps_and_whole_run(tmp_path):
    steps = 6
    # pass one: one-step solves, ActivationMap.update() after each
    s = _emi(tmp_path / "a", 1)
    p = s.problem
    amap = p.activation_map(0.0, -0.01)
    assert amap.phi is p.phi_M
    verts = amap.vertices
    trace, times = [p.phi_M.numpy()[verts].copy()], [float(p.t.value)]
    for _ in range(steps):
        s.solve()
        amap.update()
        trace.append(p.phi_M.numpy()[verts].copy())
        times.append(float(p.t.value))
    trace, times = np.array(trace), np.array(times)
    assert s.activation is None and not any((tmp_path / "a" / f).exists() for f in FILES)
    got, ref = amap.result(), detector_ref(trace, times, 0.0, -0.01)
    assert np.array_equal(got["count"], ref["count"])
    for key in ("t_act", "t_last", "t_repol", "v_peak", "t_peak", "dvdt_max", "t_dvdt"):
        assert np.array_equal(np.isnan(got[key]), np.isnan(ref[key])), key
    assert _bits(got["v_peak"]) == _bits(ref["v_peak"]) and _bits(got["t_peak"]) == _bits(ref["t_peak"])
    assert np.all(np.abs(got["dvdt_max"] - ref["dvdt_max"]) <= 4.0 * EPS * np.abs(ref["dvdt_max"]))
    assert np.abs(trace[-1] - trace[0]).max() > 0
    # pass two: the whole run with the solver's key, at a threshold the trace crosses
    thr = _midpoint_of_the_largest_rise(trace)
    count, first, tol = _first_crossings(trace, times, thr)
    s2 = _emi(tmp_path / "b", steps, save_activation={"threshold": float(thr)})
    s2.solve()
    a = _check_files(tmp_path / "b", len(verts), len(p._fv), 2, 1)
    act = a["activation.npy"]
    assert count.max() >= 1 and np.array_equal(act[:, 8], count) and np.array_equal(np.isnan(act[:, 0]), np.isnan(first))
    hit = count > 0
    assert np.all(np.abs(act[hit, 0] - first[hit]) <= tol[hit])


# ---- 4. the C ABI --------------------------------------------------------------------------------------------------------------
def test_abi_argument_checks_leave_the_buffers_untouched(tmp_path):
    from cgx_hip.backend import _i32
    p = _problem("square16", tmp_path)
    be = p.backend
    lib, ctx = be.lib, be.ctx
    err = lambda: lib.knp_last_error(ctx).decode()
    dev = be.device
    n = 8
    vertex = torch.arange(n, dtype=torch.int32, device=dev)
    phi = p.phi_m_prev.x.array
    v_last = torch.full((n,), 42.0, dtype=torch.float64, device=dev)
    state = torch.full((7, n), 42.0, dtype=torch.float64, device=dev)
    count = torch.full((n,), 42, dtype=torch.int32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())
    bufs = (P(v_last), P(state), P(count))
    inf, nan = float("inf"), float("nan")
    assert lib.knp_activation_arm(ctx, -1, P(vertex), P(phi), 0.0, *bufs) == E_ARG and "negative" in err()
    for k in range(5):
        args = [P(vertex), P(phi), 0.0, *bufs]
        args[k if k < 2 else k + 1] = None
        assert lib.knp_activation_arm(ctx, n, *args) == E_ARG and "null pointer" in err()
        args = [P(vertex), P(phi), 0.0, 1.0, 0.0, 0.0, *bufs]
        args[k if k < 2 else k + 4] = None
        assert lib.knp_activation_step(ctx, n, *args) == E_ARG and "null pointer" in err()
    assert lib.knp_activation_step(ctx, -1, P(vertex), P(phi), 0.0, 1.0, 0.0, 0.0, *bufs) == E_ARG and "negative" in err()
    for t0, t1 in ((1.0, 1.0), (2.0, 1.0), (0.0, nan), (nan, 1.0)):
        assert lib.knp_activation_step(ctx, n, P(vertex), P(phi), t0, t1, 0.0, 0.0, *bufs) == E_ARG and "later" in err()
    for up, down in ((inf, 0.0), (0.0, -inf), (nan, 0.0), (0.0, nan)):
        assert lib.knp_activation_step(ctx, n, P(vertex), P(phi), 0.0, 1.0, up, down, *bufs) == E_ARG and "threshold" in err()
    assert lib.knp_activation_arm(ctx, 0, P(vertex), P(phi), 0.0, *bufs) == 0
    assert lib.knp_activation_step(ctx, 0, P(vertex), P(phi), 0.0, 1.0, 0.0, 0.0, *bufs) == 0
    # the velocity and the summary
    nv = p.local_mesh.coords.shape[0]
    T = torch.zeros(nv, dtype=torch.float64, device=dev)
    facets = torch.arange(4, dtype=torch.int32, device=dev)
    out = torch.full((4, 5), 42.0, dtype=torch.float64, device=dev)
    assert lib.knp_activation_velocity(ctx, -1, P(facets), P(T), P(out)) == E_ARG and "negative" in err()
    for k in range(3):
        args = [P(facets), P(T), P(out)]
        args[k] = None
        assert lib.knp_activation_velocity(ctx, 4, *args) == E_ARG and "null pointer" in err()
    assert lib.knp_activation_velocity(ctx, 0, P(facets), P(T), P(out)) == 0
    assert lib.knp_diag_activation(ctx, P(T), P(out)) == E_STATE and "no activation facet map" in err()
    n_g = p.local_mesh.gamma.shape[0]
    ptr = np.array([0, 2], dtype=np.int32)
    assert lib.knp_diag_set_activation_facets(ctx, 1, _i32(ptr), _i32(np.array([0, n_g], dtype=np.int32))) == E_ARG
    assert "out of range or listed twice" in err()
    assert lib.knp_diag_set_activation_facets(ctx, 1, _i32(ptr), _i32(np.array([3, 3], dtype=np.int32))) == E_ARG
    assert lib.knp_diag_activation(ctx, P(T), P(out)) == E_STATE
    assert lib.knp_diag_set_activation_facets(ctx, 0, None, None) == 0 and lib.knp_diag_activation(ctx, P(T), P(out)) == 0
    assert lib.knp_diag_set_activation_facets(ctx, 1, _i32(ptr), _i32(np.array([0, 1], dtype=np.int32))) == 0
    assert lib.knp_diag_activation(ctx, None, P(out)) == E_ARG and "null activation-time" in err()
    assert lib.knp_diag_activation(ctx, P(T), None) == E_ARG and "null output" in err()
    torch.cuda.synchronize()
    for t in (v_last, state, out):
        assert np.all(t.cpu().numpy() == 42.0)
    assert np.all(count.cpu().numpy() == 42)
    # a listed index outside the mesh is NaN, not a read out of bounds: vertices of the detector, facets of the velocity
    bad = torch.tensor([0, -1, nv, 1], dtype=torch.int32, device=dev)
    v4, s4, c4 = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros((7, 4), dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    assert lib.knp_activation_arm(ctx, 4, P(bad), P(phi), 0.0, P(v4), P(s4), P(c4)) == 0
    assert list(np.isnan(v4.cpu().numpy())) == [False, True, True, False]
    badf = torch.tensor([0, -1, n_g, 1], dtype=torch.int32, device=dev)
    T.copy_(torch.arange(nv, dtype=torch.float64, device=dev))
    assert lib.knp_activation_velocity(ctx, 4, P(badf), P(T), P(out)) == 0
    flat = out.cpu().numpy().ravel()
    got = flat[:12].reshape(4, 3)                                # 1 + dim slots per facet
    assert np.isnan(got[1:3]).all() and np.isfinite(got[[0, 3]]).all() and np.all(flat[12:] == 42.0)
    # the summary of two facets
    assert lib.knp_diag_activation(ctx, P(T), P(out)) == 0
    row = out.cpu().numpy().ravel()[:5]
    two = np.concatenate([p._fv[0], p._fv[1]])
    assert row[2] == two.min() and row[3] == two.max() and abs(row[0] - p._fmeas[:2].sum()) <= TOL * row[0] and abs(row[4] - row[0]) <= TOL * row[0]
    # several ranks are refused in words
    from cgx_hip.activation import ActivationMap

    class TwoRanks:
        size = 2
    real, p.comm = p.comm, TwoRanks()
    try:
        with pytest.raises(NotImplementedError, match="one rank"):
            ActivationMap(p, 0.0)
    finally:
        p.comm = real
