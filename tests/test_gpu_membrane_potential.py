"""Membrane potential per membrane tag on the device (k_diag_phim and its combine kernels in csrc/knp_diagnostics.inc,
``Backend.membrane_potential``, ``ProblemKNPEMI.membrane_potential``, output key ``save_membrane_potentials``) against the
independent NumPy evaluation of tests/phim_ref.py.

Tolerances: the minimum and the maximum are selections and equal NumPy's exactly.  The integral differs from the reference by the
order of its sums only, |I_gpu - I_ref| <= 1e-12 * S with S = sum_F |F|/d sum_a |phi(v_a)| the un-cancelled sum (the bound of the
flux tests, about 4 500 ulp of S).  Areas are host sums of the same facet measures: rel 1e-13."""
import copy
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from parity_utils import ci_config, make_problem, tissue_config
from phim_ref import TOL, facet_vertices, phim_ref

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -3          # KNP_E_ARG, KNP_E_STATE of include/knpemi_hip.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FILES = ("phi_m_tags.npy", "phi_m_tags_index.npy", "phi_m_points.npy", "phi_m_points_xyz.npy", "gating_points.npy")


def _write(fn, values):
    fn.x.array.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(fn.x.array.device))


def _random_fields(p, seed):
    rng = np.random.default_rng(seed)
    n = p.local_mesh.coords.shape[0]
    for s in range(2):
        for j in range(p.N_ions):
            _write(p.wh[s][j], rng.uniform(1.0, 150.0, n))
        _write(p.wh[s][p.N_ions], rng.uniform(-0.1, 0.1, n))
    _write(p.phi_m_prev, p.wh[0][p.N_ions].numpy() - p.wh[1][p.N_ions].numpy())


def _mesh_config(case):
    if case == "square16":
        return ci_config(N=16, steps=1)
    if case == "cube8":
        return ci_config(N=8, steps=1, kind="cube")
    if case == "tissue2d":
        return tissue_config(2, 18, 3, steps=1)
    return tissue_config(3, 12, 2, steps=1)


def _check_device(got, ref, what):
    """device [n, 3] = (I, min, max) against phim_ref's (I, A, min, max, S, cover)"""
    I, A, lo, hi, S, _ = ref
    err = np.abs(got[:, 0] - I)
    print(f"{what}: max |I_gpu - I_ref| / S = {float(np.max(err / np.maximum(S, 1e-300))) if err.size else 0.0:.3e}")
    assert np.array_equal(got[:, 1], lo), what
    assert np.array_equal(got[:, 2], hi), what
    assert np.all(err <= TOL * S), what


def _solver(cfg):
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    p = make_problem(cfg, "ci")
    p.solver_config["view_ksp"] = False
    return SolverKNPEMI(p, solver_config=p.solver_config)


# ---- 1. random nodal fields ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["square16", "cube8", "tissue2d", "tissue3d_12_2"])
def test_random_fields_match_the_reference_per_tag(case):
    p = make_problem(_mesh_config(case), "ci")
    be = p.create_backend()
    _random_fields(p, 11)
    phi = p.phi_m_prev.numpy().copy()
    tags = [int(t) for t in p.gamma_tags]
    out = p.membrane_potential()
    ref = phim_ref(p, phi, [[t] for t in tags])
    I, A, lo, hi, S, cover = ref
    assert [len(c) for c in cover] == {"square16": [32], "cube8": [192], "tissue2d": [16] * 9, "tissue3d_12_2": [192] * 8}[case]
    assert list(out["tag"]) == tags and all(out[k].shape == (len(tags),) for k in ("area", "mean", "min", "max"))
    assert np.all(S > 0) and np.all(lo < hi)
    got = be.membrane_potential().cpu().numpy()
    assert got.shape == (len(tags), 3)
    _check_device(got, ref, case)
    assert np.allclose(out["area"], A, rtol=1e-13, atol=0)
    assert np.array_equal(out["min"], lo) and np.array_equal(out["max"], hi)
    assert np.array_equal(out["mean"], got[:, 0] / out["area"])
    assert np.all(np.abs(out["mean"] - I / A) <= TOL * S / A)      # the areas' 1e-13 included
    # a tag that no facet carries: area 0 and NaN
    miss = p.membrane_potential(tags=[tags[0], 987654])
    assert miss["area"][1] == 0.0 and np.isnan([miss["mean"][1], miss["min"][1], miss["max"][1]]).all()
    assert miss["mean"][0] == out["mean"][0] and miss["min"][0] == out["min"][0] and miss["max"][0] == out["max"][0]
    # a grouping that merges tags into one slot, with an empty group in the middle (backend level: groups are lists of tags)
    # (a mesh with one tag: an empty group on either side of it)
    groups = [tags[:2], [987654], tags[2:]] if len(tags) >= 3 else [[987654], tags, [424242]]
    be.set_phim_groups(groups)
    got = be.membrane_potential().cpu().numpy()
    ref = phim_ref(p, phi, groups)
    empty = [t for t, c in enumerate(ref[5]) if len(c) == 0]
    assert got.shape == (len(groups), 3) and empty == ([1] if len(tags) >= 3 else [0, 2])
    for t in empty:
        assert got[t, 0] == 0.0 and got[t, 1] == np.inf and got[t, 2] == -np.inf
    _check_device(got, ref, case + " merged")
    assert np.allclose(be.phim_layout().area, ref[1], rtol=1e-13, atol=0)
    # the same bits on every run
    assert be.membrane_potential().cpu().numpy().tobytes() == got.tobytes()
    # a NaN at one membrane vertex shows in the integral of every group that holds the vertex (fmin / fmax drop it from min and max)
    fv = facet_vertices(p)
    v = fv[ref[5][empty[0] + 1][0]][0]
    bad = phi.copy()
    bad[v] = np.nan
    _write(p.phi_m_prev, bad)
    nan = be.membrane_potential().cpu().numpy()
    hit = [t for t, c in enumerate(ref[5]) if len(c) and (fv[c] == v).any()]
    rest = [t for t in range(len(groups)) if t not in hit]
    assert hit and np.isnan(nan[hit, 0]).all() and np.array_equal(nan[rest], got[rest])


# ---- 2. a group of 188 chunks: the workgroup combine -------------------------------------------------------------------------
def test_long_group_takes_the_workgroup_combine():
    from cgx_hip.diagnostics import facet_group_map
    p = make_problem(tissue_config(3, 30, 5, steps=1), "ci")
    be = p.create_backend()
    tags = [int(t) for t in p.gamma_tags]
    assert len(tags) == 125
    for what, groups in (("merged", [tags]), ("per tag", [[t] for t in tags])):
        seg_ptr, facets = facet_group_map(p, groups)
        assert len(facets) == 24000
        chunks = [(seg_ptr[t + 1] - 1) // 128 - seg_ptr[t] // 128 + 1 for t in range(len(groups))]
        assert chunks == ([188] if what == "merged" else [2] * 125)      # more than 64: a workgroup; at most 64: a wave
        _random_fields(p, 17)
        phi = p.phi_m_prev.numpy().copy()
        first, last = p._fv[facets[0]], p._fv[facets[-1]]
        v_hi = [v for v in last if v not in first][0]
        phi[first[0]], phi[v_hi] = -7.0, 7.0          # the scan's two ends carry the extremes
        _write(p.phi_m_prev, phi)
        be.set_phim_groups(groups)
        got = be.membrane_potential().cpu().numpy()
        ref = phim_ref(p, phi, groups)
        assert [len(c) for c in ref[5]] == ([24000] if what == "merged" else [192] * 125)
        assert ref[2].min() == -7.0 and ref[3].max() == 7.0
        _check_device(got, ref, what)
        assert be.membrane_potential().cpu().numpy().tobytes() == got.tobytes()


# ---- 3. after real steps ------------------------------------------------------------------------------------------------------
def _run(cfg, out_dir, interval=None):
    """prepare / step / finish with the key on; returns the solver (with the initial phi_m) and problem.membrane_potential() after
    every step"""
    cfg = copy.deepcopy(cfg)
    cfg["output_dir"] = str(out_dir) + "/"
    cfg["solver"]["output"].update({"save_dat": True, "save_membrane_potentials": True})
    if interval is not None:
        cfg["solver"]["output"]["membrane_potential_interval"] = interval
    s = _solver(cfg)
    s.prepare()
    s.phi_initial = s.problem.phi_m_prev.numpy().copy()
    rows = [s.problem.membrane_potential()]
    for i in range(1, s.time_steps + 1):
        s.step(i)
        rows.append(s.problem.membrane_potential())
    s.finish()
    return s, rows


@pytest.mark.parametrize("case", ["square16", "tissue2d"])
def test_traces_after_real_steps(case, tmp_path):
    steps = 3
    cfg = ci_config(N=16, steps=steps) if case == "square16" else tissue_config(2, 18, 3, steps=steps)
    s, rows = _run(cfg, tmp_path / "a")
    p = s.problem
    tags = [int(t) for t in p.gamma_tags]
    n, d = len(tags), p.local_mesh.coords.shape[1]
    a = tmp_path / "a"
    tr, idx = np.load(a / "phi_m_tags.npy"), np.load(a / "phi_m_tags_index.npy")
    pts, xyz = np.load(a / "phi_m_points.npy"), np.load(a / "phi_m_points_xyz.npy")
    assert tr.shape == (steps + 1, n, 3) and idx.shape == (n, 2) and pts.shape == (steps + 1, n) and xyz.shape == (n, d)
    assert list(idx[:, 0]) == tags and np.array_equal(idx[:, 1], rows[0]["area"]) and np.all(idx[:, 1] > 0)
    # the initial phi_m is one value on every membrane
    ftags = np.asarray(p.gamma_facet_tags)
    for t, tag in enumerate(tags):
        phi0 = np.unique(s.phi_initial[p._fv[ftags == tag]])
        assert phi0.shape == (1,) and phi0[0] != 0.0
        assert tr[0, t, 1] == tr[0, t, 2] == pts[0, t] == phi0[0]
        assert abs(tr[0, t, 0] - phi0[0]) <= TOL * abs(phi0[0])
    for i, r in enumerate(rows):
        assert np.stack([r["mean"], r["min"], r["max"]], axis=1).tobytes() == tr[i].tobytes(), i
    assert np.abs(tr[-1] - tr[0]).max() > 0                   # the steps moved the field
    slack = TOL * np.abs(tr).max()                      # the mean of a constant is that constant up to rounding
    assert np.all(tr[:, :, 1] - slack <= tr[:, :, 0]) and np.all(tr[:, :, 0] <= tr[:, :, 2] + slack)
    assert np.all(tr[:, :, 1] <= pts) and np.all(pts <= tr[:, :, 2])
    # the column of the membrane-data tag is the single-point trace
    k = tags.index(int(p.membrane_data_tag))
    assert np.array_equal(1000.0 * pts[:, k], np.load(a / "phi_m.npy"))
    assert np.array_equal(xyz[k], p.png_point[0])
    assert hasattr(p, "n")                                    # the CI physics has gating variables
    gat = np.load(a / "gating_points.npy")
    assert gat.shape == (steps + 1, n, 3)
    for j, nm in enumerate(("n", "m", "h")):
        assert np.array_equal(gat[:, k, j], np.load(a / f"{nm}.npy"))
    # every second step
    s2, _ = _run(cfg, tmp_path / "b", interval=2)
    b = tmp_path / "b"
    tr2, pts2 = np.load(b / "phi_m_tags.npy"), np.load(b / "phi_m_points.npy")
    assert tr2.shape == (2, n, 3) and pts2.shape == (2, n)
    assert tr2.tobytes() == tr[[0, 2]].tobytes() and pts2.tobytes() == pts[[0, 2]].tobytes()
    assert np.load(b / "gating_points.npy").tobytes() == gat[[0, 2]].tobytes()


# ---- 4. two ranks on one GPU against one rank ---------------------------------------------------------------------------------
def _free_port():
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def _coordinate_field(x):
    """a nodal field that is the same bits at the same point on every rank layout"""
    u, v = 1.0e6 * x[:, 0], 1.0e6 * x[:, 1]      # elementwise products and sums only: no library call whose rounding may depend on the length
    return 0.05 * (u * u - 0.7 * v) - 0.03 * (v * v * u) + 0.011 * (u - v)


def _reduce_ref(p, ref):
    I, A, lo, hi, S, _ = ref
    if p.comm.size == 1:
        return I, A, lo, hi, S
    parts = p.comm.all_gather_object((I, A, lo, hi, S))
    return (np.sum([q[0] for q in parts], axis=0), np.sum([q[1] for q in parts], axis=0), np.min([q[2] for q in parts], axis=0),
            np.max([q[3] for q in parts], axis=0), np.sum([q[4] for q in parts], axis=0))


def _worker(rank, size, port, out_dir, q):
    try:
        for path in (os.path.join(ROOT, "knp-emi-cgx_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
            sys.path.insert(0, path)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        torch.cuda.set_device(0)
        if size > 1:
            dist.init_process_group("gloo", rank=rank, world_size=size)
        from parity_utils import run_native
        from cgx_hip import output as outmod
        host = []
        orig = outmod.RunOutput.record

        def record(self, i):                # the reference on this rank layout's own fields, reduced over the ranks
            orig(self, i)
            tags = [int(t) for t in self.p.gamma_tags]
            host.append(_reduce_ref(self.p, phim_ref(self.p, self.p.phi_m_prev.numpy(), [[t] for t in tags])))
        outmod.RunOutput.record = record
        cfg = tissue_config(2, 18, 3, steps=3, rtol=1e-13)
        cfg["output_dir"] = out_dir + "/"
        cfg["solver"]["output"].update({"save_dat": True, "save_membrane_potentials": True})
        s = run_native(cfg)
        p = s.problem
        # a field given by the coordinates: the layouts then hold the same values
        tags = [int(t) for t in p.gamma_tags]
        phi = _coordinate_field(np.asarray(p.local_mesh.coords))
        _write(p.phi_m_prev, phi)
        out = p.membrane_potential()
        ref = _reduce_ref(p, phim_ref(p, phi, [[t] for t in tags]))
        n_local = int((s.output.probes["owner"] == rank).sum())
        q.put((rank, "ok", {k: np.asarray(v) for k, v in out.items()}, ref, [np.stack(h) for h in zip(*host)], s.output.probes, n_local))
        if size > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:      # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc(), None, None, None, None, None))


def _spawn(layouts):
    """one group of worker processes per (size, out_dir), all groups at once (three processes on the GPU)"""
    ctx = mp.get_context("spawn")
    groups = []
    for size, out_dir in layouts:
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=_worker, args=(r, size, port, out_dir, q)) for r in range(size)]
        for pr in procs:
            pr.start()
        groups.append((size, q, procs))
    out = []
    for size, q, procs in groups:
        res = sorted([q.get(timeout=300) for _ in range(size)], key=lambda r: r[0])
        for pr in procs:
            pr.join(timeout=60)
        for r in res:
            assert r[1] == "ok", f"rank {r[0]}:\n{r[1]}"
        out.append(res)
    return out


def test_two_ranks_give_the_one_rank_membrane_potential(tmp_path):
    """On a field given by the coordinates both layouts hold the same nodal values: min, max and the probes are equal exactly, the
    mean within the integral's bound.  The traces of the runs are checked per layout against the reference on that layout's own
    fields (the two solves follow their own trajectories), and across layouts at record 0, where the fields are the same."""
    (one,), two = _spawn([(1, str(tmp_path / "one")), (2, str(tmp_path / "two"))])
    o1, o2 = one[2], two[0][2]
    assert all(np.array_equal(r[2]["min"], o1["min"]) and np.array_equal(r[2]["max"], o1["max"]) for r in two)
    assert np.array_equal(o2["tag"], o1["tag"]) and np.allclose(o2["area"], o1["area"], rtol=1e-13, atol=0)
    for r in [one] + two:                                     # every rank returns the reduction over all ranks
        I, A, lo, hi, S = r[3]
        assert np.array_equal(r[2]["min"], lo) and np.array_equal(r[2]["max"], hi)
        assert np.all(np.abs(r[2]["mean"] * r[2]["area"] - I) <= TOL * S)
    S, A = one[3][4], one[3][1]
    print("max |mean_2 - mean_1| A / S =", float(np.max(np.abs(o2["mean"] - o1["mean"]) * A / S)))
    assert np.all(np.abs(o2["mean"] - o1["mean"]) <= TOL * S / A)
    # probes: the same points, found on both ranks of the two-rank layout
    assert np.array_equal(two[0][5]["xyz"], one[5]["xyz"]) and np.array_equal(two[1][5]["xyz"], one[5]["xyz"])
    assert two[0][6] > 0 and two[1][6] > 0 and two[0][6] + two[1][6] == one[6] == 9
    files = {}
    for name, res in (("one", one), ("two", two[0])):
        d = tmp_path / name
        tr, idx = np.load(d / "phi_m_tags.npy"), np.load(d / "phi_m_tags_index.npy")
        pts, xyz = np.load(d / "phi_m_points.npy"), np.load(d / "phi_m_points_xyz.npy")
        I, A, lo, hi, S = res[4]
        assert tr.shape == (4, 9, 3) and pts.shape == (4, 9) and I.shape == (4, 9)
        assert np.array_equal(tr[:, :, 1], lo) and np.array_equal(tr[:, :, 2], hi)
        assert np.all(np.abs(tr[:, :, 0] * idx[:, 1] - I) <= TOL * S)
        assert np.array_equal(xyz, one[5]["xyz"])
        files[name] = (tr, idx, pts, np.load(d / "phi_m.npy"))
    (tr1, idx1, pts1, v1), (tr2, idx2, pts2, v2) = files["one"], files["two"]
    assert np.array_equal(tr2[0, :, 1:], tr1[0, :, 1:]) and np.array_equal(pts2[0], pts1[0])
    assert np.all(np.abs(tr2[0, :, 0] - tr1[0, :, 0]) <= TOL * one[4][4][0] / one[4][1][0])
    # in each layout one column of the probes is that layout's single-point trace
    assert any(np.array_equal(1000.0 * pts1[:, c], v1) for c in range(9)) and any(np.array_equal(1000.0 * pts2[:, c], v2) for c in range(9))


# ---- 5. the C ABI -------------------------------------------------------------------------------------------------------------
def test_abi_states_arguments_and_map_replacement():
    from cgx_hip.backend import _i32
    from cgx_hip.diagnostics import membrane_program
    p = make_problem(tissue_config(3, 12, 2, steps=1, stimulus=True), "ci")
    be = p.create_backend()
    lib, ctx = be.lib, be.ctx
    _random_fields(p, 31)
    phi = p.phi_m_prev.numpy().copy()
    n_g = p.local_mesh.gamma.shape[0]
    f = be.fields()
    out = torch.zeros(6, dtype=torch.float64, device=be.device)
    outp = C.c_void_p(out.data_ptr())
    err = lambda: lib.knp_last_error(ctx).decode()
    # before a map
    assert lib.knp_diag_membrane_potential(ctx, C.byref(f), outp) == E_STATE
    assert "no phi_m facet map" in err()
    # bad maps leave the state as it was: an index past the mesh's facets, a facet listed twice
    ptr = np.array([0, 2], dtype=np.int32)
    assert lib.knp_diag_set_phim_facets(ctx, 1, _i32(ptr), _i32(np.array([0, n_g], dtype=np.int32))) == E_ARG
    assert "out of range or listed twice" in err()
    assert lib.knp_diag_set_phim_facets(ctx, 1, _i32(ptr), _i32(np.array([5, 5], dtype=np.int32))) == E_ARG
    assert lib.knp_diag_membrane_potential(ctx, C.byref(f), outp) == E_STATE
    # no tags: nothing is launched, nothing is written
    out.fill_(42.0)
    assert lib.knp_diag_set_phim_facets(ctx, 0, None, None) == 0
    assert lib.knp_diag_membrane_potential(ctx, C.byref(f), outp) == 0
    assert np.all(out.cpu().numpy() == 42.0)
    # a map, then null arguments
    assert lib.knp_diag_set_phim_facets(ctx, 1, _i32(ptr), _i32(np.array([0, 1], dtype=np.int32))) == 0
    assert lib.knp_diag_membrane_potential(ctx, C.byref(f), None) == E_ARG
    assert "null output" in err()
    assert lib.knp_diag_membrane_potential(ctx, None, outp) == E_ARG
    assert lib.knp_diag_membrane_potential(ctx, C.byref(f), outp) == 0
    two = np.concatenate([p._fv[0], p._fv[1]])
    got = out.cpu().numpy()
    assert got[1] == phi[two].min() and got[2] == phi[two].max() and np.all(got[3:] == 42.0)
    want = sum(p._fmeas[F] / 3.0 * phi[p._fv[F]].sum() for F in (0, 1))
    assert abs(got[0] - want) <= TOL * sum(p._fmeas[F] / 3.0 * np.abs(phi[p._fv[F]]).sum() for F in (0, 1))
    # the stimulus trace's map and the flux map live next to it: replacing the phi_m map leaves their results as they were
    tags = [int(t) for t in p.gamma_tags]
    spec = membrane_program(p, p.stim_ufl_expr)
    be.set_diag_program(spec)
    be.set_facet_groups([p.stimulus_tags])
    be.set_flux_groups([[t] for t in tags])
    stim0 = be.membrane_integral(torch.zeros(1, dtype=torch.float64, device=be.device)).cpu().numpy().tobytes()
    flux0 = be.membrane_fluxes().cpu().numpy().tobytes()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for k in range(100):                     # setting maps over and over does not grow the device's use
        be.set_phim_groups([tags[:1 + k % 2]])
        be.set_phim_groups([[t] for t in tags])
    got = be.membrane_potential().cpu().numpy()
    free1 = torch.cuda.mem_get_info()[0]
    _check_device(got, phim_ref(p, phi, [[t] for t in tags]), "replaced map")
    assert free0 - free1 < 8 * 2 ** 20, (free0, free1)
    assert be.membrane_integral(torch.zeros(1, dtype=torch.float64, device=be.device)).cpu().numpy().tobytes() == stim0
    assert be.membrane_fluxes().cpu().numpy().tobytes() == flux0
    be.set_facet_groups([tags])
    be.set_flux_groups([tags])
    assert be.membrane_potential().cpu().numpy().tobytes() == got.tobytes()


# ---- 6. off by default --------------------------------------------------------------------------------------------------------
def test_off_by_default(tmp_path):
    cfg = tissue_config(2, 18, 3, steps=1)
    cfg["output_dir"] = str(tmp_path) + "/"
    cfg["solver"]["output"].update({"save_dat": True})
    s = _solver(cfg)
    s.solve()
    assert (tmp_path / "phi_m.npy").exists()
    assert not any((tmp_path / name).exists() for name in NEW_FILES)
    assert s.output.phim is None and getattr(s.backend, "_phim", None) is None      # nothing allocated, no map set
    f = s.backend.fields()
    out = torch.zeros(3, dtype=torch.float64, device=s.backend.device)
    assert s.backend.lib.knp_diag_membrane_potential(s.backend.ctx, C.byref(f), C.c_void_p(out.data_ptr())) == E_STATE
