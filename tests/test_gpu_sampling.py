"""Field sampling on the device (k_sample_locate / k_sample_weights / k_sample_gather in csrc/knp_sample.inc, ``FieldSampler`` /
``GridSampler`` of cgx_hip/sampling.py, ``ProblemKNPEMI.sample`` and the output keys ``sample_grids`` / ``sample_interval``) against
the all-pairs long-double reference of tests/sampling_ref.py, whose inputs tests/test_sampling_host.py shows to be well-posed.

Tolerances: the winning cell is a decision on inputs at least 1e-11 away from changing it and equals the reference exactly.  Weights:
1e-12 (float64 against long double differ by at most 5.9e-15 on these meshes).  Affine fields: 1e-12 max|f|.  Random nodal data
against the NumPy gather through the reference's cells and weights: 1e-13 max|f| (the weights' 1e-14 and a sum of dim + 1 terms)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import sampling_ref as SR
from parity_utils import ci_config, make_problem, run_with_snapshots, snapshot_state

pytestmark = pytest.mark.gpu
E_ARG = -1
LOCATION_CASES = ["square8_aligned", "cube4_aligned", "cube4_oblique"] + SR.IRREGULAR + ["two_tag"]
EXTREME_CASES = ["square8_257", "cube8_five", "cube8_one"]


@pytest.fixture(scope="module")
def problems(tmp_path_factory):
    """one problem with its context per mesh, shared by the tests of this module"""
    cache = {}
    tmp = tmp_path_factory.mktemp("sampling_meshes")

    def get(mesh):
        if mesh not in cache:
            p = make_problem(SR.mesh_config(mesh, tmp), "ci")
            p.create_backend()
            cache[mesh] = p
        return cache[mesh]
    return get


def _sampler(case, p, side=None):
    from cgx_hip.sampling import FieldSampler, GridSampler
    pts, grid, _, _, _ = SR.case_reference(case, p)
    if grid is None:
        return FieldSampler(p, pts, side)
    gs = GridSampler(p, *grid, side=side)
    assert np.array_equal(gs.xyz.reshape(pts.shape), pts)
    return gs


def _dev(a, p):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=p.backend.device)


def _check_location(s, p, cell, w, what):
    n = cell.shape[0]
    err = float(np.abs(s.weights.reshape(n, -1) - w).max())
    print(f"{what}: {n} points, found {(cell >= 0).sum()}, max |w_gpu - w_ref| = {err:.3e}")
    assert np.array_equal(s.cell.reshape(n), cell), what
    assert np.array_equal(s.found.reshape(n), cell >= 0), what
    assert err <= 1e-12, what
    tags = np.asarray(p.local_mesh.cell_tags)
    assert np.array_equal(s.cell_tag.reshape(n), np.where(cell >= 0, tags[np.maximum(cell, 0)], -1)) and s.cell_tag.dtype == np.int32


def _random_nodal(p, seed, n_fields=3):
    rng = np.random.default_rng(seed)
    nv = p.local_mesh.coords.shape[0]
    return rng.uniform(-150.0, 150.0, (n_fields, nv)), rng.uniform(-150.0, 150.0, (n_fields, nv))


def _check_gather(s, p, cell, w, seed, what):
    lm = p.local_mesh
    Fi, Fe = _random_nodal(p, seed)
    got = s([_dev(f, p) for f in Fi], [_dev(f, p) for f in Fe], fill=-7.5).cpu().numpy().reshape(len(Fi), -1)
    scale = max(np.abs(Fi).max(), np.abs(Fe).max())
    for f in range(len(Fi)):
        want = SR.interpolate_ref(np.asarray(lm.cells), p.cell_side, cell, w, Fi[f], Fe[f], fill=-7.5)
        err = float(np.abs(got[f] - want).max())
        assert err <= 1e-13 * scale, (what, f, err)
    assert np.all(got[:, cell < 0] == -7.5)
    return got


# ---- 1. location ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LOCATION_CASES)
def test_cells_and_weights_match_the_reference(case, problems):
    p = problems(SR.CASES[case][0])
    _, grid, cell, w, _ = SR.case_reference(case, p)
    s = _sampler(case, p)
    assert s.cell.shape == tuple(grid[2]) and s.weights.shape == tuple(grid[2]) + (p.local_mesh.coords.shape[1] + 1,)
    _check_location(s, p, cell, w, case)
    if case == "square8_aligned":      # the membrane lines x, y in {0.25, 0.75} are ties between the sides: the lowest cell decides
        side = np.where(s.found, p.cell_side[np.maximum(s.cell, 0)].astype(np.int64), -1)
        lines = np.concatenate([side[4, 4:13], side[12, 4:13], side[4:13, 4], side[4:13, 12]])
        assert np.all(side[5:12, 5:12] == 0) and np.all(side[:4] == 1) and np.all(side[:, 13:] == 1) and set(np.unique(lines)) == {0, 1}
    if case == "two_tag":
        assert set(np.unique(s.cell_tag)) == {-1, 1, 2, 3}
    s.close()


# ---- 2. interpolation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LOCATION_CASES)
def test_interpolation_fill_and_sides(case, problems):
    from cgx_hip.sampling import FieldSampler
    p = problems(SR.CASES[case][0])
    lm = p.local_mesh
    coords, cells = np.asarray(lm.coords), np.asarray(lm.cells)
    pts, _, cell, w, _ = SR.case_reference(case, p)
    s = _sampler(case, p)
    found = cell >= 0
    side = np.where(found, p.cell_side[np.maximum(cell, 0)].astype(np.int64), -1)
    # per-side affine fields a.x + b are reproduced
    L = coords.max(axis=0) - coords.min(axis=0)
    d = coords.shape[1]
    a_i, b_i = np.array([3.0, -2.0, 1.5])[:d] / L, 0.7
    a_e, b_e = np.array([-1.0, 4.0, 2.5])[:d] / L, -1.3
    f_i, f_e = coords @ a_i + b_i, coords @ a_e + b_e
    got = s([_dev(f_i, p)], [_dev(f_e, p)]).cpu().numpy().reshape(-1)
    want = np.where(side == 0, pts @ a_i + b_i, pts @ a_e + b_e)
    scale = max(np.abs(f_i).max(), np.abs(f_e).max())
    err = float(np.abs(got[found] - want[found]).max())
    print(f"{case}: affine max error / max|f| = {err / scale:.3e}")
    assert err <= 1e-12 * scale
    assert np.isnan(got[~found]).all() and not np.isnan(got[found]).any()          # the default fill
    # random nodal data against the NumPy gather through the reference's cells and weights; an explicit fill value
    _check_gather(s, p, cell, w, 5, case)
    # f_i = 1, f_e = 2: 1 + side of the winning cell (the renormalised weights sum to 1 within 2 (d + 1) roundings: 9e-16, twice that on f_e)
    nv = coords.shape[0]
    got = s([_dev(np.ones(nv), p)], [_dev(np.full(nv, 2.0), p)], fill=0.0).cpu().numpy().reshape(-1)
    assert np.array_equal(np.rint(got), np.where(found, 1.0 + side, 0.0)) and np.abs(got - np.rint(got)).max() <= 2e-15
    # into a given buffer, two calls: the same bits
    out = torch.full((1,) + s.cell.shape, 9.0, dtype=torch.float64, device=p.backend.device)
    r = s([_dev(f_i, p)], [_dev(f_e, p)], out=out)
    assert r.data_ptr() == out.data_ptr() and r.shape == out.shape
    assert out.cpu().numpy().tobytes() == s([_dev(f_i, p)], [_dev(f_e, p)]).cpu().numpy().tobytes()
    s.close()
    # side = 0 / 1 restrict the search: points in the other side's cells count as outside
    for sd in (0, 1):
        sel = np.nonzero(p.cell_side[:lm.n_cells_owned] == sd)[0]
        c_ref, w_ref, _ = SR.locate_ref(coords, cells, pts, select=sel)
        r = FieldSampler(p, pts, side=sd)
        _check_location(r, p, c_ref, w_ref, f"{case} side {sd}")
        assert np.all(p.cell_side[c_ref[c_ref >= 0]] == sd) and np.array_equal(c_ref[side == sd], cell[side == sd])
        if case.startswith("delaunay") or case in ("two_tag", "cube4_oblique"):      # no grid point on the membrane: no tie between the sides
            assert np.all(c_ref[side == 1 - sd] < 0)
        only = (r([_dev(f_i, p)], None) if sd == 0 else r(None, [_dev(f_e, p)])).cpu().numpy()[0]      # the other side's list is not needed
        want = SR.interpolate_ref(cells, p.cell_side, c_ref, w_ref, f_i, f_e)
        ok = c_ref >= 0
        assert np.abs(only[ok] - want[ok]).max() <= 1e-13 * scale and np.isnan(only[~ok]).all()
        r.close()


def test_problem_sample_returns_the_merged_fields(problems):
    p = problems("delaunay2d_12")
    pts, grid, cell, w, _ = SR.case_reference("delaunay2d_12", p)
    rng = np.random.default_rng(21)
    for side in range(2):
        for k in range(4):
            p.wh[side][k].x.array.copy_(_dev(rng.uniform(1.0, 150.0, p.local_mesh.coords.shape[0]), p))
    cells = np.asarray(p.local_mesh.cells)
    want = np.stack([SR.interpolate_ref(cells, p.cell_side, cell, w, p.wh[0][k].numpy(), p.wh[1][k].numpy()) for k in range(4)])
    got = p.sample(pts)
    assert got.shape == (4, pts.shape[0]) and isinstance(got, np.ndarray)
    assert np.allclose(got, want, rtol=0, atol=1e-13 * 150.0, equal_nan=True) and np.isnan(got[:, cell < 0]).all()
    s = _sampler("delaunay2d_12", p)
    sub = p.sample(s, fields=["phi", "K"])
    assert sub.shape == (2,) + tuple(grid[2]) and sub.reshape(2, -1).tobytes() == got[[3, 1]].tobytes()
    with pytest.raises(ValueError, match="Ca"):
        p.sample(s, fields=["Ca"])
    s.close()


# ---- 3. load extremes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXTREME_CASES)
def test_load_extremes(case, problems):
    p = problems(SR.CASES[case][0])
    _, _, cell, w, _ = SR.case_reference(case, p)
    s = _sampler(case, p)
    n_cells = p.local_mesh.cells.shape[0]
    assert cell.shape[0] / n_cells > 500 if case == "square8_257" else cell.shape[0] <= 5
    _check_location(s, p, cell, w, case)
    _check_gather(s, p, cell, w, 9, case)
    if case == "cube8_five":
        assert list(cell >= 0) == [True, True, True, False, True]
    s.close()


# ---- 4. repeatability -----------------------------------------------------------------------------------------------------------
def test_plans_are_repeatable_and_independent(problems):
    from cgx_hip.sampling import FieldSampler
    p = problems("hub3d_5_60")
    pts, _, cell, w, _ = SR.case_reference("hub3d_5_60", p)
    Fi, Fe = _random_nodal(p, 13)
    fi, fe = [_dev(f, p) for f in Fi], [_dev(f, p) for f in Fe]
    a = FieldSampler(p, pts)
    b = FieldSampler(p, pts)                      # two builds: the same bits
    assert a.plan != b.plan
    assert a.cell.tobytes() == b.cell.tobytes() and a.weights.tobytes() == b.weights.tobytes()
    ra = a(fi, fe).cpu().numpy()
    assert ra.tobytes() == a(fi, fe).cpu().numpy().tobytes() == b(fi, fe).cpu().numpy().tobytes()      # two calls, two plans
    other = FieldSampler(p, pts[::3] * 0.5, side=1)         # a different plan alive next to them does not disturb them
    ro = other(None, fe).cpu().numpy()
    assert a(fi, fe).cpu().numpy().tobytes() == ra.tobytes()
    # destroying one and creating another reuses its id and nothing of its content
    freed = b.plan
    b.close()
    with pytest.raises(Exception, match="closed"):
        b(fi, fe)
    c = FieldSampler(p, pts[::-1].copy())
    assert c.plan == freed
    assert np.array_equal(c.cell, cell[::-1]) and np.abs(c.weights - w[::-1]).max() <= 1e-12
    assert c(fi, fe).cpu().numpy().tobytes() == ra[:, ::-1].tobytes()
    assert other(None, fe).cpu().numpy().tobytes() == ro.tobytes() and a(fi, fe).cpu().numpy().tobytes() == ra.tobytes()
    for s in (a, c, other):
        s.close()


# ---- 5. the C ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_validation(problems):
    from cgx_hip._lib import f64p, i32p
    from cgx_hip.sampling import FieldSampler, bin_points
    p = problems("cube4")
    be = p.backend
    lib, ctx = be.lib, be.ctx
    pts, _, cell, w, _ = SR.case_reference("cube4_oblique", p)
    pts = np.ascontiguousarray(pts)
    n = pts.shape[0]
    b = bin_points(pts)
    nb = len(b["bin_ptr"]) - 1
    err = lambda: lib.knp_last_error(ctx).decode()
    plan = C.c_int32(-5)
    f64, i32 = (lambda a: a.ctypes.data_as(f64p)), (lambda a: a.ctypes.data_as(i32p))
    origin, size = np.ascontiguousarray(b["origin"]), np.ascontiguousarray(b["size"])

    def create(n_points=n, pts_=pts, side=-1, n_bins=nb, bin_ptr=b["bin_ptr"], bin_pts=b["bin_pts"], org=origin, sz=size, shp=b["shape"], out=plan):
        return lib.knp_sample_plan_create(ctx, n_points, None if pts_ is None else f64(pts_), side, n_bins, None if bin_ptr is None else i32(bin_ptr),
                                          None if bin_pts is None else i32(bin_pts), f64(org), f64(sz), i32(shp), None if out is None else C.byref(out))
    for bad, word in ((dict(n_points=0), "n_points"), (dict(n_points=-3), "n_points"), (dict(pts_=None), "null"), (dict(bin_ptr=None), "null"),
                      (dict(bin_pts=None), "null"), (dict(out=None), "null"), (dict(side=2), "side"), (dict(n_bins=nb + 1), "n_bins")):
        assert create(**bad) == E_ARG, bad
        assert word in err(), (bad, err())
    swapped = b["bin_ptr"].copy()                   # non-monotone, ends unchanged
    k = [k for k in range(1, nb - 1) if swapped[k + 1] > swapped[k]][0]
    swapped[k], swapped[k + 1] = swapped[k + 1], swapped[k]
    assert create(bin_ptr=swapped) == E_ARG and "non-decreasing" in err()
    twice = b["bin_pts"].copy()
    twice[1] = twice[0]
    assert create(bin_pts=twice) == E_ARG and "every point once" in err()
    moved = np.roll(b["bin_pts"], 1)                # a permutation, but the points are not in their bins
    assert create(bin_pts=moved) == E_ARG and "not in the bin" in err()
    nan = pts.copy()
    nan[3, 1] = np.nan
    assert create(pts_=nan) == E_ARG and "not finite" in err()
    assert create(sz=np.zeros(3)) == E_ARG and "positive bin sizes" in err()
    assert plan.value == -5                         # nothing was created
    # unknown plans
    cbuf, wbuf = np.empty(n, dtype=np.int32), np.empty((n, 4))
    out = torch.full((n,), 42.0, dtype=torch.float64, device=be.device)
    nv = p.local_mesh.coords.shape[0]
    ones = torch.ones(nv, dtype=torch.float64, device=be.device)
    ptr = (C.c_void_p * 1)(ones.data_ptr())
    null = (C.c_void_p * 1)(None)
    for bad in (-1, 999, 2 ** 31 - 1):
        assert lib.knp_sample_plan_get(ctx, bad, i32(cbuf), f64(wbuf)) == E_ARG and "unknown sampling plan" in err()
        assert lib.knp_sample(ctx, bad, 1, ptr, ptr, 0.0, C.c_void_p(out.data_ptr())) == E_ARG and "unknown sampling plan" in err()
        assert lib.knp_sample_plan_destroy(ctx, bad) == E_ARG
    # a good plan, then bad sampling calls: nothing is launched, the buffer keeps its content
    assert create() == 0 and plan.value >= 0
    assert lib.knp_sample_plan_get(ctx, plan.value, i32(cbuf), f64(wbuf)) == 0
    assert np.array_equal(cbuf, cell) and np.abs(wbuf - w).max() <= 1e-12
    assert lib.knp_sample_plan_get(ctx, plan.value, None, f64(wbuf)) == E_ARG and "null" in err()
    assert lib.knp_sample(ctx, plan.value, 1, ptr, ptr, 0.0, None) == E_ARG and "null output" in err()
    assert lib.knp_sample(ctx, plan.value, 0, ptr, ptr, 0.0, C.c_void_p(out.data_ptr())) == E_ARG and "n_fields" in err()
    assert (p.cell_side[cell[cell >= 0]] == 0).any() and (p.cell_side[cell[cell >= 0]] == 1).any()
    assert lib.knp_sample(ctx, plan.value, 1, None, ptr, 0.0, C.c_void_p(out.data_ptr())) == E_ARG and "null intracellular field" in err()
    assert lib.knp_sample(ctx, plan.value, 1, ptr, null, 0.0, C.c_void_p(out.data_ptr())) == E_ARG and "null extracellular field" in err()
    assert np.all(out.cpu().numpy() == 42.0)
    assert lib.knp_sample(ctx, plan.value, 1, ptr, ptr, -3.0, C.c_void_p(out.data_ptr())) == 0
    assert np.allclose(out.cpu().numpy(), np.where(cell >= 0, 1.0, -3.0), rtol=0, atol=1e-15)
    assert lib.knp_sample_plan_destroy(ctx, plan.value) == 0
    assert lib.knp_sample_plan_destroy(ctx, plan.value) == E_ARG and "unknown sampling plan" in err()
    assert lib.knp_sample(ctx, plan.value, 1, ptr, ptr, 0.0, C.c_void_p(out.data_ptr())) == E_ARG
    # the Python layer's own argument checks
    with pytest.raises(ValueError):
        FieldSampler(p, np.zeros((0, 3)))
    with pytest.raises(ValueError):
        FieldSampler(p, pts, side=2)
    s = FieldSampler(p, pts)
    with pytest.raises(ValueError, match="one value per local vertex"):
        s([ones[:-1]], [ones])
    with pytest.raises(ValueError, match="out must be"):
        s([ones], [ones], out=torch.zeros(n + 1, dtype=torch.float64, device=be.device))
    s.close()


# ---- 6. end to end --------------------------------------------------------------------------------------------------------------
GRIDS = {"square8": {"name": "whole", "origin": [-0.05, -0.04], "axes": [[1.1, 0.0], [0.0, 1.08]], "shape": [12, 10], "fields": ["K", "phi"]},
         "cube4": {"name": "mid_z", "origin": [0.0, 0.0, 0.4], "axes": [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], "shape": [9, 7]}}


@pytest.mark.parametrize("mesh", ["square8", "cube4"])
def test_sample_grids_of_a_run_match_the_reference(mesh, tmp_path):
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    from cgx_hip.sampling import grid_points
    cfg = ci_config(steps=4, **SR.GENERATED[mesh])
    cfg["output_dir"] = str(tmp_path) + "/"
    grid = copy.deepcopy(GRIDS[mesh])
    cfg["solver"]["output"].update({"sample_grids": [grid], "sample_interval": 2})
    p = make_problem(cfg, "ci")
    p.solver_config["view_ksp"] = False
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    s.setup_solver()                                  # record 0 is taken here: snapshot the same state
    states = {0: snapshot_state(p)}
    s.setup_solver = lambda: None
    snaps = run_with_snapshots(s, {2, 4})
    states.update({i: snaps[i]["state"] for i in (2, 4)})
    name, shape = grid["name"], tuple(grid["shape"])
    fields = grid.get("fields", ["Na", "K", "Cl", "phi"])
    data, tags = np.load(tmp_path / f"grid_{name}.npy"), np.load(tmp_path / f"grid_{name}_tags.npy")
    xyz, t = np.load(tmp_path / f"grid_{name}_xyz.npy"), np.load(tmp_path / f"grid_{name}_t.npy")
    lm = p.local_mesh
    dim = lm.coords.shape[1]
    assert data.shape == (3, len(fields)) + shape and tags.shape == shape and tags.dtype == np.int32
    assert xyz.shape == shape + (dim,) and t.shape == (3,)
    f = float(p.mesh_conversion_factor)
    want_xyz = grid_points(np.array(grid["origin"]) * f, np.array(grid["axes"]) * f, shape)
    assert np.array_equal(xyz, want_xyz)
    assert np.allclose(t, [0.0, 2 * float(p.dt.value), 4 * float(p.dt.value)], rtol=1e-12, atol=0)
    cell, w, margin = SR.locate_ref(np.asarray(lm.coords), np.asarray(lm.cells), xyz.reshape(-1, dim))
    assert margin > 1e-11 and (cell >= 0).sum() >= 30 and ((cell < 0).sum() >= 10 or mesh == "cube4")
    assert np.array_equal(tags.reshape(-1), np.where(cell >= 0, np.asarray(lm.cell_tags)[np.maximum(cell, 0)], -1))
    assert set(np.unique(tags)) >= {1, 2}
    for r, step in enumerate((0, 2, 4)):
        st = states[step]
        for k, nm in enumerate(fields):
            fi, fe = (st["phi_i"], st["phi_e"]) if nm == "phi" else (st["k_i"][("Na", "K", "Cl").index(nm)], st["k_e"][("Na", "K", "Cl").index(nm)])
            want = SR.interpolate_ref(np.asarray(lm.cells), p.cell_side, cell, w, fi, fe)
            got = data[r, k].reshape(-1)
            scale = max(np.abs(fi).max(), np.abs(fe).max())
            assert np.isnan(got[cell < 0]).all(), (step, nm)
            assert np.abs(got[cell >= 0] - want[cell >= 0]).max() <= 1e-13 * scale, (step, nm)
    assert np.abs(data[2] - data[0])[~np.isnan(data[0])].max() > 0          # the steps moved the fields
    # a run without the key makes none of the new calls and writes none of the files
    cfg2 = ci_config(steps=1, **SR.GENERATED[mesh])
    cfg2["output_dir"] = str(tmp_path / "off") + "/"
    cfg2["solver"]["output"]["save_dat"] = True
    p2 = make_problem(cfg2, "ci")
    p2.solver_config["view_ksp"] = False
    s2 = SolverKNPEMI(p2, solver_config=p2.solver_config)
    s2.solve()
    assert s2.sample_grids == [] and s2.output.grids == [] and not list((tmp_path / "off").glob("grid_*"))


def test_field_sampler_on_an_emi_problem():
    from cgx_hip.emi_models import g_syn
    from cgx_hip.emi_problem import ProblemEMI
    from cgx_hip.emi_solver import SolverEMI
    from cgx_hip.sampling import FieldSampler
    cfg = {"problem_type": "EMI", "dt": 5e-5, "time_steps": 1, "C_M": 0.02, "sigma_i": 0.7, "sigma_e": 1.3, "quiet": True,
           "cell_tag_file": "square8.xdmf", "facet_tag_file": "square8.xdmf", "mesh_conversion_factor": 1e-6,
           "ics_tags": [1], "ecs_tags": [2], "membrane_tags": [4]}
    p = ProblemEMI(cfg)
    with pytest.raises(Exception, match="no library context"):
        FieldSampler(p, np.zeros((1, 2)))
    p.add_ionic_model("HH", stim_fun=g_syn)
    p.init_ionic_model()
    s = SolverEMI(p)
    s.solve()
    lm = p.local_mesh
    coords, cells = np.asarray(lm.coords), np.asarray(lm.cells)
    pts, _ = SR.case_points("delaunay2d_12", coords)          # the widened 17 x 13 grid on this mesh's box
    cell, w, margin = SR.locate_ref(coords, cells, pts)
    assert margin > 1e-11 and (cell < 0).sum() >= 10
    fs = FieldSampler(p, pts)
    _check_location(fs, p, cell, w, "EMI square8")
    phi_i, phi_e = p.wh[0].numpy(), p.wh[1].numpy()
    assert np.abs(phi_i).max() > 0
    got = fs([p.wh[0]], [p.wh[1]]).cpu().numpy()[0]
    want = SR.interpolate_ref(cells, p.cell_side, cell, w, phi_i, phi_e)
    ok = cell >= 0
    assert np.abs(got[ok] - want[ok]).max() <= 1e-13 * max(np.abs(phi_i).max(), np.abs(phi_e).max()) and np.isnan(got[~ok]).all()
    fs.close()
