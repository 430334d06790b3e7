"""Host side of the field sampling (cgx_hip/sampling.py, the ``sample_grids`` keys of cgx_hip/output.py): the reference of the GPU
tests (tests/sampling_ref.py) against ``output._barycentric``, the binning handed to the library, the grid generator, the config
errors, and the conditions on the inputs of tests/test_gpu_sampling.py.  CPU only."""
import numpy as np
import pytest

import sampling_ref as SR


@pytest.fixture(scope="module")
def problems(tmp_path_factory):
    from cgx_hip.problem import ProblemKNPEMI
    cache = {}
    tmp = tmp_path_factory.mktemp("sampling_meshes")

    def get(mesh):
        if mesh not in cache:
            cache[mesh] = ProblemKNPEMI(SR.mesh_config(mesh, tmp))
        return cache[mesh]
    return get


@pytest.mark.parametrize("case", sorted(SR.CASES))
def test_reference_agrees_with_barycentric_and_the_inputs_are_well_posed(case, problems):
    from cgx_hip.output import _barycentric
    p = problems(SR.CASES[case][0])
    lm = p.local_mesh
    pts, grid, cell, w, margin = SR.case_reference(case, p)
    c0, w0 = _barycentric(np.asarray(lm.coords), np.asarray(lm.cells), pts)
    print(f"{case}: {pts.shape[0]} points, found {(cell >= 0).sum()}, margin {margin:.3e}, "
          f"max |w_ref - w_barycentric| = {np.abs(w - w0).max():.3e}")
    assert np.array_equal(cell, c0)
    assert np.abs(w - w0).max() <= 1e-12
    assert np.allclose(w[cell >= 0].sum(axis=1), 1.0, rtol=0, atol=4e-16) and w.min() >= 0.0 and w.max() <= 1.0
    assert np.all(w[cell < 0] == 0.0)
    # no weight of any (point, cell) pair within 1e-11 of the threshold: rounding cannot change a winner
    assert margin > 1e-11


@pytest.mark.parametrize("case", SR.IRREGULAR)
def test_irregular_cases_cover_inside_outside_and_both_sides(case, problems):
    p = problems(case)
    pts, grid, cell, w, _ = SR.case_reference(case, p)
    found = cell >= 0
    intra = int((p.cell_side[cell[found]] == 0).sum())
    print(f"{case}: found {found.sum()} of {found.size}, outside {(~found).sum()}, in intracellular cells {intra}")
    assert found.sum() >= found.size / 4 and intra >= 10 and (~found).sum() >= 10
    if case == "delaunay2d_12":
        assert (found.size, int(found.sum()), intra) == (221, 165, 35)
    if case == "delaunay3d_5":
        assert (found.size, int(found.sum()), intra) == (315, 105, 20)


def test_the_tie_cases_are_ties(problems):
    """every interior point of the vertex-aligned grid on square 8 lies in more than one cell; so does the centre point of the hub meshes"""
    p = problems("square8")
    lm = p.local_mesh
    pts, _, cell, _, _ = SR.case_reference("square8_aligned", p)
    hits = np.zeros(pts.shape[0], dtype=int)
    for c in range(lm.cells.shape[0]):
        hits += np.all(SR.pair_weights(lm.coords, lm.cells[c], pts) >= -SR.TOL, axis=1)
    assert hits.reshape(17, 17)[1:-1, 1:-1].min() >= 2 and hits.min() >= 1 and np.all(cell >= 0)      # (the outer boundary: one cell at an edge midpoint)
    sides = p.cell_side[cell].reshape(17, 17)
    assert sides[8, 8] == 0 and sides[0, 0] == 1 and set(np.unique(sides)) == {0, 1}
    for name in ("hub2d_12_40", "hub3d_5_60"):
        q = problems(name)
        pts, grid, cell, _, _ = SR.case_reference(name, q)
        mid = int(np.ravel_multi_index(tuple(s // 2 for s in grid[2]), grid[2]))
        n_in = sum(bool(np.all(SR.pair_weights(q.local_mesh.coords, cc, pts[mid:mid + 1]) >= -SR.TOL)) for cc in q.local_mesh.cells)
        assert n_in > 2 and cell[mid] >= 0


@pytest.mark.parametrize("case", sorted(SR.CASES))
def test_binning_puts_every_point_in_exactly_one_bin(case, problems):
    from cgx_hip.sampling import bin_points
    p = problems(SR.CASES[case][0])
    pts, _ = SR.case_points(case, np.asarray(p.local_mesh.coords))
    b = bin_points(pts)
    n, dim = pts.shape
    nb = int(np.prod(b["shape"]))
    assert b["bin_ptr"].shape == (nb + 1,) and b["bin_ptr"][0] == 0 and b["bin_ptr"][-1] == n
    assert np.all(np.diff(b["bin_ptr"]) >= 0)
    assert sorted(b["bin_pts"]) == list(range(n))
    assert np.all(b["size"] > 0) and np.all(b["shape"] >= 1) and nb <= 4 * n + 64
    # the bin a point is listed in is the one the documented formula gives
    idx = np.clip(np.floor((pts - b["origin"]) / b["size"]), 0, b["shape"] - 1).astype(np.int64)
    lin = np.ravel_multi_index(tuple(idx.T), tuple(int(s) for s in b["shape"]))
    listed = np.repeat(np.arange(nb), np.diff(b["bin_ptr"]))
    assert np.array_equal(lin[b["bin_pts"]], listed)
    # every point lies inside its bin's box (the end of an axis is clamped into the last bin)
    lo = b["origin"] + idx * b["size"]
    assert np.all(pts >= lo) and np.all((pts <= lo + b["size"] * (1 + 1e-12)) | (idx == b["shape"] - 1))


def test_binning_of_degenerate_sets():
    from cgx_hip.sampling import bin_points
    one = bin_points(np.array([[1e-6, 2e-6, 3e-6]]))
    assert list(one["shape"]) == [1, 1, 1] and list(one["bin_ptr"]) == [0, 1] and np.all(one["size"] > 0)
    same = bin_points(np.tile([[0.0, 5e-6]], (7, 1)))
    assert list(same["shape"]) == [1, 1] and list(same["bin_ptr"]) == [0, 7]
    rng = np.random.default_rng(3)
    plane = np.column_stack([rng.uniform(0, 1e-4, 500), np.full(500, 2.5e-5), rng.uniform(0, 3e-4, 500)])
    b = bin_points(plane)
    assert b["shape"][1] == 1 and b["size"][1] < 1e-18 and 100 <= int(np.prod(b["shape"])) <= 500


def test_grid_generator_gives_the_documented_lattice():
    from cgx_hip.sampling import grid_points
    o = np.array([1.0, -2.0, 0.5])
    ax = np.array([[2.0, 0.0, 1.0], [0.0, 3.0, -1.0]])
    xyz = grid_points(o, ax, (5, 4))
    assert xyz.shape == (5, 4, 3)
    for i in range(5):
        for j in range(4):
            assert np.allclose(xyz[i, j], o + i / 4 * ax[0] + j / 3 * ax[1], rtol=0, atol=1e-15)
    assert np.array_equal(xyz[0, 0], o) and np.allclose(xyz[-1, -1], o + ax[0] + ax[1], rtol=0, atol=1e-15)
    line = grid_points([0.0, 0.0], [[1.0, 1.0]], [3])
    assert np.array_equal(line, [[0.0, 0.0], [0.5, 0.5], [1.0, 1.0]])
    vol = grid_points(np.zeros(3), np.eye(3), (2, 3, 4))
    assert vol.shape == (2, 3, 4, 3) and np.array_equal(vol[1, 2, 3], [1.0, 1.0, 1.0]) and np.array_equal(vol[0, 1, 0], [0.0, 0.5, 0.0])
    for bad in (dict(axes=[[1.0, 0.0]], shape=(2, 2)), dict(axes=[[1.0, 0.0], [0.0, 1.0]], shape=(1, 3)),
                dict(axes=[[0.0, 0.0]], shape=(3,)), dict(axes=np.ones((4, 2)), shape=(2, 2, 2, 2))):
        with pytest.raises(ValueError):
            grid_points(np.zeros(2), bad["axes"], bad["shape"])


GOOD = {"name": "mid", "origin": [0, 0, 0.5], "axes": [[1, 0, 0], [0, 1, 0]], "shape": [5, 4], "fields": ["K", "phi"]}


def _parse(grids, **more):
    from cgx_hip.output import parse_sample_grids
    return parse_sample_grids(dict({"sample_grids": grids}, **more), 3, 1e-6, 20, 100)


def test_output_keys_parse():
    from cgx_hip.output import parse_sample_grids
    assert parse_sample_grids({}, 3, 1e-6, 20, 100) == ([], 20)
    assert parse_sample_grids({"sample_interval": 7}, 2, 1.0, 20, 100) == ([], 7)
    (e,), interval = _parse([GOOD], sample_interval=10)
    assert interval == 10 and e["name"] == "mid" and e["shape"] == (5, 4) and e["fields"] == ["K", "phi"] and e["records"] == 11
    assert np.array_equal(e["origin"], [0.0, 0.0, 0.5e-6]) and np.array_equal(e["axes"], [[1e-6, 0, 0], [0, 1e-6, 0]])
    (d,), interval = _parse([{k: v for k, v in GOOD.items() if k != "fields"}])
    assert interval == 20 and d["fields"] == ["Na", "K", "Cl", "phi"] and d["records"] == 6


@pytest.mark.parametrize("what,change,word", [
    ("duplicate name", None, "twice"),
    ("axes count", {"shape": [5, 4, 3]}, "2 axes but 3"),
    ("one point on an axis", {"shape": [5, 1]}, "two points"),
    ("zero axis", {"axes": [[1, 0, 0], [0, 0, 0]]}, "zero vector"),
    ("unknown field", {"fields": ["K", "Ca"]}, "Ca"),
])
def test_invalid_entries_raise_and_name_the_entry(what, change, word):
    grids = [GOOD, dict(GOOD)] if change is None else [dict(GOOD, **change)]
    with pytest.raises(ValueError) as e:
        _parse(grids)
    assert "'mid'" in str(e.value) and word in str(e.value), str(e.value)


def test_other_invalid_keys_raise():
    with pytest.raises(ValueError, match="sample_interval"):
        _parse([GOOD], sample_interval=0)
    with pytest.raises(ValueError, match=r"sample_grids\[0\]"):
        _parse([{"origin": [0, 0, 0]}])
    with pytest.raises(ValueError, match="missing key 'axes'"):
        _parse([{k: v for k, v in GOOD.items() if k != "axes"}])
    with pytest.raises(ValueError, match="3 components"):
        _parse([dict(GOOD, origin=[0, 0])])


def test_a_buffer_over_one_gibibyte_is_refused_with_its_size():
    from cgx_hip.output import parse_sample_grids
    big = dict(GOOD, shape=[2048, 2048], fields=["Na", "K", "Cl", "phi"])
    with pytest.raises(ValueError) as e:          # 11 records x 4 fields x 2048^2 x 8 B = 1.375 GiB
        parse_sample_grids({"sample_grids": [big], "sample_interval": 10}, 3, 1e-6, 20, 100)
    assert str(8 * 11 * 4 * 2048 * 2048) in str(e.value) and "sample_interval" in str(e.value) and "'mid'" in str(e.value)
    (ok,), _ = parse_sample_grids({"sample_grids": [big], "sample_interval": 20}, 3, 1e-6, 20, 100)     # 6 records: 0.75 GiB
    assert ok["records"] == 6


def test_solver_reads_the_keys_and_more_than_one_rank_is_refused(problems):
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    from cgx_hip.sampling import FieldSampler
    p = problems("cube4")
    cfg = dict(p.solver_config)
    cfg["output"] = dict(cfg.get("output", {}), sample_grids=[GOOD], sample_interval=2)
    s = SolverKNPEMI(p, solver_config=cfg)
    assert s.sample_interval == 2 and s.sample_grids[0]["records"] == p.time_steps // 2 + 1
    assert SolverKNPEMI(p, solver_config=p.solver_config).sample_grids == []
    cfg["output"]["sample_grids"] = [dict(GOOD, fields=["Zn"])]
    with pytest.raises(ValueError, match="Zn"):
        SolverKNPEMI(p, solver_config=cfg)

    class TwoRanks:
        size, rank = 2, 0
    comm, p.comm = p.comm, TwoRanks()
    try:
        with pytest.raises(NotImplementedError, match="field sampling"):
            FieldSampler(p, np.zeros((1, 3)))
    finally:
        p.comm = comm
