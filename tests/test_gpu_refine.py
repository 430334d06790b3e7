"""Mesh refinement on the GPU (knp_refine_* in csrc/knp_refine.inc, cgx_hip/refine.py) against tests/refine_ref.py, the NumPy
restatement pinned by tests/test_refine_host.py: exact agreement array for array, the refusals, the prolongation kernel, the config
key ``refine_levels`` under both problem classes, and ``transfer_state`` from a mesh to its refinement."""
import copy
import os

import numpy as np
import pytest
import torch

import irregular_meshes as IM
import refine_ref as R
from cgx_hip import mesh as meshmod
from parity_utils import ci_config, make_problem, mms_config, run_native

pytestmark = pytest.mark.gpu

IRREGULAR = ["delaunay2d_12", "hub2d_12_300", "hub2d_12_48m_cw", "delaunay3d_5", "hub3d_5_140"]


def _box_facets(coords, cells, tags):
    """the membrane of the box, two values split at x = 0.5"""
    _, _, gverts = meshmod.gamma_integration_entities(cells, tags, (1,), (2,), None)
    return gverts, np.where(coords[gverts].mean(axis=1)[:, 0] < 0.5, 5, 6).astype(np.int32)


def _case(name):
    if name in IRREGULAR:
        coords, cells, tags = IM.mesh(name)
        return coords, cells, tags, _box_facets(coords, cells, tags)
    if name in ("cube2", "cube3"):
        coords, cells = meshmod.create_unit_cube(int(name[-1]))
        tags = meshmod.mark_subdomains_box(coords, cells, *((0.25, 0.75) if name == "cube2" else (0.3, 0.7)))
        ft = _box_facets(coords, cells, tags)
        assert name == "cube2" or len(ft[0]) > 0
        return coords, cells, tags, ft
    if name.startswith("tet"):
        if name == "tet_regular":
            X = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / 3.0
        else:
            p, q, r, t = R.DIAGONALS[int(name[-1])]
            X = np.zeros((4, 3))
            X[p], X[q], X[r], X[t] = (0.0, 0.0, 0.1), (1.0, 0.0, 0.1), (0.5, -0.5, -0.1), (0.5, 0.5, -0.1)
        return X, np.array([[0, 1, 2, 3]], dtype=np.int32), np.array([7], dtype=np.int32), (np.array([[3, 1, 2]]), np.array([9]))
    X = np.array([[0.0, 0.0], [1.0, 0.125], [0.25, 1.0], [1.5, 1.25]])
    if name == "triangle":
        return X[:3], np.array([[2, 0, 1]], dtype=np.int32), np.array([3], dtype=np.int32), None
    assert name == "two_triangles"
    return X, np.array([[0, 1, 2], [2, 3, 1]], dtype=np.int32), np.array([1, 2], dtype=np.int32), (np.array([[2, 1]]), np.array([4]))


def _assert_equal(rec, ref_levels):
    last = ref_levels[-1]
    assert rec.coords.dtype == np.float64 and np.array_equal(rec.coords.view(np.uint64), last["coords"].view(np.uint64))       # bit for bit
    assert np.array_equal(rec.cells, last["cells"]) and np.array_equal(rec.cell_tags, last["cell_tags"])
    if last["facet_tags"] is None or isinstance(last["facet_tags"], str):
        assert rec.facet_tags == last["facet_tags"]
    else:
        assert np.array_equal(rec.facet_tags[0], last["facet_tags"][0]) and np.array_equal(rec.facet_tags[1], last["facet_tags"][1])
    assert rec.levels == len(ref_levels) == len(rec.edge_vertices)
    for lv, r in enumerate(ref_levels):
        assert rec.edge_vertices[lv].is_cuda and np.array_equal(rec.edge_vertices[lv].cpu().numpy(), r["edge_vertices"])
        assert rec.n_coarse_vertices[lv] == len(r["coords"]) - len(r["edge_vertices"])
        if r["diagonal"] is None:
            assert rec.diagonal[lv] is None
        else:
            assert rec.diagonal[lv].dtype == np.uint8 and np.array_equal(rec.diagonal[lv], r["diagonal"])
        assert np.array_equal(rec.parent_cell(lv + 1), np.arange(len(r["cells"])) // 2 ** rec.dim)


CASES = IRREGULAR + ["cube2", "cube3", "tet_short0", "tet_short1", "tet_short2", "tet_regular", "triangle", "two_triangles"]


@pytest.mark.parametrize("name", CASES)
def test_device_equals_the_restatement(name):
    from cgx_hip.refine import refine
    coords, cells, tags, ft = _case(name)
    rec = refine(coords, cells, tags, ft, 1)
    _assert_equal(rec, R.refine(coords, cells, tags, ft, 1))
    if name.startswith("tet_short"):
        assert rec.diagonal[0].tolist() == [int(name[-1])]
    if name == "tet_regular":
        assert rec.diagonal[0].tolist() == [0]


@pytest.mark.parametrize("name,how", [("delaunay3d_5", "box"), ("delaunay2d_12", "intra"), ("hub2d_12_48m_cw", "box")])
def test_two_levels_equal_the_restatement(name, how):
    from cgx_hip.refine import refine
    coords, cells, tags, ft = _case(name)
    ft = "intra" if how == "intra" else ft
    rec = refine(coords, cells, tags, ft, 2)
    _assert_equal(rec, R.refine(coords, cells, tags, ft, 2))
    assert len(rec.cells) == len(cells) * 4 ** rec.dim


def test_zero_levels_return_the_mesh():
    from cgx_hip.refine import refine
    coords, cells, tags, ft = _case("two_triangles")
    rec = refine(coords, cells, tags, ft, 0)
    assert np.array_equal(rec.coords, coords) and np.array_equal(rec.cells, cells) and np.array_equal(rec.cell_tags, tags)
    assert rec.levels == 0 and rec.edge_vertices == []


@pytest.mark.parametrize("name", ["delaunay3d_5", "delaunay2d_12"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_around_the_launch_geometry(name, n):
    """blocks of 256 lanes, waves of 64: one lane, a wave less one, a full wave, one more, a block and one (no kernel caps its grid)"""
    from cgx_hip.refine import refine
    coords, cells, tags = IM.mesh(name)
    cells, tags = cells[:n], tags[:n]
    fv = meshmod.build_facets(cells)[0][:n]                                     # as many tagged facets as cells
    ft = (fv, np.arange(len(fv)) % 5)
    _assert_equal(refine(coords, cells, tags, ft, 1), R.refine(coords, cells, tags, ft, 1))


def test_child_cells_past_two_to_the_31_entries():
    """2^26 + 257 tetrahedra: the last children lie past entry 2^31 of the fine cell array (8.6 GB), where a 32-bit offset would wrap.
    The cells walk round 997 vertices, (i, i+1, i+2, i+3) mod 997, so the last 1024 of them have every edge of the mesh and the
    restatement of that tail alone gives their children; the kernel is called directly with the tail's unique keys."""
    from cgx_hip import _lib
    lib = _lib.load()
    dev = torch.device("cuda")
    nv, nc, tail = 997, 2 ** 26 + 257, 1024
    coords = np.random.default_rng(3).uniform(size=(nv, 3))
    i = torch.arange(nc, dtype=torch.int64, device=dev)
    cells = torch.stack([(i + k) % nv for k in range(4)], dim=1).to(torch.int32).contiguous()
    tags = (i % 5).to(torch.int32)
    del i
    host_tail = cells[nc - tail:].cpu().numpy()
    ref = R.refine_once(coords, host_tail, tags[nc - tail:].cpu().numpy())
    ukeys = torch.as_tensor(np.unique(R.edge_keys(host_tail, nv, R.EDGES[3])), device=dev)
    assert ukeys.numel() == 3 * nv == len(ref["edge_vertices"])
    fcells = torch.empty((nc * 8, 4), dtype=torch.int32, device=dev)
    assert fcells.numel() > 2 ** 31
    ftags = torch.empty(nc * 8, dtype=torch.int32, device=dev)
    diag = torch.empty(nc, dtype=torch.uint8, device=dev)
    fcells[-8 * tail:] = -1
    x = torch.as_tensor(coords, device=dev)
    rc = lib.knp_refine_cells(3, nc, nv, ukeys.numel(), ukeys.data_ptr(), cells.data_ptr(), tags.data_ptr(), x.data_ptr(), fcells.data_ptr(),
                              ftags.data_ptr(), diag.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert np.array_equal(fcells[-8 * tail:].cpu().numpy(), ref["cells"]) and np.array_equal(ftags[-8 * tail:].cpu().numpy(), ref["cell_tags"])
    assert np.array_equal(diag[-tail:].cpu().numpy(), ref["diagonal"])
    assert np.array_equal(fcells[:8 * tail].cpu().numpy()[:, 0] < nv, np.tile([True] + [False] * 7, tail))     # and the head is children, not wrapped tail
    assert lib.knp_refine_cells(3, 2 ** 28, nv, ukeys.numel(), ukeys.data_ptr(), cells.data_ptr(), tags.data_ptr(), x.data_ptr(), fcells.data_ptr(),
                                ftags.data_ptr(), diag.data_ptr(), None) == -1                                  # 2^31 fine cells: refused


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_a_tagged_facet_that_is_no_facet_of_the_mesh_is_refused_and_nothing_is_written_for_it():
    from cgx_hip.refine import refine, refine_facets_device
    coords, cells, tags, (fv, vals) = _case("delaunay3d_5")
    far = np.setdiff1d(np.arange(len(coords)), np.unique(cells[(cells == fv[5, 0]).any(axis=1)]))[0]
    bad = fv.copy()
    bad[5, 2] = far                                                              # an edge that no cell has
    second = len(fv) - 3
    assert second > 5
    bad[second, 1] = bad[second, 0]                                              # a vertex twice
    with pytest.raises(ValueError, match=r"\b2 tagged facets"):
        refine(coords, cells, tags, (bad, vals), 1)
    with pytest.raises(ValueError):
        R.refine(coords, cells, tags, (bad, vals), 1)
    # the kernel itself: the rows of the refused facets keep what was there, the others are the restatement's
    dev = torch.device("cuda")
    nv = len(coords)
    ukeys = torch.as_tensor(np.unique(R.edge_keys(cells, nv, R.EDGES[3])), device=dev)
    out = torch.full((len(fv) * 4, 3), -7, dtype=torch.int32, device=dev)
    oval = torch.full((len(fv) * 4,), -7, dtype=torch.int32, device=dev)
    _, _, missing = refine_facets_device(3, nv, ukeys, torch.as_tensor(bad.astype(np.int32), device=dev),
                                         torch.as_tensor(vals.astype(np.int32), device=dev), out, oval)
    assert missing == 2
    good = R.refine_once(coords, cells, tags, (fv, vals))["facet_tags"]
    out, oval = out.cpu().numpy().reshape(-1, 4, 3), oval.cpu().numpy().reshape(-1, 4)
    keep = np.ones(len(fv), dtype=bool)
    keep[[5, second]] = False
    assert (out[~keep] == -7).all() and (oval[~keep] == -7).all()
    assert np.array_equal(out[keep], good[0].reshape(-1, 4, 3)[keep]) and np.array_equal(oval[keep], good[1].reshape(-1, 4)[keep])


@pytest.mark.parametrize("name", ["delaunay2d_12", "delaunay3d_5"])
@pytest.mark.parametrize("what", ["past_the_end", "negative", "twice"])
def test_bad_cells_are_refused(name, what):
    from cgx_hip.refine import refine
    coords, cells, tags = IM.mesh(name)
    bad = cells.copy()
    bad[130, 1] = {"past_the_end": len(coords), "negative": -1, "twice": bad[130, 2]}[what]
    with pytest.raises(ValueError, match="out of range or the same vertex twice"):
        refine(coords, bad, tags, None, 1)


@pytest.mark.parametrize("n", [-1, 1.5, "2", True])
def test_refine_levels_must_be_a_non_negative_integer(n):
    cfg = ci_config(N=8, steps=1)
    cfg["refine_levels"] = n
    with pytest.raises(ValueError, match="refine_levels"):
        make_problem(cfg)


def test_refine_levels_is_refused_for_mms_meshes_and_local_mesh_overrides():
    cfg = mms_config(dim=2, N=8)
    cfg["refine_levels"] = 1
    with pytest.raises(ValueError, match="MMS"):
        make_problem(cfg)
    p = make_problem(ci_config(N=8, steps=1))
    cfg = ci_config(N=8, steps=1)
    cfg["refine_levels"] = 1
    with pytest.raises(ValueError, match="local_mesh"):
        make_problem(cfg, local_mesh=p.local_mesh)


# ---- prolongation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["delaunay2d_12", "delaunay3d_5"])
@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("n_fields", [1, 9])
def test_prolongation_kernel_equals_the_restatement(name, levels, n_fields):
    from cgx_hip.refine import refine
    coords, cells, tags = IM.mesh(name)
    rec = refine(coords, cells, tags, None, levels)
    ref = R.refine(coords, cells, tags, None, levels)
    f = np.random.default_rng(5).standard_normal((n_fields, len(coords))) * 10.0 ** np.arange(-4, n_fields - 4)[:, None]
    want = np.stack([R.prolong(ref, row) for row in f])
    fd = torch.as_tensor(f, device="cuda")
    got = rec.prolong(fd)
    assert got.is_cuda and got.shape == want.shape and np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64))
    as_list = rec.prolong([fd[k] for k in range(n_fields)])
    assert len(as_list) == n_fields and all(np.array_equal(a.cpu().numpy(), w) for a, w in zip(as_list, want))
    out = torch.full(want.shape, np.nan, dtype=torch.float64, device="cuda")
    assert rec.prolong(fd, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(rec.restrict(got).cpu().numpy(), f)
    one = rec.prolong(fd[0])
    assert one.shape == (want.shape[1],) and np.array_equal(one.cpu().numpy(), want[0])


# ---- the config key ---------------------------------------------------------------------------------------------------------------
def test_refined_square8_gives_the_solution_of_square16():
    """The same mesh with another numbering of vertices and cells -- the situation of test_morton_vertex_order_gives_the_same_solution,
    whose tolerances these are: two converged solves, not bit for bit."""
    s0 = run_native(ci_config(N=16, steps=2, rtol=1e-12))
    cfg = ci_config(N=8, steps=2, rtol=1e-12)
    cfg["refine_levels"] = 1
    s1 = run_native(cfg)
    p0, p1 = s0.problem, s1.problem
    assert "refined 1×" in p1.mesh_description and p1.refinement.levels == 1 and p0.refinement is None
    assert all(r > 0 for r in s0.reasons) and all(r > 0 for r in s1.reasons)

    def order(p):
        q = np.rint(p.local_mesh.coords / 1e-6 * 16).astype(np.int64)
        assert np.abs(q - p.local_mesh.coords / 1e-6 * 16).max() < 1e-9
        return np.argsort(q[:, 1] * 17 + q[:, 0])
    o0, o1 = order(p0), order(p1)
    assert len(o0) == len(o1) == 17 * 17 and np.allclose(p0.local_mesh.coords[o0], p1.local_mesh.coords[o1], rtol=1e-14, atol=0)
    pot_scale = np.abs(p0.wh[0][3].numpy()).max()
    for side in (0, 1):
        for f in range(4):
            a, b = p0.wh[side][f].numpy()[o0], p1.wh[side][f].numpy()[o1]
            tol = 1e-6 * pot_scale if f == 3 else 1e-7 * max(np.abs(a).max(), 1e-300)
            print(f"side {side} field {f}: max difference {np.abs(a - b).max():.3e}, tolerance {tol:.3e}")
            assert np.abs(a - b).max() <= tol, (side, f, np.abs(a - b).max(), tol)
    pm0, pm1 = p0.phi_m_prev.numpy()[o0], p1.phi_m_prev.numpy()[o1]
    assert np.abs(pm0 - pm1).max() <= 1e-6 * np.abs(pm0).max()
    n0, n1 = s0.potential_norms(), s1.potential_norms()
    assert abs(n0[0] - n1[0]) <= 1e-6 * n0[0] and abs(n0[1] - n1[1]) <= 1e-6 * n0[0]


def test_refined_3d_mesh_runs_and_keeps_volumes_and_areas(tmp_path):
    """delaunay3d_5 with two cells whose membranes carry the cells' tags in the file: the facet tags go through the refinement too, and
    ``ion_budget`` has an area for every intracellular tag"""
    cfg = IM.two_tag_config(tmp_path, steps=1)
    p0 = make_problem(copy.deepcopy(cfg))
    cfg["refine_levels"] = 1
    s1 = run_native(cfg)
    p1 = s1.problem
    assert all(r > 0 for r in s1.reasons) and "refined 1×" in p1.mesh_description
    assert p1.mesh.num_cells == 8 * p0.mesh.num_cells and len(p1.gamma_entities) == 4 * len(p0.gamma_entities)
    b0, b1 = p0.ion_budget(), p1.ion_budget()
    assert np.array_equal(b0["tag"], b1["tag"]) and (b0["area"][b0["side"] == 0] > 0).all() and (b0["volume"] > 0).all()
    for key in ("volume", "area"):
        print(key, b0[key], np.abs(b1[key] - b0[key]) / np.maximum(b0[key], 1e-300))
        assert (np.abs(b1[key] - b0[key]) <= 1e-11 * b0[key]).all(), key


def test_refined_mesh_under_the_emi_problem(tmp_path):
    from test_gpu_emi import _config, _run
    path = IM.write_npz(tmp_path, "delaunay2d_12", *IM.mesh("delaunay2d_12"))
    cfg = _config("delaunay2d_12", time_steps=2, cell_tag_file=path, facet_tag_file=path, input_dir="", refine_levels=1)
    s = _run("delaunay2d_12", 2, config=cfg)
    p = s.problem
    assert "refined 1×" in p.mesh_description and p.mesh.num_cells == 4 * len(IM.mesh("delaunay2d_12")[1])
    assert len(s.reasons) == 2 and all(r > 0 for r in s.reasons)


# ---- state transfer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["native", "morton"])
def test_transfer_state_carries_a_coarse_run_to_the_refined_problem(order, tmp_path):
    from cgx_hip.refine import transfer_state
    cfg = IM.config(tmp_path, "delaunay2d_12", steps=2)
    s0 = run_native(copy.deepcopy(cfg))
    p0 = s0.problem
    assert all(r > 0 for r in s0.reasons) and hasattr(p0, "n")
    cfg["refine_levels"] = 1
    if order == "morton":
        cfg["vertex_order"] = "morton"
    p1 = make_problem(cfg)
    assert (order == "morton") == ("Morton" in p1.mesh_description)
    before = p1.wh[0][0].numpy().copy()
    gc, gf = np.argsort(p0.local_mesh.l2g), np.argsort(p1.local_mesh.l2g)
    nvc = p0.mesh.num_vertices
    pairs = [(p0.wh[s][f], p1.wh[s][f]) for s in (0, 1) for f in range(4)] + [(p0.phi_m_prev, p1.phi_m_prev), (p0.n, p1.n), (p0.m, p1.m), (p0.h, p1.h)]

    def transfer_and_compare(what):
        transfer_state(p0, p1)
        assert not np.array_equal(before, p1.wh[0][0].numpy())
        for a, b in pairs:            # at the coarse vertices the fine problem holds the coarse values, function by function
            assert np.array_equal(a.numpy()[gc], b.numpy()[gf][:nvc]), a.name
        m0, m1 = p0.membrane_potential(), p1.membrane_potential()
        assert np.array_equal(m0["tag"], m1["tag"]) and np.isfinite(m0["mean"]).all()
        print(what, "phi_m mean", m0["mean"], m1["mean"], "min", m0["min"], m1["min"], "max", m0["max"], m1["max"])
        assert (np.abs(m1["mean"] - m0["mean"]) <= 1e-11 * np.abs(m0["mean"])).all()
        assert np.array_equal(m0["min"], m1["min"]) and np.array_equal(m0["max"], m1["max"])
        b0, b1 = p0.ion_budget(), p1.ion_budget()
        for key in ("Na", "K", "Cl"):
            print(what, key, b0[key], np.abs(b1[key] - b0[key]) / np.abs(b0[key]))
            assert (np.abs(b1[key] - b0[key]) <= 1e-11 * np.abs(b0[key])).all(), key
        return m0
    transfer_and_compare("after two steps:")
    # two steps from uniform initial conditions leave the fields nearly uniform: the same again from a state that varies in space, with
    # another factor for every function, so that a function carried into the wrong place or with the wrong numbering shows
    X = torch.as_tensor(p0.local_mesh.coords / p0.local_mesh.coords.max(), device=p0.mesh.device)
    for k, (a, _) in enumerate(pairs):
        a.x.array *= 1.0 + 0.01 * (k + 1) * torch.sin(3.0 * X[:, 0] + 1.0 + k) * torch.cos(2.0 * X[:, 1] + 0.5)
    m0 = transfer_and_compare("perturbed:")
    assert (m0["max"] - m0["min"] > 1e-3 * np.abs(m0["mean"])).all()


def test_transfer_state_refuses_what_it_cannot_match(tmp_path):
    from cgx_hip.refine import transfer_state
    cfg = IM.config(tmp_path, "delaunay2d_12", steps=1)
    p0 = make_problem(copy.deepcopy(cfg))
    with pytest.raises(ValueError, match="refine_levels"):
        transfer_state(p0, make_problem(copy.deepcopy(cfg)))
    cfg["refine_levels"] = 1
    with pytest.raises(ValueError, match="gates"):
        transfer_state(p0, make_problem(copy.deepcopy(cfg), models="passive"))
    other = ci_config(N=8, steps=1)
    other["refine_levels"] = 1
    with pytest.raises(ValueError, match="vertices"):
        transfer_state(p0, make_problem(other))


# ---- the reference's command line ------------------------------------------------------------------------------------------------
def test_refine_mesh_script_writes_the_refined_files(tmp_path):
    from cgx_hip import xdmf
    from CGx.utils.refine_mesh import main
    coords, cells, tags, (fv, vals) = _case("delaunay3d_5")
    d = str(tmp_path) + os.sep
    xdmf.write_mesh_and_tags(d + "tissue.xdmf", coords, cells, tags, fv, vals)
    main([d, "tissue.xdmf", "tissue.xdmf", "--levels", "2"])
    got = xdmf.read_mesh_and_tags(d + "tissue_refined.xdmf", d + "tissue_refined.xdmf")
    want = R.refine(coords, cells, tags, (fv, vals), 2)[-1]
    assert np.array_equal(got[0], want["coords"]) and np.array_equal(got[1], want["cells"]) and np.array_equal(got[2], want["cell_tags"])
    assert np.array_equal(got[3][0], want["facet_tags"][0]) and np.array_equal(got[3][1], want["facet_tags"][1])
