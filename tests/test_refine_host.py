"""The NumPy restatement of the red refinement (tests/refine_ref.py) checked on its own, because tests/test_gpu_refine.py trusts it:
conformity, volumes, orientation, the diagonal rule, tag transfer, prolongation, and the XDMF files the refined meshes are written to."""
import os

import numpy as np
import pytest

import irregular_meshes as IM
import refine_ref as R
from cgx_hip import mesh as meshmod

IRREGULAR = ["delaunay2d_12", "hub2d_12_300", "hub2d_12_48m_cw", "delaunay3d_5", "hub3d_5_140"]


def _cube2():
    coords, cells = meshmod.create_unit_cube(2)
    return coords, cells, meshmod.mark_subdomains_box(coords, cells)


def _mesh(name):
    return _cube2() if name == "cube2" else IM.mesh(name)


@pytest.fixture(scope="module")
def refined():
    cache = {}

    def get(name):
        if name not in cache:
            coords, cells, tags = _mesh(name)
            cache[name] = (coords, cells, tags, R.refine_once(coords, cells, tags))
        return cache[name]
    return get


@pytest.mark.parametrize("name", IRREGULAR + ["cube2"])
def test_fine_mesh_is_conforming_and_fills_the_parents(name, refined):
    coords, cells, tags, r = refined(name)
    dim = coords.shape[1]
    fc, fx = r["cells"], r["coords"]
    fverts, c0, l0, c1, l1 = meshmod.build_facets(fc)
    # a facet is in one cell (boundary) or two; three or more would show up as a facet listed twice by build_facets' pairing
    table, _, _ = meshmod._facet_table(fc)
    _, counts = np.unique(table, axis=0, return_counts=True)
    assert counts.max() == 2 and len(counts) == len(fverts)
    n_bnd_coarse = len(meshmod.exterior_facets(cells)[0])
    assert int((c1 < 0).sum()) == 2 ** (dim - 1) * n_bnd_coarse
    assert np.array_equal(np.unique(fc), np.arange(len(fx)))                          # every fine vertex is used
    v, fv = R.signed_volumes(coords, cells), R.signed_volumes(fx, fc)
    assert np.array_equal(np.sign(fv), np.repeat(np.sign(v), 2 ** dim))               # the parent's orientation
    err = np.abs(fv.reshape(len(cells), -1).sum(axis=1) - v) / np.abs(v)
    print(f"{name}: max relative volume defect {err.max():.2e}")
    assert err.max() <= 1e-12
    assert np.array_equal(r["cell_tags"], np.repeat(tags, 2 ** dim))
    ev = r["edge_vertices"]
    assert (ev[:, 0] < ev[:, 1]).all() and np.array_equal(fx[len(coords):], (coords[ev[:, 0]] + coords[ev[:, 1]]) * 0.5)


def test_all_three_diagonals_occur(refined):
    diag = refined("delaunay3d_5")[3]["diagonal"]
    counts = np.bincount(diag, minlength=3)
    print("delaunay3d_5 diagonals:", counts)
    assert (counts > 0).all() and counts.sum() == len(diag)
    assert counts.tolist() == [269, 295, 275]                  # what the rule gives on this mesh: a changed rule or table order shows here


def _tet_with_shortest(k):
    """a tetrahedron whose candidate ``k`` is clearly the shortest diagonal: the two edges that diagonal joins are brought together"""
    p, q, r, t = R.DIAGONALS[k]
    X = np.zeros((4, 3))
    X[p], X[q] = (0.0, 0.0, 0.1), (1.0, 0.0, 0.1)             # edge p-q and edge r-t cross at a distance of 0.2: midpoints 0.2 apart
    X[r], X[t] = (0.5, -0.5, -0.1), (0.5, 0.5, -0.1)
    return X, np.array([[0, 1, 2, 3]])


@pytest.mark.parametrize("k", [0, 1, 2])
def test_single_tetrahedra_take_their_shortest_diagonal(k):
    X, cells = _tet_with_shortest(k)
    r = R.refine_once(X, cells, np.array([1]))
    assert r["diagonal"].tolist() == [k]
    inner = r["cells"][4:]
    p, q, rr, t = R.DIAGONALS[k]
    key = lambda a, b: min(a, b) * 4 + max(a, b)
    ukeys = np.unique(R.edge_keys(cells, 4, R.EDGES[3]))
    ends = {4 + int(np.searchsorted(ukeys, key(p, q))), 4 + int(np.searchsorted(ukeys, key(rr, t)))}
    assert all(ends <= set(c.tolist()) for c in inner)                               # the four inner children share the diagonal
    v = R.signed_volumes(r["coords"], r["cells"])
    assert np.array_equal(np.sign(v), np.full(8, np.sign(R.signed_volumes(X, cells)[0])))
    assert abs(v.sum() - R.signed_volumes(X, cells)[0]) <= 1e-15


def test_regular_tetrahedron_is_a_tie_and_gives_candidate_zero():
    X = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / 3.0
    for perm in ([0, 1, 2, 3], [3, 1, 0, 2], [2, 0, 3, 1]):
        r = R.refine_once(X[perm] * 0.7 + 0.1, np.array([[0, 1, 2, 3]]), np.array([1]))
        assert r["diagonal"].tolist() == [0]


def _box_gamma(coords, cells, tags, facet_tags=None):
    return meshmod.gamma_integration_entities(cells, tags, (1,), (2,), facet_tags)


@pytest.mark.parametrize("name", IRREGULAR + ["cube2"])
def test_membrane_facets_and_their_tags_are_carried_to_the_children(name):
    coords, cells, tags = _mesh(name)
    dim = coords.shape[1]
    _, _, gverts = _box_gamma(coords, cells, tags)
    # two membrane tags, split at x = 0.5, so that the transfer of the VALUES is seen
    vals = np.where(coords[gverts].mean(axis=1)[:, 0] < 0.5, 5, 6).astype(np.int32)
    r = R.refine_once(coords, cells, tags, (gverts, vals))
    fv, fvals = r["facet_tags"]
    assert len(fv) == 2 ** (dim - 1) * len(gverts)
    gam, gtags, gv = _box_gamma(r["coords"], r["cells"], r["cell_tags"], (fv, fvals))
    assert len(gam) == 2 ** (dim - 1) * len(gverts) and (gtags > 0).all()            # every membrane facet of the fine mesh found its tag
    allf = {tuple(f) for f in meshmod.build_facets(r["cells"])[0].tolist()}
    assert all(tuple(f) in allf for f in np.sort(fv, axis=1).tolist())               # every child is a facet of the fine mesh
    for t in (5, 6):
        a0 = R.facet_measures(coords, gverts[vals == t]).sum()
        a1 = R.facet_measures(r["coords"], gv[gtags == t]).sum()
        assert abs(a1 - a0) <= 1e-12 * a0, (t, a0, a1)


def test_a_tagged_facet_that_is_no_facet_of_the_mesh_is_refused():
    coords, cells, tags = IM.mesh("delaunay2d_12")
    far = np.array([[int(cells[0, 0]), int(np.setdiff1d(np.arange(len(coords)), np.unique(cells[(cells == cells[0, 0]).any(axis=1)]))[0])]])
    with pytest.raises(ValueError, match="1 tagged facets"):
        R.refine_once(coords, cells, tags, (far, np.array([4])))
    bad = cells.copy()
    bad[3, 1] = bad[3, 0]
    with pytest.raises(ValueError):
        R.refine_once(coords, bad, tags)
    bad = cells.copy()
    bad[3, 1] = len(coords)
    with pytest.raises(ValueError):
        R.refine_once(coords, bad, tags)


def test_refined_square8_is_square16():
    c8, t8 = meshmod.create_unit_square(8)
    r = R.refine_once(c8, t8, meshmod.mark_subdomains_box(c8, t8))
    c16, t16 = meshmod.create_unit_square(16)
    g16 = meshmod.mark_subdomains_box(c16, t16)

    def keyed(coords, cells, tags):
        q = np.rint(coords * 16).astype(np.int64)
        assert np.array_equal(q / 16.0, coords)
        vid = q[:, 1] * 17 + q[:, 0]
        return {tuple(sorted(row)) + (int(t),) for row, t in zip(vid[cells].tolist(), tags.tolist())}
    assert keyed(r["coords"], r["cells"], r["cell_tags"]) == keyed(c16, t16, g16)


@pytest.mark.parametrize("name,levels", [("delaunay2d_12", 1), ("delaunay3d_5", 1), ("delaunay3d_5", 2), ("hub2d_12_48m_cw", 2)])
def test_prolongation_reproduces_linear_functions(name, levels):
    coords, cells, tags = IM.mesh(name)
    lv = R.refine(coords, cells, tags, None, levels)
    w = np.array([0.7, -1.3, 2.1])[:coords.shape[1]]
    f = coords @ w + 0.25
    g = R.prolong(lv, f)
    exact = lv[-1]["coords"] @ w + 0.25
    assert g.shape == exact.shape and np.array_equal(g[:len(f)], f)
    assert np.abs(g - exact).max() <= 1e-15 * (f.max() - f.min())


@pytest.mark.parametrize("name", ["hub2d_12_48m_cw", "delaunay3d_5"])
def test_xdmf_round_trip_of_a_refined_mesh(name, tmp_path):
    from cgx_hip import xdmf
    coords, cells, tags = IM.mesh(name)
    _, _, gverts = _box_gamma(coords, cells, tags)
    vals = np.where(coords[gverts].mean(axis=1)[:, 0] < 0.5, 5, 6).astype(np.int32)
    r = R.refine_once(coords, cells, tags, (gverts, vals))
    path = os.path.join(str(tmp_path), name + "_refined.xdmf")
    xdmf.write_mesh_and_tags(path, r["coords"], r["cells"], r["cell_tags"], r["facet_tags"][0], r["facet_tags"][1])
    assert os.path.exists(path) and os.path.exists(path[:-5] + ".h5")
    c2, k2, t2, (f2, v2) = xdmf.read_mesh_and_tags(path, path)
    assert np.array_equal(c2, r["coords"]) and np.array_equal(k2, r["cells"]) and np.array_equal(t2, r["cell_tags"])
    assert np.array_equal(f2, r["facet_tags"][0]) and np.array_equal(v2, r["facet_tags"][1])
    # and through load_mesh, the way a config names the file
    c3, k3, t3, ft3, desc = meshmod.load_mesh(path, path, 1e-6)
    assert np.array_equal(c3, r["coords"] * 1e-6) and np.array_equal(k3, r["cells"]) and np.array_equal(ft3[1], r["facet_tags"][1])


def test_refinement_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from cgx_hip._lib import KnpError
    from cgx_hip.refine import refine
    from parity_utils import ci_config, make_problem
    with pytest.raises(KnpError, match="no CPU fallback"):
        refine(*IM.mesh("delaunay2d_12"), None, 1)
    cfg = ci_config(N=8, steps=1)
    cfg["refine_levels"] = 1
    with pytest.raises(KnpError):
        make_problem(cfg)
