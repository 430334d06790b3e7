"""The irregular meshes of tests/irregular_meshes.py are valid input and have the properties the GPU tests of
tests/test_gpu_irregular.py rest on (no GPU here): a failure there is then the kernels', not the mesh's."""
import numpy as np
import pytest

import irregular_meshes as IM

ALL = list(IM.MESHES)
HUBS = {"hub2d_12_40": (0.5, 0.5), "hub2d_12_48m": IM.MEMBRANE_HUB, "hub2d_12_300": (0.5, 0.5),
        "hub3d_5_60": (0.5, 0.5, 0.5), "hub3d_5_140": (0.5, 0.5, 0.5)}


@pytest.fixture(scope="module")
def oracles():
    cache = {}

    def get(name):
        if name not in cache:
            o = IM.oracle(name)
            IM.perturb(o)
            cache[name] = o
        return cache[name]
    return get


@pytest.mark.parametrize("name", ALL)
def test_generators_are_deterministic_and_renumbered(name):
    a = IM.mesh(name)
    b = IM.MESHES[name]()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    coords, cells, tags = a
    assert cells.dtype == np.int32 and cells.min() == 0 and cells.max() == coords.shape[0] - 1
    assert len(np.unique(cells)) == coords.shape[0] and set(np.unique(tags)) == {1, 2}
    # not the lexicographic numbering of the generated grids: the coordinates are not sorted along any axis order
    assert not np.array_equal(np.lexsort(coords.T), np.arange(coords.shape[0]))
    assert not np.array_equal(np.lexsort(coords.T[::-1]), np.arange(coords.shape[0]))


@pytest.mark.parametrize("name", ALL)
def test_geometry_is_valid_and_not_uniform(name, oracles):
    coords, cells, tags = IM.mesh(name)
    vol = IM.cell_volumes(coords, cells)
    assert vol.min() > 0 and vol.min() >= 1e-3 * vol.mean()
    assert abs(vol.sum() - 1.0) <= 1e-12                        # the cells tile the unit square / cube: no hole, no overlap
    o = oracles(name)
    assert o.fmeas.min() > 0 and len(o.fmeas) >= 20
    assert vol.max() >= 3.0 * vol.min() and o.fmeas.max() >= 3.0 * o.fmeas.min()


@pytest.mark.parametrize("name", ALL)
def test_valence_is_on_the_intended_side_of_the_thresholds(name, oracles):
    o = oracles(name)
    g = IM.graph_stats(o)
    e = IM.EXPECT[name]
    pairs, ncell = int(g["pairs"].max()), int(g["cells_per_node"].max())
    assert pairs > e["asm_group"]                               # a second trip of every lane-group loop, at the default width
    if name in HUBS and name != "hub2d_12_48m":
        assert pairs > 32                                       # ... and at the widest instantiation
    assert (ncell > 255) == (name in ("hub2d_12_300", "hub3d_5_140"))
    assert (pairs > 255) == (name == "hub2d_12_300")
    IM.check_launch(IM.predicted_launch(o), name)
    # the self pair of some node sits past the first trip (k_assemble_nodes_tr emits it from lane selfq & (G - 1)); the plain 2D meshes
    # have too few nodes of 9 pairs for that, the transposed kernel gets it from the two small 2D hubs
    lay = o.lay
    import scipy.sparse as sp
    cn = o.cnode
    nv1 = cn.shape[1]
    E = sp.coo_matrix((np.ones(cn.size * nv1), (np.repeat(cn, nv1, axis=1).ravel(), np.tile(cn, (1, nv1)).ravel())),
                      shape=(lay.n_nodes, lay.n_nodes)).tocsr()
    E.sort_indices()
    selfq = np.array([np.searchsorted(E.indices[E.indptr[n]:E.indptr[n + 1]], n) for n in range(lay.n_nodes)])
    if not name.startswith("delaunay2d"):
        assert selfq.max() >= e["asm_group"]


def test_the_membrane_hub_has_a_node_on_both_sides(oracles):
    o = oracles("hub2d_12_48m")
    coords = IM.mesh("hub2d_12_48m")[0]
    v = IM.hub_vertex(coords, IM.MEMBRANE_HUB)
    ni, ne = int(o.lay.node_i[v]), int(o.lay.node_e[v])
    assert ni >= 0 and ne >= 0
    pairs = IM.graph_stats(o)["pairs"]
    assert pairs[ni] > 8 and pairs[ne] > 8
    # the membrane passes through it: two membrane edges, the spokes of the ring (shorter than the grid's edges)
    on = np.any(o.fv == v, axis=1)
    assert on.sum() == 2 and o.fmeas[on].max() < np.median(o.fmeas)


@pytest.mark.parametrize("name", ["hub2d_12_40", "hub2d_12_300", "hub3d_5_60", "hub3d_5_140"])
def test_interior_hubs_are_one_sided(name, oracles):
    o = oracles(name)
    v = IM.hub_vertex(IM.mesh(name)[0], HUBS[name])
    assert o.lay.node_i[v] >= 0 and o.lay.node_e[v] < 0
    assert IM.graph_stats(o)["pairs"][o.lay.node_i[v]] == IM.graph_stats(o)["pairs"].max()


@pytest.mark.parametrize("name", ALL)
def test_oracle_assembles_and_steps(name, oracles):
    o = oracles(name)
    A = o.assemble_A()
    P = o.assemble_P()
    b = o.assemble_b()
    assert np.isfinite(A.data).all() and np.isfinite(P.data).all() and np.isfinite(b).all()
    assert np.linalg.norm(A @ o.nullspace()) <= 1e-10 * np.abs(A.data).max()
    o2 = IM.oracle(name)
    o2.run(1, solver="lu_gauge")
    ni, ne = o2.potential_norms()
    assert np.isfinite([ni, ne]).all() and ni > 0


def test_two_tag_split_has_two_cells_with_membrane():
    from cgx_hip import mesh as meshmod
    coords, cells, tags = IM.mesh("delaunay3d_5")
    t2 = IM.two_tag(coords, cells, tags)
    assert set(np.unique(t2)) == {1, 2, 3} and np.array_equal(t2 == 1, tags == 2)
    gamma, ftags, fverts = meshmod.gamma_integration_entities(cells, t2, (2, 3), (1,), "intra")
    assert set(np.unique(ftags)) == {2, 3} and min((ftags == 2).sum(), (ftags == 3).sum()) >= 20


def test_the_eight_meshes_are_meant_to_reach_every_assembly_path():
    paths = {(IM.EXPECT[n]["asm_variant"], IM.EXPECT[n]["fused"]) for n in IM.EIGHT}
    assert paths == {(2, True), (1, True), (1, False), (0, False)}
    trips = [IM.EXPECT[n]["trips"] for n in IM.EIGHT]
    assert min(trips) >= 2 and sum(t >= 4 for t in trips) >= 4
