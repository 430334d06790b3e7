"""The inputs of tests/test_gpu_derived_fields.py, pinned without a GPU: the NumPy reference of the derived fields
(tests/derived_field_ref.py) meets closed forms, its inverted index and plan rules are the ones of csrc/knp_fields.inc as the header
states them, every derivative case has a rounding floor <= ``functionals_irregular.BOUND``, and ``fields.FieldsWriter`` writes a
complete fields.xdmf / fields.h5 pair from host arrays."""
import math
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import derived_field_ref as DR
import functional_ref
import functionals_irregular as FI
import irregular_meshes as IM
from cgx_hip.fields import PROJECT_INFO, FieldsWriter


@pytest.fixture(scope="module")
def probs(tmp_path_factory):
    cache = {}
    tmp = tmp_path_factory.mktemp("derived_fields_host")

    def get(name):
        if name not in cache:
            cache[name] = FI.Prob(tmp, name)
        return cache[name]
    return get


def _lib_declares_the_new_entries():
    from cgx_hip import _lib
    for n in ("knp_functional_eval_items", "knp_membrane_functional_eval_items", "knp_project_create", "knp_project_apply",
              "knp_project_get_info", "knp_project_destroy"):
        assert n in _lib.SIGNATURES, n


# ---------------------------------------------------------------------------------------------- per-item means against closed forms
@pytest.mark.parametrize("name", ["delaunay2d_12_cw", "hub2d_12_300", "hub3d_5_60"])
def test_affine_function_has_its_constant_gradient_in_every_cell(probs, name):
    from cgx_hip import fem
    _lib_declares_the_new_entries()
    P = probs(name)
    g = list(fem.grad(P.lin))
    cells, side, mean, scale = DR.cell_field(P.p, g, g, degree=1)
    assert mean.shape == (len(cells), P.dim) and set(side.tolist()) == {0, 1}
    # lin = slope . x + 1e3 in fp64 nodal values: each value is off by at most 2^-44, a difference by 2^-43, against edges of length h
    lm = P.p.local_mesh
    G = functional_ref.simplex_gradients(lm.coords[np.asarray(lm.cells)[cells]])
    bound = 2.0 ** -43 * np.abs(G[:, 1:, :]).sum(axis=1) + 1e-12 * np.abs(P.slope)[None, :]
    assert np.all(np.abs(mean - P.slope[None, :]) <= bound), np.abs(mean - P.slope[None, :]).max()


@pytest.mark.parametrize("name", ["delaunay2d_12_cw", "hub3d_5_60"])
def test_the_coordinate_has_the_centroid_as_its_mean(probs, name):
    from cgx_hip import fem
    P = probs(name)
    x = list(fem.SpatialCoordinate(P.p.mesh))
    for degree in (1, 3):
        cells, _, mean, scale = DR.cell_field(P.p, x, x, degree=degree)
        lm = P.p.local_mesh
        cen = lm.coords[np.asarray(lm.cells)[cells]].mean(axis=1)
        assert np.all(np.abs(mean - cen) <= 1e-14 * scale)
    facets, fmean, fscale = DR.facet_field(P.p, x, degree=2)
    fcen = P.p.local_mesh.coords[np.asarray(P.p._fv)[facets]].mean(axis=1)
    assert len(facets) == len(P.p._fv) and np.all(np.abs(fmean - fcen) <= 1e-14 * fscale)


@pytest.mark.parametrize("name", DR.CELL_MESHES)
def test_measure_times_mean_summed_per_tag_is_the_functional_reference(probs, name):
    P = probs(name)
    p = P.p
    lm = p.local_mesh
    for case in DR.CELL_CASES:
        fi, fe, degree = DR.cell_forms(P, case)
        cells, side, mean, _ = DR.cell_field(p, fi, fe, degree=degree)
        tags, tside, want, scale = functional_ref.reference(p, fi, fe, degree=degree)
        vol = functional_ref.cell_volumes(lm.coords[np.asarray(lm.cells)[cells]])
        ctag = np.asarray(lm.cell_tags)[cells]
        got = np.array([[math.fsum(vol[ctag == t] * mean[ctag == t, j]) for j in range(mean.shape[1])] for t in tags])
        assert np.all(np.abs(got - want) <= 1e-13 * scale), (name, case)
    assert list(tags) == ([2, 3, 1] if name == FI.TWO_TAG else [1, 2])


# ---------------------------------------------------------------------------------------------- the projection
def _star(lengths, nv, n_vertices, rng):
    """items of ``nv`` vertices: list k has ``lengths[k]`` items around vertex k, whose other vertices are fresh ones past the hubs"""
    iv, nxt = [], len(lengths)
    for k, ln in enumerate(lengths):
        for _ in range(ln):
            iv.append([k] + list(range(nxt, nxt + nv - 1)))
            nxt += nv - 1
    iv = np.array(iv, dtype=np.int32).reshape(-1, nv)
    assert nxt <= n_vertices
    return iv[rng.permutation(len(iv))] if len(iv) else iv


def test_inverted_index_lists_every_item_once_per_vertex_ascending():
    rng = np.random.default_rng(5)
    coords, cells, _ = IM.mesh("hub2d_12_300")
    ptr, items = DR.inverted_index(len(coords), cells)
    assert ptr[-1] == cells.size
    for v in rng.integers(0, len(coords), 40).tolist() + [IM.hub_vertex(coords, (0.5, 0.5))]:
        want = np.nonzero((cells == v).any(axis=1))[0]
        assert np.array_equal(items[ptr[v]:ptr[v + 1]], want)
    info = DR.plan_info(ptr)
    assert info["longest"] >= 300 and info["n_split"] == 0 and info["lanes"] == 8 and info["n_units"] == len(coords)


def test_plan_rules_lanes_and_split():
    for L in DR.LANES:
        ln = np.array([0, 1, L - 1, L, L + 1] if L > 2 else [0, 1, 1, 2, 3])
        assert DR.plan_info(np.concatenate([[0], np.cumsum(ln)]))["lanes"] == L, L
    ptr = np.concatenate([[0], np.cumsum([DR.SPLIT, DR.SPLIT + 1, 3 * DR.SPLIT + 7, 0])])
    info = DR.plan_info(ptr)
    assert tuple(info) == PROJECT_INFO      # the slots of knp_project_get_info, in its order
    assert info == {"lanes": 32, "longest": 3 * DR.SPLIT + 7, "n_split": 2, "n_units": 1 + 2 + 4 + 1, "split": DR.SPLIT}


def test_projecting_a_constant_gives_the_constant_and_empty_lists_the_fill():
    rng = np.random.default_rng(7)
    iv = _star([0, 1, 5, 40], 3, 200, rng)
    meas = 10.0 ** rng.uniform(-3, 3, len(iv))
    out, scale, ptr = DR.project(200, iv, meas, np.full((len(iv), 2), -3.5), fill=-7.0)
    used = np.diff(ptr) > 0
    assert np.all(np.abs(out[:, used] + 3.5) <= 1e-15 * 3.5) and np.all(out[:, ~used] == -7.0) and not used[0]
    assert np.allclose(scale[:, used], 3.5)
    out, _, _ = DR.project(200, iv, meas, np.zeros((len(iv), 1)))
    assert np.all(np.isnan(out[:, ~used])) and np.all(out[:, used] == 0.0)


@pytest.mark.parametrize("name", ["hub2d_12_300", "hub3d_5_140"])
def test_projection_identity_on_meshes(name):
    """sum_v u(v) (sum_{T in list(v)} |T|) / (d + 1) = sum_T |T| mean_T"""
    rng = np.random.default_rng(9)
    coords, cells, _ = IM.mesh(name)
    d = coords.shape[1]
    vol = IM.cell_volumes(coords, cells)
    val = rng.uniform(-1.0, 2.0, (len(cells), 1))
    out, _, ptr = DR.project(len(coords), cells, vol, val)
    lump = np.zeros(len(coords))
    np.add.at(lump, cells.ravel(), np.repeat(vol, d + 1))
    lhs = math.fsum(np.nan_to_num(out[0]) * lump / (d + 1))
    assert abs(lhs - math.fsum(vol * val[:, 0])) <= 1e-13 * np.abs(vol * val[:, 0]).sum()


# ---------------------------------------------------------------------------------------------- the tolerance floors
def test_tolerance_floors(probs):
    for name in DR.CELL_MESHES:
        for case in DR.CELL_CASES:
            f = DR.cell_floor(probs(name), case)
            assert f <= (FI.BOUND if case in DR.DERIVATIVE_CASES else 1e-15), (name, case, f)
    for name in DR.FACET_MESHES:
        for case in DR.FACET_CASES:
            f = DR.facet_floor(probs(name), case)
            assert f <= (FI.BOUND if case in DR.DERIVATIVE_CASES else 1e-15), (name, case, f)
    print("\n".join(DR.floor_table()))


# ---------------------------------------------------------------------------------------------- fields.xdmf / fields.h5
@pytest.mark.parametrize("name", ["delaunay2d_12_cw", "delaunay3d_5"])
def test_fields_writer_on_host_arrays(tmp_path, name):
    from cgx_hip import hdf5_min
    from cgx_hip.xdmf import XdmfFile
    rng = np.random.default_rng(11)
    coords, cells, _ = IM.mesh(name)
    d = coords.shape[1]
    fv = np.ascontiguousarray(cells[:17, :d], dtype=np.int64)
    xname, hname = str(tmp_path / "fields.xdmf"), str(tmp_path / "fields.h5")
    W = FieldsWriter(xname, hname, coords, cells, [{"name": "J", "kind": "cell", "n_out": d}, {"name": "rho", "kind": "node", "n_out": 1},
                                                    {"name": "I", "kind": "facet", "n_out": 1, "vertices": fv},
                                                    {"name": "two", "kind": "facet", "n_out": 5 - d, "vertices": fv}])
    recs = []
    for k in range(3):
        data = {"J": rng.normal(size=(len(cells), d)), "I": rng.normal(size=(17, 1))}
        if k != 1:      # another interval
            data["rho"] = (rng.normal(size=(1, len(coords))), rng.normal(size=(1, len(coords))))
            data["two"] = rng.normal(size=(17, 5 - d))
        W.write(0.1 * k, data)
        recs.append(data)
        root = ET.parse(xname).getroot()      # a complete document after every record
        steps = [g for g in root.iter("Grid") if g.get("CollectionType") == "Spatial"]
        assert len(steps) == k + 1 and [g.get("Name") for g in steps[-1].findall("Grid")] == ["mesh", "membrane"]
    W.close()
    h5 = hdf5_min.Hdf5File(hname)
    assert np.array_equal(h5.read("/Mesh/membrane/topology"), fv) and np.array_equal(h5.read("/Mesh/mesh/topology"), cells)
    J2 = h5.read("/Field/J/2")
    assert J2.shape == (len(cells), 3) and np.array_equal(J2[:, :d], recs[2]["J"]) and (d == 3 or np.all(J2[:, 2] == 0.0))
    assert np.array_equal(h5.read("/Field/rho_i/1")[:, 0], recs[2]["rho"][0][0]) and np.array_equal(h5.read("/Field/rho_e/0")[:, 0], recs[0]["rho"][1][0])
    assert np.array_equal(h5.read("/Field/I/1"), recs[1]["I"])
    if d == 2:      # 3 outputs in 2D: a vector needs dim outputs, so three scalars
        assert np.array_equal(h5.read("/Field/two_2/1")[:, 0], recs[2]["two"][:, 2])
    else:           # 2 outputs in 3D: two scalars
        assert np.array_equal(h5.read("/Field/two_1/0")[:, 0], recs[0]["two"][:, 1])
    txt = open(xname).read()
    assert txt.count('AttributeType="Vector" Center="Cell"') == 3 and txt.count('Center="Node"') == 4
    assert ('TopologyType="Polyline" NumberOfElements="17" NodesPerElement="2"' in txt) == (d == 2)
    assert ('TopologyType="Triangle" NumberOfElements="17" NodesPerElement="3"' in txt) == (d == 3)
    topo, pts, _ = XdmfFile(xname).grid("membrane")      # the project's own reader takes the facet grid
    assert np.array_equal(topo, fv) and np.array_equal(pts, coords)
    assert not os.path.exists(str(tmp_path / "solution.h5"))
