"""Level-set surfaces on the device (csrc/knp_surface.inc, ``LevelSetSurface`` / ``ClipSurface`` / ``IsoSurface`` of
cgx_hip/surfaces.py, ``ActivationMap.isochrones``, ``add_surface`` and the output key ``clip_surfaces``) against the NumPy
restatement of tests/surface_ref.py, whose inputs and outputs tests/test_surface_host.py shows to be sound.

Tolerances, all derived: elements, their item / tag / kind, (a, b, side) and the vertex numbering equal the reference exactly -- every
input keeps |t_v| exactly 0 or at least 1e-9 max|s| (asserted), so no decision depends on rounding; |w - w_ref| <= 4 eps (two
correctly rounded operations, w < 1); positions and fields <= 8 eps max(|F_a|, |F_b|) per value (three operations, either
contraction choice).  The measured maxima are printed (-s)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import irregular_meshes as IM
import surface_ref as SR
from parity_utils import ci_config, make_problem, snapshot_state

pytestmark = pytest.mark.gpu
E_ARG = -1
EPS = SR.EPS
NAN = float("nan")


# ---- comparison -------------------------------------------------------------------------------------------------------------------
def _host(t):
    return t.cpu().numpy()


def _compare(S, R, coords, what):
    """the built surface ``S`` against the reference dict ``R``: structure exactly, w and positions to the derived bounds"""
    assert R["margin"] >= 1e-9, (what, R["margin"])
    assert S.n_elements == len(R["elements"]) and S.n_vertices == len(R["a"]), (what, S.n_elements, len(R["elements"]), S.n_vertices, len(R["a"]))
    assert S.elements.dtype == torch.int32 and S.elements.shape == (S.n_elements, S.npe)
    assert np.array_equal(_host(S.elements), R["elements"]), what
    assert np.array_equal(_host(S.element_item), R["element_item"]) and np.array_equal(_host(S.element_tag), R["element_tag"]), what
    assert np.array_equal(_host(S.element_kind), R["element_kind"]), what
    v = S.vertices
    assert np.array_equal(_host(v.a), R["a"]) and np.array_equal(_host(v.b), R["b"]) and np.array_equal(_host(v.side), R["side"]), what
    assert [int(k) for k in _host(S.keys)] == R["key"], what
    if S.n_vertices == 0:
        return
    ew = float(np.abs(_host(v.w).astype(SR.LD) - R["w"]).max())
    X = np.asarray(coords, dtype=np.float64)
    scale = np.maximum(np.abs(X[R["a"]]), np.abs(X[R["b"]]))
    bound = 8 * EPS * scale
    err = np.abs(_host(S.xyz).astype(SR.LD) - R["xyz"]).astype(np.float64)
    rel = float((err[scale > 0] / (EPS * scale[scale > 0])).max()) if (scale > 0).any() else 0.0
    print(f"{what}: {S.n_elements} elements, {S.n_vertices} vertices, max |w - w_ref| = {ew / EPS:.2f} eps, max position error = {rel:.2f} eps max(|x_a|, |x_b|)")
    assert ew <= 4 * EPS, (what, ew)
    assert np.all(err <= bound), (what, rel)
    assert np.all(_host(v.w)[R["a"] == R["b"]] == 0.0) and np.array_equal(_host(S.xyz)[R["a"] == R["b"]], X[R["a"][R["a"] == R["b"]]])


def _dev(a, S=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda" if S is None else S.device)


def _check_gather(S, R, seed, what, n_fields=3):
    rng = np.random.default_rng(seed)
    nv = S.n_mesh_vertices
    Fi, Fe = rng.uniform(-150.0, 150.0, (n_fields, nv)), rng.uniform(-150.0, 150.0, (n_fields, nv))
    got = _host(S([_dev(f, S) for f in Fi], [_dev(f, S) for f in Fe]))
    assert got.shape == (n_fields, S.n_vertices)
    worst = 0.0
    for f in range(n_fields):
        want, scale = SR.gather(R, Fi[f], Fe[f])
        err = np.abs(got[f].astype(SR.LD) - want).astype(np.float64)
        assert np.all(err <= 8 * EPS * scale), (what, f, float((err / (EPS * scale)).max()))
        worst = max(worst, float((err / (EPS * scale)).max())) if len(err) else worst
        orig = R["a"] == R["b"]
        assert np.array_equal(got[f][orig], np.where(R["side"] == 0, Fi[f][R["a"]], Fe[f][R["a"]])[orig]), what      # F[a] exactly
    print(f"{what}: gather of {n_fields} x {S.n_vertices} values, max error = {worst:.2f} eps max(|F_a|, |F_b|)")


def _surface(coords, items, side, ref, bf=None, bi=None):
    from cgx_hip.surfaces import LevelSetSurface
    return LevelSetSurface(np.asarray(coords), items, side, ref, bf, bi)


# ---- 1. the tables, through the context-free entry points on hand-made arrays --------------------------------------------------------
TET = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
TRI = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])


def _patterns(X, flips, zero_every=3, nan_items=2):
    """one simplex per inside / outside pattern and per orientation, each on vertices of its own: (coords, items, s); in every
    ``zero_every``-th simplex the inside vertices lie exactly on the level; ``nan_items`` more simplices have a NaN"""
    npi = X.shape[0]
    coords, items, s = [], [], []
    k = 0
    for flip in flips:
        for mask in range(2 ** npi):
            base = len(coords)
            coords += [x + 3.0 * k * np.eye(X.shape[1])[0] for x in X]
            order = list(range(npi))
            if flip:
                order[-2], order[-1] = order[-1], order[-2]
            items.append([base + j for j in order])
            for j in range(npi):
                inside = bool(mask >> j & 1)
                s.append((0.0 if k % zero_every == 0 else 0.5 + 0.25 * j) if inside else -(0.75 + 0.125 * j))
            k += 1
    for n in range(nan_items):
        base = len(coords)
        coords += [x + 3.0 * k * np.eye(X.shape[1])[0] for x in X]
        items.append([base + j for j in range(npi)])
        s += [1.0 if j != n else NAN for j in range(npi - 1)] + [-1.0]
        k += 1
    return np.array(coords), np.array(items, dtype=np.int64), np.array(s)


def test_table_of_the_tetrahedron_in_all_patterns_and_both_orientations():
    coords, items, s = _patterns(TET, (False, True))
    side, ref = np.arange(len(items)) % 2, 100 + np.arange(len(items))
    S = _surface(coords, items, side, ref).build(_dev(s), 0.0)
    R = SR.cut(coords, items, side, ref, s, 0.0)
    _compare(S, R, coords, "tetrahedron table")
    counts = np.bincount(R["element_item"], minlength=len(items))
    n_in = (s.reshape(-1, 4) >= 0).sum(axis=1)[:32]
    assert np.array_equal(counts[:32], np.array([0, 1, 2, 1, 0])[n_in]) and np.all(counts[32:] == 0)      # NaN items emit nothing
    # every cut face with an area has its normal from the inside vertices to the outside ones
    xyz, el = _host(S.xyz), _host(S.elements)
    for e, it in zip(el, R["element_item"]):
        X, sv = coords[items[it]], s[items[it]]
        n = np.cross(xyz[e[1]] - xyz[e[0]], xyz[e[2]] - xyz[e[0]])
        if np.linalg.norm(n) > 0:
            assert n @ (X[sv < 0].mean(axis=0) - X[sv >= 0].mean(axis=0)) > 0
    _check_gather(S, R, 5, "tetrahedron table")


@pytest.mark.parametrize("dim", [2, 3])
def test_table_of_the_triangle_in_all_patterns(dim):
    X = TRI if dim == 2 else np.column_stack([TRI, [0.25, 0.5, 0.75]])
    coords, items, s = _patterns(X, (False, True), nan_items=1)
    side, ref = np.zeros(len(items), dtype=np.int64), 7 * np.arange(len(items))
    S = _surface(coords, items, side, ref).build(_dev(s), 0.0)
    R = SR.cut(coords, items, side, ref, s, 0.0)
    _compare(S, R, coords, f"triangle table, {dim}D")
    assert S.npe == 2 and np.array_equal(np.bincount(R["element_item"], minlength=len(items))[:16],
                                         np.array([0, 1, 1, 0])[(s.reshape(-1, 3) >= 0).sum(axis=1)[:16]])
    if dim == 2:      # the kept part lies to the left of every segment with a length
        xyz, el = _host(S.xyz), _host(S.elements)
        for e, it in zip(el, R["element_item"]):
            P, sv = coords[items[it]], s[items[it]]
            d, to_in = xyz[e[1]] - xyz[e[0]], P[sv >= 0].mean(axis=0) - P[sv < 0].mean(axis=0)
            if np.linalg.norm(d) > 0:
                assert d[0] * to_in[1] - d[1] * to_in[0] > 0


def test_table_of_the_boundary_facet_in_all_patterns_and_both_orientations():
    # one all-outside tetrahedron per facet as its item (it cuts nothing: its own vertices sit below the level), the facet on
    # vertices of its own
    coords, facets, s = _patterns(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), (False, True), nan_items=1)
    nf, base = len(facets), len(coords)
    coords = np.vstack([coords, np.tile(TET, (nf, 1)) + np.repeat(np.arange(nf), 4)[:, None] * np.array([0.0, 5.0, 0.0])])
    items = base + np.arange(4 * nf).reshape(nf, 4)
    s = np.concatenate([s, np.full(4 * nf, -2.0)])
    side, ref = np.arange(nf) % 2, 50 + np.arange(nf)
    bi = np.arange(nf)[::-1].copy()
    S = _surface(coords, items, side, ref, facets, bi).build(_dev(s), 0.0)
    R = SR.cut(coords, items, side, ref, s, 0.0, facets, bi)
    _compare(S, R, coords, "boundary facet table")
    assert np.all(R["element_kind"] == 1)
    n_in = (s[:3 * 16].reshape(-1, 3) >= 0).sum(axis=1)
    per_facet = np.bincount(nf - 1 - R["element_item"], minlength=nf)          # facet f belongs to item nf - 1 - f
    assert np.array_equal(per_facet[:16], np.array([0, 1, 2, 1])[n_in]) and per_facet[16] == 0
    # clipping keeps the cyclic order: every clipped piece with an area has the normal of its facet
    xyz, el = _host(S.xyz), _host(S.elements)
    for e, it in zip(el, R["element_item"]):
        F = coords[facets[nf - 1 - it]]
        n, nF = np.cross(xyz[e[1]] - xyz[e[0]], xyz[e[2]] - xyz[e[0]]), np.cross(F[1] - F[0], F[2] - F[0])
        if np.linalg.norm(n) > 0:
            assert n @ nF > 0


def test_table_of_the_boundary_edge_in_2d():
    coords, edges, s = _patterns(np.array([[0.0, 0.0], [1.0, 0.0]]), (False, True), zero_every=3, nan_items=1)
    nf, base = len(edges), len(coords)
    coords = np.vstack([coords, np.tile(TRI, (nf, 1)) + np.repeat(np.arange(nf), 3)[:, None] * np.array([0.0, 5.0])])
    items = base + np.arange(3 * nf).reshape(nf, 3)
    s = np.concatenate([s, np.full(3 * nf, -2.0)])
    side, ref, bi = np.zeros(nf, dtype=np.int64), np.arange(nf), np.arange(nf)
    S = _surface(coords, items, side, ref, edges, bi).build(_dev(s), 0.0)
    R = SR.cut(coords, items, side, ref, s, 0.0, edges, bi)
    _compare(S, R, coords, "boundary edge table")
    assert np.array_equal(np.bincount(R["element_item"], minlength=nf)[:8], [0, 1, 1, 1, 0, 1, 1, 1])


# ---- 2. meshes ----------------------------------------------------------------------------------------------------------------------
MESH_CASES = {      # case -> (mesh, tags kept, plane)
    "cube4_aligned": ("cube4", (1,), "aligned"), "cube4_oblique": ("cube4", (1,), "oblique"),
    "delaunay3d": ("delaunay3d_5", (1,), "oblique"), "hub3d": ("hub3d_5_60", (1,), "oblique"),
    "reoriented3d": ("delaunay3d_5_reoriented", (1,), "oblique"),
    "delaunay2d": ("delaunay2d_12", (1,), "oblique"), "hub2d": ("hub2d_12_40", (1,), "oblique"),
    "two_tag_seam": ("two_tag", (1, 2, 3), "oblique"), "two_tag_one": ("two_tag", (3,), "oblique"),
    "miss": ("cube4", (1,), "miss"), "all_inside": ("cube4", (1,), "all_inside"),
}


def _mesh_config(mesh, tmp):
    if mesh == "cube4":
        return ci_config(N=4, steps=1, kind="cube")
    if mesh == "two_tag":
        return IM.two_tag_config(tmp)
    if mesh == "delaunay3d_5_reoriented":
        coords, cells, tags = IM.reoriented("delaunay3d_5", seed=31)
        path = IM.write_npz(tmp, mesh, coords, cells, tags)
        cfg = IM.config(tmp, "delaunay3d_5")
        cfg.update({"cell_tag_file": path, "facet_tag_file": path})
        return cfg
    return IM.config(tmp, mesh)


@pytest.fixture(scope="module")
def problems(tmp_path_factory):
    """one problem per mesh, shared by the tests of this module"""
    cache, tmp = {}, tmp_path_factory.mktemp("surface_meshes")

    def get(mesh):
        if mesh not in cache:
            cache[mesh] = make_problem(_mesh_config(mesh, tmp), "ci")
        return cache[mesh]
    return get


def _plane(p, which):
    f, dim = float(p.mesh_conversion_factor), p.local_mesh.coords.shape[1]
    origin, normal = {"aligned": (np.array([0.5, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])), "oblique": SR.OBLIQUE,
                      "miss": (np.array([2.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0])),
                      "all_inside": (np.array([-1.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0]))}[which]
    return origin[:dim] * f, normal[:dim]


_REF = {}


def _reference(case, boundary, p):
    """the reference surface of a mesh case, computed once per process"""
    if (case, boundary) not in _REF:
        mesh, keep, plane = MESH_CASES[case]
        lm = p.local_mesh
        origin, normal = _plane(p, plane)
        arrays = SR.kept_arrays(lm.coords, np.asarray(lm.cells), np.asarray(lm.cell_tags), keep, p.intra_tags, boundary)
        s = SR.plane_s(lm.coords, origin, normal)
        _REF[(case, boundary)] = (SR.cut(lm.coords, *arrays[:3], s, 0.0, arrays[3], arrays[4]), s, arrays[5])
    return _REF[(case, boundary)]


@pytest.mark.parametrize("boundary", [True, False])
@pytest.mark.parametrize("case", list(MESH_CASES))
def test_clip_surfaces_match_the_reference(case, boundary, problems):
    from cgx_hip.surfaces import ClipSurface
    mesh, keep, plane = MESH_CASES[case]
    p = problems(mesh)
    R, s, item_cell = _reference(case, boundary, p)
    S = ClipSurface(p, keep, None, *_plane(p, plane), boundary=boundary)
    assert np.array_equal(_host(S._s), s), case                    # the plane's level function, bit for bit
    assert np.array_equal(S.item_cell, item_cell)
    _compare(S, R, p.local_mesh.coords, f"{case}, boundary {boundary}")
    assert np.array_equal(_host(S.element_cell), item_cell[R["element_item"]])
    m = SR.measures(R["xyz"], R["elements"])
    # a position is off by at most 8 eps max|x|; moving the vertices of an element with longest edge L by d changes its measure by at
    # most 3 d L / 2 (a segment: 2 d), and the cross product of fp64 edges adds a few eps L^2: slivers keep an absolute bound, no relative one
    X = np.asarray(R["xyz"], dtype=np.float64)[R["elements"]]
    L = np.linalg.norm(X - np.roll(X, 1, axis=1), axis=2).max(axis=1) if len(X) else np.zeros(0)
    bound = 24 * EPS * float(np.abs(p.local_mesh.coords).max()) * (L if S.npe == 3 else 1.0) + 8 * EPS * L * (L if S.npe == 3 else 1.0)
    assert np.all(np.abs(_host(S.measure()) - m) <= bound) and abs(S.area() - m.sum()) <= bound.sum() + 4 * EPS * m.sum()
    if case == "miss":
        assert S.n_elements == 0 and S.n_vertices == 0 and S([p.wh[0][0]], [p.wh[1][0]]).shape == (1, 0)      # the gather is a no-op
    elif case == "cube4_aligned" and boundary:
        f = float(p.mesh_conversion_factor)
        assert S.n_elements == 80 and int((m == 0.0).sum()) == 48 and abs(m.sum() - f * f) <= 1e-13 * f * f
    elif case == "two_tag_seam" and boundary:
        assert set(np.unique(R["side"])) == {0, 1} and not SR.topology(R["elements"])[0]
        assert SR.topology(_host(S.elements), merge=np.column_stack([_host(S.vertices.a), _host(S.vertices.b)])) == (True, 2)
    elif case == "all_inside":
        # everything inside: the surface of the intracellular cells is their membrane facets plus their exterior facets (none here)
        F = p.facet_field(p.phi_m_prev)
        if boundary:
            assert S.n_elements == len(F.area) and np.all(R["element_kind"] == 1)
            assert abs(S.area() - F.area.sum()) <= 1e-13 * F.area.sum()
        else:
            assert S.n_elements == 0
    if S.n_vertices:
        _check_gather(S, R, 11, case)


def test_membrane_vertices_take_the_value_of_their_elements_side_and_affine_fields_are_reproduced(problems):
    from cgx_hip.surfaces import ClipSurface
    p = problems("two_tag")
    lm = p.local_mesh
    X = np.asarray(lm.coords)
    S = ClipSurface(p, (1, 2, 3), None, *_plane(p, "oblique"))
    a, b, side = _host(S.vertices.a).astype(np.int64), _host(S.vertices.b).astype(np.int64), _host(S.vertices.side)
    got = _host(S([_dev(np.full(len(X), 1.0), S)], [_dev(np.full(len(X), -1.0), S)]))[0]
    assert np.array_equal(got, np.where(side == 0, 1.0, -1.0))
    on_membrane = np.zeros(len(X), dtype=bool)
    on_membrane[np.unique(p._fv)] = True
    nv = len(X)
    both = np.intersect1d((a * nv + b)[side == 0], (a * nv + b)[side == 1])
    assert len(both) > 0 and np.all(on_membrane[both // nv]) and np.all(on_membrane[both % nv])      # the same point of a membrane edge, once per side
    L = X.max(axis=0) - X.min(axis=0)
    c_i, c_e = np.array([3.0, -2.0, 1.5]) / L, np.array([-1.0, 4.0, 2.5]) / L
    f_i, f_e = X @ c_i + 0.7, X @ c_e - 1.3
    got = _host(S([_dev(f_i, S)], [_dev(f_e, S)]))[0]
    xyz = _host(S.xyz)
    want = np.where(side == 0, xyz @ c_i + 0.7, xyz @ c_e - 1.3)
    scale = max(np.abs(f_i).max(), np.abs(f_e).max())
    err = float(np.abs(got - want).max())
    print(f"affine fields on the two-sided clip: max error {err / (EPS * scale):.2f} eps max|f|")
    assert err <= 32 * EPS * scale      # f(xyz) is itself a sum of dim + 1 products of rounded positions: 8 eps each side of the comparison, dim + 1 terms


def test_iso_surface_of_a_function_and_its_update(problems):
    from cgx_hip import fem
    from cgx_hip.surfaces import IsoSurface
    p = problems("cube4")
    lm = p.local_mesh
    f = float(p.mesh_conversion_factor)
    s = SR.sphere_s(np.asarray(lm.coords) / f)
    fn = fem.Function(p.V if getattr(p, "V", None) is not None else fem.FunctionSpace(p.mesh), "level")
    fn.x.array.copy_(torch.as_tensor(s, device=fn.x.array.device))
    tags = tuple(int(t) for t in p.extra_tag)
    S = IsoSurface(p, None, fn, iso=0.0, tags=tags)
    arrays = SR.kept_arrays(lm.coords, np.asarray(lm.cells), np.asarray(lm.cell_tags), tags, p.intra_tags, False)
    _compare(S, SR.cut(lm.coords, *arrays[:3], s, 0.0), lm.coords, "iso-surface in the extracellular cells")
    assert np.all(_host(S.vertices.side) == 1) and np.all(_host(S.element_kind) == 0)
    fn.x.array.mul_(2.0)
    S.update(iso=0.1)
    _compare(S, SR.cut(lm.coords, *arrays[:3], 2.0 * s, 0.1), lm.coords, "iso-surface after update")
    with pytest.raises(ValueError):
        IsoSurface(p, fn, fn, iso=0.0, tags=tuple(p.intra_tags) + tags)


# ---- 3. launch width ------------------------------------------------------------------------------------------------------------------
def test_item_lists_beyond_the_grid_wrap_the_stride():
    """1024 blocks of 256 lanes: the cells of create_unit_cube(36) (279936) are the smallest generated mesh that wraps"""
    from cgx_hip import _lib, mesh as meshmod
    from cgx_hip.surfaces import launch_info
    coords, cells = meshmod.create_unit_cube(36)
    assert len(cells) > 1024 * 256 >= 6 * 35 ** 3
    tags = meshmod.mark_subdomains_box(coords, cells)
    s = SR.plane_s(coords, *SR.OBLIQUE)
    S = _surface(coords, cells, np.zeros(len(cells), dtype=np.uint8), tags)
    sd = _dev(s, S)
    assert _lib.load().knp_surface_count(4, len(cells), len(coords), S._items.data_ptr(), 0, None, None, sd.data_ptr(), 0.0,
                                         S._counts.data_ptr(), None) == 0
    info = launch_info()
    assert info == {"kernel": 2, "blocks": 1024, "threads": 256, "n": len(cells), "trips": 2, "grid_y": 1}
    torch.cuda.synchronize()
    S.build(sd, 0.0)
    R = SR.cut(coords, cells, np.zeros(len(cells), dtype=np.int64), tags, s, 0.0)
    _compare(S, R, coords, "cube36 slice")
    assert S.n_elements > 256 and launch_info()["kernel"] == 5 and launch_info()["blocks"] == min(-(-S.n_elements * 3 // 256), 1024)


def test_vertex_lists_just_above_one_block():
    from cgx_hip import mesh as meshmod
    from cgx_hip.surfaces import launch_info
    for N in range(4, 12):
        coords, cells = meshmod.create_unit_cube(N)
        s = SR.plane_s(coords, *SR.OBLIQUE)
        R = SR.cut(coords, cells, np.zeros(len(cells), dtype=np.int64), np.zeros(len(cells), dtype=np.int64), s, 0.0)
        if len(R["a"]) > 256:
            break
    assert 256 < len(R["a"]) <= 512
    S = _surface(coords, cells, None, None).build(_dev(s), 0.0)
    _compare(S, R, coords, f"cube{N} slice")
    _check_gather(S, R, 13, f"cube{N} slice", n_fields=2)
    assert launch_info() == {"kernel": 6, "blocks": 2, "threads": 256, "n": S.n_vertices, "trips": 1, "grid_y": 2}


# ---- 5. interfaces --------------------------------------------------------------------------------------------------------------------
def _read_surface(path):
    """(elements, xyz, tag, kind, times, {name: [records, n_vertices]}) of a surface_<name>.xdmf through the project's decoder"""
    from cgx_hip.xdmf import XdmfFile, _local
    X = XdmfFile(path)
    steps = sorted((g for g in X.grids if g.startswith("step_")), key=lambda g: int(g[5:]))
    el, xyz, _ = X.grid(steps[0])
    cell, node, times = {}, {}, []
    for g in steps:
        for c in X.grids[g]:
            if _local(c.tag) == "Time":
                times.append(float(c.get("Value")))
            if _local(c.tag) == "Attribute":
                arr = np.asarray(X._data(X._child(c, "DataItem"))).reshape(-1)
                (cell if c.get("Center") == "Cell" else node).setdefault(c.get("Name"), []).append(arr)
    return el, xyz, cell["tag"][0], cell["kind"][0], times, {k: np.array(v) for k, v in node.items()}


def _expect_records(S, R, states, names, got, what):
    for r, st in enumerate(states):
        for nm in names:
            want, scale = SR.gather(R, st[nm][0], st[nm][1])
            err = np.abs(got[nm][r].astype(SR.LD) - want).astype(np.float64)
            assert np.all(err <= 8 * EPS * scale), (what, nm, r)


def _knp_state(p):
    st = snapshot_state(p)
    return {"Na": (st["k_i"][0], st["k_e"][0]), "K": (st["k_i"][1], st["k_e"][1]), "Cl": (st["k_i"][2], st["k_e"][2]),
            "phi": (st["phi_i"], st["phi_e"])}


def test_a_run_records_surfaces_from_the_config_and_from_add_surface(tmp_path):
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    cfg = ci_config(N=4, steps=2, kind="cube")
    cfg["output_dir"] = str(tmp_path) + os.sep
    cfg["solver"]["output"] = dict(cfg["solver"].get("output", {}), save_interval=2, surface_interval=1, clip_surfaces=[
        {"name": "half", "tags": [1], "origin": [0.43, 0.51, 0.47], "normal": [0.8, -0.5, 0.33], "fields": ["phi", "K"]},
        {"name": "slice", "side": 1, "origin": [0.43, 0.51, 0.47], "normal": [0.8, -0.5, 0.33], "boundary": False}])
    p = make_problem(cfg, "ci")
    p.solver_config["view_ksp"] = False
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    own = p.clip_surface(side=0, origin=_plane(p, "oblique")[0], normal=_plane(p, "oblique")[1])
    s.add_surface("own", own)                                   # interval: save_interval = 2
    s.add_surface("pairs", own, fields={"sum": (p.wh[0][0], None)}, interval=1)
    for bad in ("own", "half", ""):
        with pytest.raises(ValueError):
            s.add_surface(bad, own)
    s.setup_solver()
    states = [_knp_state(p)]
    unpack = s.backend.unpack

    def recording_unpack():
        unpack()
        states.append(_knp_state(p))
    s.backend.unpack = recording_unpack
    s.setup_solver = lambda: None
    s.solve()
    with pytest.raises(RuntimeError):
        s.add_surface("late", own)
    assert len(states) == 3
    lm = p.local_mesh
    sp = SR.plane_s(lm.coords, *_plane(p, "oblique"))
    cases = {"half": ((1,), True, ["phi", "K"], [0, 1, 2]), "slice": (tuple(p.extra_tag), False, ["Na", "K", "Cl", "phi"], [0, 1, 2]),
             "own": (tuple(p.intra_tags), True, ["Na", "K", "Cl", "phi"], [0, 2])}
    for name, (keep, boundary, names, steps) in cases.items():
        arrays = SR.kept_arrays(lm.coords, np.asarray(lm.cells), np.asarray(lm.cell_tags), keep, p.intra_tags, boundary)
        R = SR.cut(lm.coords, *arrays[:3], sp, 0.0, arrays[3], arrays[4])
        el, xyz, tag, kind, times, got = _read_surface(os.path.join(str(tmp_path), f"surface_{name}.xdmf"))
        assert np.array_equal(el, R["elements"]) and np.array_equal(tag, R["element_tag"]) and np.array_equal(kind, R["element_kind"]), name
        assert np.all(np.abs(xyz.astype(SR.LD) - R["xyz"]) <= 8 * EPS * np.abs(lm.coords).max())
        assert sorted(got) == sorted(names) and len(times) == len(steps) and all(got[nm].shape == (len(steps), len(R["a"])) for nm in names), name
        assert np.allclose(times, [k * float(p.dt.value) for k in steps], rtol=1e-12, atol=0.0)
        _expect_records(None, R, [states[k] for k in steps], names, got, name)
    _, _, _, _, times, got = _read_surface(os.path.join(str(tmp_path), "surface_pairs.xdmf"))
    assert len(times) == 3 and np.all(np.isnan(got["sum"][:, _host(own.vertices.side) == 1])) and not np.isnan(got["sum"]).all()
    assert not os.path.exists(os.path.join(str(tmp_path), "solution.h5")) and not os.path.exists(os.path.join(str(tmp_path), "fields.h5"))


def test_an_emi_run_records_a_surface(tmp_path):
    from cgx_hip.emi_models import g_syn
    from cgx_hip.emi_problem import ProblemEMI
    from cgx_hip.emi_solver import SolverEMI
    cfg = {"problem_type": "EMI", "dt": 5e-5, "time_steps": 2, "C_M": 0.02, "sigma_i": 0.7, "sigma_e": 1.3, "quiet": True,
           "cell_tag_file": "cube4.xdmf", "facet_tag_file": "cube4.xdmf", "mesh_conversion_factor": 1e-6,
           "ics_tags": [1], "ecs_tags": [2], "membrane_tags": [4], "output_dir": str(tmp_path) + os.sep}
    p = ProblemEMI(cfg)
    p.add_ionic_model("HH", stim_fun=g_syn)
    p.init_ionic_model()
    s = SolverEMI(p, use_direct_solver=True)
    origin, normal = _plane(p, "oblique")
    S = p.clip_surface(origin=origin, normal=normal)
    s.add_surface("intra", S, interval=2)
    s.add_surface("every", p.clip_surface(side=1, origin=origin, normal=normal, boundary=False))
    state = lambda: {"phi": (p.wh[0].numpy().copy(), p.wh[1].numpy().copy())}
    states = [state()]
    update = s.backend.update

    def recording_update(*a):
        update(*a)
        states.append(state())
    s.backend.update = recording_update
    s.solve()
    assert len(states) == 3
    lm = p.local_mesh
    sp = SR.plane_s(lm.coords, origin, normal)
    for name, keep, boundary, steps in (("intra", tuple(p.intra_tags), True, [0, 2]), ("every", tuple(p.extra_tag), False, [0, 1, 2])):
        arrays = SR.kept_arrays(lm.coords, np.asarray(lm.cells), np.asarray(lm.cell_tags), keep, p.intra_tags, boundary)
        R = SR.cut(lm.coords, *arrays[:3], sp, 0.0, arrays[3], arrays[4])
        el, xyz, tag, kind, times, got = _read_surface(os.path.join(str(tmp_path), f"surface_{name}.xdmf"))
        assert np.array_equal(el, R["elements"]) and np.array_equal(tag, R["element_tag"]) and np.array_equal(kind, R["element_kind"]), name
        assert list(got) == ["phi"] and got["phi"].shape == (len(steps), len(R["a"])) and len(times) == len(steps)
        _expect_records(None, R, [states[k] for k in steps], ["phi"], got, name)
    assert np.abs(got["phi"][-1]).max() > 0.0


def test_isochrones_of_an_activation_map(problems):
    from cgx_hip.activation import ActivationMap
    p = problems("cube4")
    lm = p.local_mesh
    f = float(p.mesh_conversion_factor)
    amap = ActivationMap(p, threshold=0.0)
    T = np.asarray(lm.coords)[amap.vertices, 0] / f                    # the front passes x at time x
    amap.state[0].copy_(torch.as_tensor(T, device=amap.state.device))
    level = 0.4                                                        # strictly between the grid planes 0.25 and 0.5
    iso = amap.isochrones([level, 0.6])
    full = np.full(len(lm.coords), NAN)
    full[amap.vertices] = T
    for lv, got in zip((level, 0.6), iso):
        R = SR.cut(lm.coords, amap.facet_vertices, np.zeros(len(amap.facets), dtype=np.int64), amap.facet_tag, full, lv)
        assert R["margin"] >= 1e-9 and got["level"] == lv
        assert np.array_equal(got["segments"], R["elements"]) and np.array_equal(got["facet"], R["element_item"])
        assert np.array_equal(got["tag"], R["element_tag"])
        assert np.all(np.abs(got["xyz"].astype(SR.LD) - R["xyz"]) <= 8 * EPS * np.abs(lm.coords).max())
        total = got["length"].sum()
        print(f"isochrone T = {lv}: {len(got['segments'])} segments, length {total / f!r}")
        assert abs(total - 2.0 * f) <= 1e-13 * f                        # the perimeter of the box [0.25, 0.75]^2
        assert np.all(np.abs(got["xyz"][:, 0] - lv * f) <= 8 * EPS * f)
    # a vertex that did not fire takes its facets out
    dead = int(np.argmin(np.abs(T - 0.5) + np.abs(np.asarray(lm.coords)[amap.vertices, 1] / f - 0.5)))
    amap.state[0, dead] = NAN
    full[amap.vertices[dead]] = NAN
    got = amap.isochrones(level)[0]
    R = SR.cut(lm.coords, amap.facet_vertices, np.zeros(len(amap.facets), dtype=np.int64), amap.facet_tag, full, level)
    assert np.array_equal(got["segments"], R["elements"]) and np.array_equal(got["facet"], R["element_item"])
    assert len(got["segments"]) < len(iso[0]["segments"]) and not np.isnan(got["xyz"]).any()
    assert not np.isin(amap.vertices[dead], amap.facet_vertices[got["facet"]])


def test_isochrones_of_a_2d_membrane_are_refused(problems):
    from cgx_hip.activation import ActivationMap
    with pytest.raises(ValueError):
        ActivationMap(problems("delaunay2d_12"), threshold=0.0).isochrones([0.5])


# ---- 6. errors and determinism ------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing():
    from cgx_hip import _lib
    from cgx_hip.surfaces import launch_info
    lib = _lib.load()
    dev = torch.device("cuda")
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=dev)
    items, s, counts, x = i32(2, 4), f64(8), i32(3), f64(8, 3)
    bf, bi = i32(1, 3), i32(1)
    assert lib.knp_surface_count(4, 2, 8, items.data_ptr(), 1, bf.data_ptr(), bi.data_ptr(), s.data_ptr(), 0.0, counts.data_ptr(), None) == 0
    torch.cuda.synchronize()
    before = launch_info()
    assert before["kernel"] == 2 and before["n"] == 3
    P = lambda t: t.data_ptr()
    o3 = (C.c_double * 3)(0.0, 0.0, 0.0)
    off, keys, ei, et, ek = torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(6, dtype=torch.int64, device=dev), i32(2), i32(2), u8(2)
    a, b, w, sd, xyz, out = i32(4), i32(4), f64(4), u8(4), f64(4, 3), f64(4)
    tab = (C.c_void_p * 1)(P(s))
    big = 2 ** 31
    bad = [
        lambda: lib.knp_surface_plane(4, 8, P(x), o3, o3, P(s), None), lambda: lib.knp_surface_plane(3, 8, None, o3, o3, P(s), None),
        lambda: lib.knp_surface_plane(3, 8, P(x), None, o3, P(s), None), lambda: lib.knp_surface_plane(3, big, P(x), o3, o3, P(s), None),
        lambda: lib.knp_surface_plane(3, -1, P(x), o3, o3, P(s), None),
        lambda: lib.knp_surface_count(5, 2, 8, P(items), 0, None, None, P(s), 0.0, P(counts), None),
        lambda: lib.knp_surface_count(2, 2, 8, P(items), 0, None, None, P(s), 0.0, P(counts), None),
        lambda: lib.knp_surface_count(4, -1, 8, P(items), 0, None, None, P(s), 0.0, P(counts), None),
        lambda: lib.knp_surface_count(4, big, 8, P(items), 0, None, None, P(s), 0.0, P(counts), None),
        lambda: lib.knp_surface_count(4, 2, 0, P(items), 0, None, None, P(s), 0.0, P(counts), None),
        lambda: lib.knp_surface_count(4, 2, 8, None, 0, None, None, P(s), 0.0, P(counts), None),
        lambda: lib.knp_surface_count(4, 2, 8, P(items), 1, None, P(bi), P(s), 0.0, P(counts), None),
        lambda: lib.knp_surface_count(4, 2, 8, P(items), 1, P(bf), None, P(s), 0.0, P(counts), None),
        lambda: lib.knp_surface_count(4, 2, 8, P(items), 0, None, None, None, 0.0, P(counts), None),
        lambda: lib.knp_surface_count(4, 2, 8, P(items), 0, None, None, P(s), 0.0, None, None),
        lambda: lib.knp_surface_emit(2, 4, 2, 8, P(items), P(u8(2)), P(i32(2)), 0, None, None, P(s), 0.0, P(x), P(off), 2, P(keys), P(ei), P(et), P(ek), None),
        lambda: lib.knp_surface_emit(3, 4, 2, 8, P(items), None, P(i32(2)), 0, None, None, P(s), 0.0, P(x), P(off), 2, P(keys), P(ei), P(et), P(ek), None),
        lambda: lib.knp_surface_emit(3, 4, 2, 8, P(items), P(u8(2)), P(i32(2)), 0, None, None, P(s), 0.0, None, P(off), 2, P(keys), P(ei), P(et), P(ek), None),
        lambda: lib.knp_surface_emit(3, 4, 2, 8, P(items), P(u8(2)), P(i32(2)), 0, None, None, P(s), 0.0, P(x), None, 2, P(keys), P(ei), P(et), P(ek), None),
        lambda: lib.knp_surface_emit(3, 4, 2, 8, P(items), P(u8(2)), P(i32(2)), 0, None, None, P(s), 0.0, P(x), P(off), big, P(keys), P(ei), P(et), P(ek), None),
        lambda: lib.knp_surface_emit(3, 4, 2, 8, P(items), P(u8(2)), P(i32(2)), 0, None, None, P(s), 0.0, P(x), P(off), 2, None, P(ei), P(et), P(ek), None),
        lambda: lib.knp_surface_vertices(1, 8, 4, P(keys), P(s), 0.0, P(x), P(a), P(b), P(w), P(sd), P(xyz), None),
        lambda: lib.knp_surface_vertices(3, 0, 4, P(keys), P(s), 0.0, P(x), P(a), P(b), P(w), P(sd), P(xyz), None),
        lambda: lib.knp_surface_vertices(3, 8, -1, P(keys), P(s), 0.0, P(x), P(a), P(b), P(w), P(sd), P(xyz), None),
        lambda: lib.knp_surface_vertices(3, 8, 4, None, P(s), 0.0, P(x), P(a), P(b), P(w), P(sd), P(xyz), None),
        lambda: lib.knp_surface_vertices(3, 8, 4, P(keys), P(s), 0.0, P(x), P(a), P(b), None, P(sd), P(xyz), None),
        lambda: lib.knp_surface_remap(-1, 4, P(keys), P(keys), P(i32(6)), None), lambda: lib.knp_surface_remap(6, big, P(keys), P(keys), P(i32(6)), None),
        lambda: lib.knp_surface_remap(6, 4, None, P(keys), P(i32(6)), None), lambda: lib.knp_surface_remap(6, 4, P(keys), None, P(i32(6)), None),
        lambda: lib.knp_surface_remap(6, 4, P(keys), P(keys), None, None),
        lambda: lib.knp_surface_gather(17, 4, P(a), P(b), P(w), P(sd), tab, tab, P(out), None),
        lambda: lib.knp_surface_gather(-1, 4, P(a), P(b), P(w), P(sd), tab, tab, P(out), None),
        lambda: lib.knp_surface_gather(1, 4, P(a), P(b), P(w), P(sd), None, None, P(out), None),
        lambda: lib.knp_surface_gather(1, 4, None, P(b), P(w), P(sd), tab, tab, P(out), None),
        lambda: lib.knp_surface_gather(1, 4, P(a), P(b), P(w), P(sd), tab, tab, None, None),
        lambda: lib.knp_surface_gather(1, big, P(a), P(b), P(w), P(sd), tab, tab, P(out), None),
        lambda: lib.knp_surface_measure(2, 3, 2, 4, P(i32(2, 3)), P(xyz), P(out), None),
        lambda: lib.knp_surface_measure(3, 4, 2, 4, P(i32(2, 3)), P(xyz), P(out), None),
        lambda: lib.knp_surface_measure(3, 3, 2, 4, None, P(xyz), P(out), None),
        lambda: lib.knp_surface_measure(3, 3, -2, 4, P(i32(2, 3)), P(xyz), P(out), None),
        lambda: lib.knp_surface_get_info(None, 6),
    ]
    for k, call in enumerate(bad):
        assert call() == E_ARG, k
        assert launch_info() == before, k
    # zero counts are successful no-ops that launch nothing either
    assert lib.knp_surface_count(4, 0, 8, None, 0, None, None, P(s), 0.0, None, None) == 0
    assert lib.knp_surface_gather(0, 4, P(a), P(b), P(w), P(sd), tab, tab, P(out), None) == 0
    assert lib.knp_surface_gather(1, 0, None, None, None, None, tab, tab, None, None) == 0
    assert launch_info() == before
    torch.cuda.synchronize()


def test_more_than_one_rank_is_refused(problems):
    from cgx_hip.surfaces import ClipSurface, IsoSurface, LevelSetSurface
    p = problems("cube4")
    fake = types.SimpleNamespace(comm=types.SimpleNamespace(size=2, rank=0), local_mesh=p.local_mesh, mesh=p.mesh, intra_tags=p.intra_tags,
                                 extra_tag=p.extra_tag, cell_side=p.cell_side)
    for make in (lambda: ClipSurface(fake, origin=[0, 0, 0], normal=[1, 0, 0]), lambda: IsoSurface(fake, p.wh[0][0]),
                 lambda: LevelSetSurface(fake, np.asarray(p.local_mesh.cells))):
        with pytest.raises(NotImplementedError, match="runs on one rank"):
            make()


def test_two_builds_give_the_same_bits(problems):
    from cgx_hip.surfaces import ClipSurface
    p = problems("hub3d_5_60")
    first = ClipSurface(p, origin=_plane(p, "oblique")[0], normal=_plane(p, "oblique")[1])
    keep = [t.clone() for t in (first.elements, first.element_item, first.element_tag, first.element_kind, first.keys, first.vertices.a,
                                first.vertices.b, first.vertices.w, first.vertices.side, first.xyz)]
    again = [first.move(first.origin, first.normal), ClipSurface(p, origin=first.origin, normal=first.normal)]
    for S in again:
        now = (S.elements, S.element_item, S.element_tag, S.element_kind, S.keys, S.vertices.a, S.vertices.b, S.vertices.w, S.vertices.side, S.xyz)
        assert all(torch.equal(x, y) for x, y in zip(keep, now))


def test_oversized_record_buffers_and_unbuilt_surfaces_are_refused(problems):
    from cgx_hip._lib import KnpError
    from cgx_hip.surfaces import LevelSetSurface, SurfaceRecorder
    p = problems("cube4")
    S = p.clip_surface(origin=_plane(p, "oblique")[0], normal=_plane(p, "oblique")[1])
    with pytest.raises(ValueError, match="more than the"):
        SurfaceRecorder("big", S, ["phi"], [p.wh[0][3]], [p.wh[1][3]], 1, 2 ** 30 // S.n_vertices, "unused")
    raw = LevelSetSurface(p, np.asarray(p.local_mesh.cells))
    with pytest.raises(KnpError):
        raw([p.wh[0][0]], None)
    assert S.plan_bytes == S.n_vertices * 49 + S.n_elements * 21
