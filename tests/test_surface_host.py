"""The NumPy restatement of the level-set cut (tests/surface_ref.py) and the inputs of tests/test_gpu_surfaces.py are sound: the
surfaces it produces are closed, consistently oriented and have the areas, volumes and counts geometry gives.  No GPU.

Every input keeps |t_v| exactly 0 by construction or at least 1e-9 max|s| away from 0 (asserted through ``margin``), so that no
inside / outside decision of the GPU tests depends on rounding."""
import math

import numpy as np
import pytest

import irregular_meshes as IM
import surface_ref as SR


def _clip(N, keep, origin, normal, boundary=True, intra=(1,)):
    coords, cells, tags = SR.cube(N)
    items, side, ref, bf, bi, _ = SR.kept_arrays(coords, cells, tags, keep, intra, boundary)
    return SR.cut(coords, items, side, ref, SR.plane_s(coords, origin, normal), 0.0, bf, bi)


def _zero_area(R):
    return int((SR.measures(R["xyz"], R["elements"]) == 0.0).sum())


def test_aligned_clip_of_the_box_has_the_counts_of_the_prototype():
    R = _clip(4, (1,), (0.5, 0.0, 0.0), (1.0, 0.0, 0.0))
    assert R["margin"] >= 1e-9
    assert len(R["elements"]) == 80 and _zero_area(R) == 48
    assert abs(SR.measures(R["xyz"], R["elements"]).sum() - 1.0) <= 1e-14
    assert abs(SR.enclosed_volume(R["xyz"], R["elements"]) - 0.0625) <= 1e-15
    assert SR.topology(R["elements"]) == (True, 2)


@pytest.mark.parametrize("N", [4, 6])
@pytest.mark.parametrize("plane", ["aligned", "oblique", "all_inside"])
def test_single_side_clips_are_closed_and_oriented(N, plane):
    origin, normal = {"aligned": ((0.5, 0.0, 0.0), (1.0, 0.0, 0.0)), "oblique": SR.OBLIQUE, "all_inside": ((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0))}[plane]
    R = _clip(N, (1,), origin, normal)
    assert R["margin"] >= 1e-9
    assert SR.topology(R["elements"]) == (True, 2)
    assert SR.enclosed_volume(R["xyz"], R["elements"]) > 0.0
    if plane == "all_inside":
        side = {4: 0.5, 6: 1.0 / 3.0}[N]        # the box of cells with every vertex in [0.25, 0.75]^3
        assert np.all(R["element_kind"] == 1) and abs(SR.measures(R["xyz"], R["elements"]).sum() - 6.0 * side * side) <= 1e-14


@pytest.mark.parametrize("N,zero", [(4, 132), (6, None)])
def test_diagonal_slice_of_all_cells(N, zero):
    coords, cells, tags = SR.cube(N)
    items, side, ref, _, _, _ = SR.kept_arrays(coords, cells, tags, (1, 2), (1,), False)
    R = SR.cut(coords, items, side, ref, SR.diagonal_s(coords, N), 1.5 * N)
    assert R["margin"] >= 1e-9 and np.all(R["element_kind"] == 0)
    assert abs(SR.measures(R["xyz"], R["elements"]).sum() - 3.0 * math.sqrt(3.0) / 4.0) <= 1e-13
    if zero is not None:
        assert _zero_area(R) == zero


def test_iso_surface_of_a_sphere_is_closed_with_outward_normals():
    coords, cells, tags = SR.cube(6)
    items, side, ref, _, _, _ = SR.kept_arrays(coords, cells, tags, (1, 2), (1, 2), False)
    R = SR.cut(coords, items, side, ref, SR.sphere_s(coords), 0.0)
    assert R["margin"] >= 1e-9
    assert SR.topology(R["elements"]) == (True, 2)
    vol = SR.enclosed_volume(R["xyz"], R["elements"])      # normals toward decreasing s: the ball s >= 0 is enclosed, volume positive
    assert 0.5 * 4.0 / 3.0 * math.pi * 0.4 ** 3 < vol < 4.0 / 3.0 * math.pi * 0.4 ** 3


def test_two_sides_leave_a_seam_along_the_membrane():
    coords, cells, tags = IM.mesh("delaunay3d_5")
    t2 = IM.two_tag(coords, cells, tags)
    items, side, ref, bf, bi, _ = SR.kept_arrays(coords, cells, t2, (1, 2, 3), (2, 3), True)
    R = SR.cut(coords, items, side, ref, SR.plane_s(coords, *SR.OBLIQUE), 0.0, bf, bi)
    assert R["margin"] >= 1e-9 and set(np.unique(R["side"])) == {0, 1}
    assert not SR.topology(R["elements"])[0]
    assert SR.topology(R["elements"], merge=np.column_stack([R["a"], R["b"]])) == (True, 2)


@pytest.mark.parametrize("name", ["delaunay3d_5", "hub3d_5_60"])
def test_irregular_and_reoriented_meshes_clip_to_closed_surfaces(name):
    coords, cells, tags = IM.mesh(name)
    for c in (cells, SR.permuted_cells(cells, 23)):
        items, side, ref, bf, bi, _ = SR.kept_arrays(coords, c, tags, (1,), (1,), True)
        R = SR.cut(coords, items, side, ref, SR.plane_s(coords, *SR.OBLIQUE), 0.0, bf, bi)
        assert R["margin"] >= 1e-9 and len(R["elements"]) > 0
        # the intracellular cells of these meshes are no ball (cells that meet in an edge, handles): what every boundary of a solid
        # has is that each directed edge occurs as often as its reverse, and a positive enclosed volume
        assert SR.balanced(R["elements"])
        assert SR.enclosed_volume(R["xyz"], R["elements"]) > 0.0


@pytest.mark.parametrize("name", ["delaunay2d_12", "hub2d_12_40"])
def test_isolines_of_2d_meshes_bound_the_kept_area(name):
    """2D: the clipped boundary of the intracellular cells is a closed polygon, walked counter-clockwise (the kept part to the left):
    its shoelace area equals the kept area"""
    coords, cells, tags = IM.mesh(name)
    origin, normal = SR.OBLIQUE[0][:2], SR.OBLIQUE[1][:2]
    s = SR.plane_s(coords, origin, normal)
    for c in (cells, SR.permuted_cells(cells, 29)):
        items, side, ref, bf, bi, _ = SR.kept_arrays(coords, c, tags, (1,), (1,), True)
        R = SR.cut(coords, items, side, ref, s, 0.0, bf, bi)
        assert R["margin"] >= 1e-9
        el = R["elements"]
        assert np.array_equal(np.sort(el[:, 0]), np.sort(el[:, 1])) and len(np.unique(el[:, 0])) == len(el)      # every vertex: one in, one out
        X = np.asarray(R["xyz"], dtype=np.float64)[el]
        shoelace = 0.5 * float((X[:, 0, 0] * X[:, 1, 1] - X[:, 1, 0] * X[:, 0, 1]).sum())
        # the kept area: every intracellular triangle clipped to the half-plane, by the same cut of its three edges
        area = 0.0
        for tri in items:
            P = [coords[v] for v in tri]
            sv = [s[v] for v in tri]
            poly = []
            for k in range(3):
                a, b = k, (k + 1) % 3
                if sv[a] >= 0:
                    poly.append(P[a])
                if (sv[a] >= 0) != (sv[b] >= 0):
                    poly.append(P[a] + (P[b] - P[a]) * (sv[a] / (sv[a] - sv[b])))
            if len(poly) >= 3:
                Q = np.array(poly)
                area += 0.5 * abs(float((Q[:, 0] * np.roll(Q[:, 1], -1) - np.roll(Q[:, 0], -1) * Q[:, 1]).sum()))
        assert abs(shoelace - area) <= 1e-12, (shoelace, area)
