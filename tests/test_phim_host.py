"""Host side of the per-tag membrane potential (cgx_hip/diagnostics.py, cgx_hip/output.py): the NumPy checker of the GPU tests
(tests/phim_ref.py) on fields whose answer is known by hand, ``threshold_crossings``, the per-tag probe vertices and the
``save_membrane_potentials`` output key.  CPU only."""
import copy

import numpy as np
import pytest

from parity_utils import ci_config, make_problem, tissue_config
from phim_ref import TOL, facet_vertices, phim_ref


def _problem(cfg):
    from cgx_hip.problem import ProblemKNPEMI
    return ProblemKNPEMI(cfg)


@pytest.mark.parametrize("case,n_facets,n_tags", [("square16", 32, 1), ("cube8", 192, 1), ("tissue2d_18_3", 144, 9),
                                                   ("tissue3d_12_2", 1536, 8)])
def test_reference_on_a_constant_field(case, n_facets, n_tags):
    cfg = {"square16": lambda: ci_config(N=16, steps=1), "cube8": lambda: ci_config(N=8, steps=1, kind="cube"),
           "tissue2d_18_3": lambda: tissue_config(2, 18, 3), "tissue3d_12_2": lambda: tissue_config(3, 12, 2)}[case]()
    p = _problem(cfg)
    lm = p.local_mesh
    tags = [int(t) for t in p.gamma_tags]
    assert lm.gamma.shape[0] == n_facets and len(tags) == n_tags
    c = -0.0678
    I, A, lo, hi, S, cover = phim_ref(p, np.full(lm.coords.shape[0], c), [[t] for t in tags] + [[987654]])
    assert [len(q) for q in cover] == [n_facets // n_tags] * n_tags + [0]
    assert np.all(lo[:-1] == c) and np.all(hi[:-1] == c)
    assert np.all(np.abs(I[:-1] / A[:-1] - c) <= TOL * S[:-1] / A[:-1]) and np.allclose(S[:-1], abs(c) * A[:-1], rtol=1e-13)
    assert (I[-1], A[-1], S[-1], lo[-1], hi[-1]) == (0.0, 0.0, 0.0, np.inf, -np.inf)
    # the areas are the library's: facet measures of the problem, summed per group
    from cgx_hip.diagnostics import facet_areas, facet_group_map
    seg_ptr, facets = facet_group_map(p, [[t] for t in tags] + [[987654]])
    assert np.allclose(facet_areas(p, seg_ptr, facets), A, rtol=1e-13, atol=0)
    for t in range(len(tags) + 1):
        assert sorted(facets[seg_ptr[t]:seg_ptr[t + 1]]) == sorted(cover[t])


def test_reference_on_a_linear_field_gives_the_centre_of_the_closed_membrane():
    """phi = a.x on the membrane of the cube inclusion: the surface of an axis-aligned box has its centroid at the box's centre, and
    the P1 integral of a linear field is exact, so mean = a . centre."""
    p = _problem(ci_config(N=8, steps=1, kind="cube"))
    x = np.asarray(p.local_mesh.coords)
    mv = np.unique(facet_vertices(p))
    centre = 0.5 * (x[mv].min(axis=0) + x[mv].max(axis=0))
    a = np.array([3.0e4, -1.0e4, 2.0e4])
    I, A, lo, hi, S, cover = phim_ref(p, x @ a, [list(p.gamma_tags)])
    assert len(cover[0]) == 192
    want = float(a @ centre)
    assert abs(want) > 1e3 * TOL * S[0] / A[0], "the expected value drowns in the bound"
    assert abs(I[0] / A[0] - want) <= TOL * S[0] / A[0]
    assert lo[0] == (x[mv] @ a).min() and hi[0] == (x[mv] @ a).max() and lo[0] < want < hi[0]
    side = x[mv].max(axis=0) - x[mv].min(axis=0)
    assert A[0] == pytest.approx(2.0 * (side[0] * side[1] + side[1] * side[2] + side[0] * side[2]), rel=1e-12)


def test_reduce_over_ranks_and_groups_without_facets():
    from cgx_hip.diagnostics import reduce_membrane_potential
    inf = np.inf
    r0 = np.array([[2.0, -1.0, 3.0], [0.0, inf, -inf], [0.0, inf, -inf]])
    r1 = np.array([[4.0, -2.0, 1.0], [1.0, 0.5, 0.5], [0.0, inf, -inf]])
    area, val = reduce_membrane_potential([r0, r1], [np.array([1.0, 0.0, 0.0]), np.array([2.0, 2.0, 0.0])])
    assert list(area) == [3.0, 2.0, 0.0]
    assert np.array_equal(val[:2], [[2.0, -2.0, 3.0], [0.5, 0.5, 0.5]]) and np.all(np.isnan(val[2]))
    area, val = reduce_membrane_potential([np.stack([r0, r1])], [np.array([1.0, 2.0, 0.0])])      # a trace: [records, n, 3]
    assert val.shape == (2, 3, 3) and val[0, 0, 0] == 2.0 and val[1, 1, 0] == 0.5 and np.all(np.isnan(val[:, 2]))


def test_threshold_crossings():
    from cgx_hip.diagnostics import threshold_crossings
    t = np.arange(9) * 0.5
    v = np.stack([np.full(9, -70.0),                                             # never
                  [-70, -40, -20, 30, 10, -50, -70, -70, -70],                   # exactly at a sample (record 2)
                  [-70, 30, -70, -70, -60, 20, 40, -30, -70],                    # two spikes; the first between records 0 and 1
                  [10, 20, 30, 30, 20, 10, 0, -10, 0]], axis=1).astype(float)    # never below the threshold
    count, first = threshold_crossings(v, t, -20.0)
    assert count.dtype == np.int64 and list(count) == [0, 1, 2, 0]
    assert np.isnan(first[0]) and np.isnan(first[3])
    assert first[1] == 1.0
    assert first[2] == pytest.approx(0.25, rel=1e-15)
    count, first = threshold_crossings(v[:, 2], t, -20.0)                        # one column
    assert list(count) == [2] and first[0] == pytest.approx(0.25, rel=1e-15)
    count, first = threshold_crossings(v[:1], t[:1], -20.0)
    assert list(count) == [0] * 4 and np.all(np.isnan(first))
    with pytest.raises(ValueError):
        threshold_crossings(v, t[:-1], 0.0)


@pytest.mark.parametrize("case", ["square16", "tissue3d_12_2"])
def test_probe_vertices_follow_the_measurement_vertex_rule(case):
    from cgx_hip.output import find_membrane_measurement_vertex, find_membrane_probe_vertices
    p = make_problem(ci_config(N=16, steps=1) if case == "square16" else tissue_config(3, 12, 2, steps=1), "ci")
    find_membrane_measurement_vertex(p)
    tags = [int(t) for t in p.gamma_tags] + [987654]
    pr = find_membrane_probe_vertices(p, tags)
    k = tags.index(int(p.membrane_data_tag))
    assert pr["vertex"][k] == p.png_dof and pr["owner"][k] == p.owner_rank_membrane_vertex
    assert np.array_equal(pr["xyz"][k], p.png_point[0])
    assert pr["owner"][-1] == -1 and pr["vertex"][-1] == -1 and np.all(np.isnan(pr["xyz"][-1]))
    # every probe is a vertex of its own tag's facets, and none of them is closer to the centre
    x = np.asarray(p.local_mesh.coords)
    centre = 0.5 * (x.min(axis=0) + x.max(axis=0))
    fv, ftags = facet_vertices(p), np.asarray(p.local_mesh.gamma_tags)
    for t, tag in enumerate(tags[:-1]):
        mv = np.unique(fv[ftags == tag])
        dist = ((x[mv] - centre) ** 2).sum(axis=1)
        assert pr["vertex"][t] == mv[np.argmin(dist)]


def test_output_key_parsing():
    from cgx_hip.output import parse_membrane_potential_keys
    from cgx_hip.solver import SolverKNPEMI
    assert parse_membrane_potential_keys({}, (3, 4)) == (None, 1)
    assert parse_membrane_potential_keys({"save_membrane_potentials": False}, (3, 4)) == (None, 1)
    assert parse_membrane_potential_keys({"save_membrane_potentials": True}, (3, 4)) == ([3, 4], 1)
    assert parse_membrane_potential_keys({"save_membrane_potentials": [4], "membrane_potential_interval": 5}, (3, 4)) == ([4], 5)
    for bad in ({"save_membrane_potentials": "all"}, {"save_membrane_potentials": [3, 3]}, {"save_membrane_potentials": [1.5]},
                {"save_membrane_potentials": True, "membrane_potential_interval": 0}):
        with pytest.raises(ValueError):
            parse_membrane_potential_keys(bad, (3, 4))
    cfg = tissue_config(2, 18, 3, steps=1)
    p = _problem(cfg)
    assert SolverKNPEMI.membrane_potential_tags is None
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    assert s.membrane_potential_tags is None and s.membrane_potential_interval == 1
    for key, want in ((True, [int(t) for t in p.gamma_tags]), ([5, 2], [5, 2])):
        cfg2 = copy.deepcopy(cfg)
        cfg2["solver"]["output"].update({"save_membrane_potentials": key, "membrane_potential_interval": 2})
        p2 = _problem(cfg2)
        s2 = SolverKNPEMI(p2, solver_config=p2.solver_config)
        assert s2.membrane_potential_tags == want and s2.membrane_potential_interval == 2
