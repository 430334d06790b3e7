"""Host side of the per-tag diagnostics (cgx_hip/diagnostics.py): the tag maps the HIP kernels reduce over, the time-invariant
per-tag volumes and membrane areas, and the ``save_ion_budget`` output key.  CPU only."""
import copy

import numpy as np
import pytest

from parity_utils import ci_config, tissue_config

S = 1e-6     # mesh_conversion_factor of the generated configs


def _problem(cfg):
    from cgx_hip.problem import ProblemKNPEMI
    return ProblemKNPEMI(cfg)


@pytest.mark.parametrize("dim,N,m", [(2, 18, 3), (3, 12, 2), (2, 24, 6)])
def test_cell_tag_map_on_tissue_lattice(dim, N, m):
    from cgx_hip.diagnostics import BudgetLayout
    p = _problem(tissue_config(dim, N, m, stimulus=False))
    lm = p.local_mesh
    lay = BudgetLayout(p)
    assert lay.n_tags == m ** dim + 1 >= 8
    assert list(lay.tags) == list(p.intra_tags) + [1]
    assert list(lay.side) == [0] * m ** dim + [1]
    nco = int(lm.n_cells_owned)
    # every owned cell in exactly one segment
    assert lay.cells.dtype == np.int32 and lay.seg_ptr.dtype == np.int32
    assert np.array_equal(np.sort(lay.cells), np.arange(nco))
    # segments contiguous, in tag order, each holding exactly the cells of its tag (ascending cell ids: stable sort)
    assert lay.seg_ptr[0] == 0 and lay.seg_ptr[-1] == nco and np.all(np.diff(lay.seg_ptr) >= 0)
    for t, tag in enumerate(lay.tags):
        seg = lay.cells[lay.seg_ptr[t]:lay.seg_ptr[t + 1]]
        assert seg.size > 0
        assert np.all(lm.cell_tags[seg] == tag)
        assert np.all(np.diff(seg) > 0)
    # per-tag volumes sum to the domain volume; every cell has the closed-form volume of the lattice generator
    assert lay.volume.sum() == pytest.approx(S ** dim, rel=1e-12)
    assert np.all(lay.volume[:-1] > 0)
    # membrane tag = cell tag: every cell's area is the boundary of its box
    assert np.all(lay.area[:-1] > 0) and lay.area[-1] == 0.0


@pytest.mark.parametrize("kind,N,vol,area", [("square", 16, 0.25, 2.0), ("cube", 8, 0.125, 1.5)])
def test_volumes_and_areas_of_the_generated_boxes(kind, N, vol, area):
    from cgx_hip.diagnostics import BudgetLayout, owned_facets, tag_map
    p = _problem(ci_config(N=N, steps=1, kind=kind))
    d = 2 if kind == "square" else 3
    lay = BudgetLayout(p)
    assert list(lay.tags) == [1, 2] and list(lay.side) == [0, 1]
    assert lay.volume[0] == pytest.approx(vol * S ** d, rel=1e-12)
    assert lay.volume[1] == pytest.approx((1.0 - vol) * S ** d, rel=1e-12)
    # dS(tag) of the reference: the membrane facets carry tag 4, not a cell tag -> no area for either cell tag
    assert np.array_equal(lay.area, [0.0, 0.0])
    # the facet map of the membrane integrals: the inner box's boundary
    own = np.nonzero(owned_facets(p))[0]
    fptr, fitems = tag_map(np.asarray(p.gamma_facet_tags)[own], [4])
    assert fptr[-1] == len(own) == len(p.gamma_facet_tags)
    assert p._fmeas[own[fitems]].sum() == pytest.approx(area * S ** (d - 1), rel=1e-12)


def test_tissue_areas_match_the_closed_form():
    from cgx_hip.diagnostics import BudgetLayout
    dim, N, m = 3, 12, 2
    p = _problem(tissue_config(dim, N, m, stimulus=False))
    lay = BudgetLayout(p)
    side = (N // m - 2) / N            # generator: blocks of N/m voxels holding a cube of N/m - 2 voxels
    assert np.allclose(lay.volume[:-1], (side * S) ** dim, rtol=1e-12, atol=0)
    assert np.allclose(lay.area[:-1], 2 * dim * (side * S) ** (dim - 1), rtol=1e-12, atol=0)


def test_tag_map_leaves_out_unlisted_tags_and_keeps_order():
    from cgx_hip.diagnostics import tag_map
    tags = np.array([7, 3, 9, 3, 7, 5, 3])
    seg_ptr, items = tag_map(tags, [3, 7, 1])
    assert list(seg_ptr) == [0, 3, 5, 5]
    assert list(items) == [1, 3, 6, 0, 4]
    with pytest.raises(ValueError):
        tag_map(tags, [3, 3])
    seg_ptr, items = tag_map(tags, [])
    assert list(seg_ptr) == [0] and items.size == 0


def test_save_ion_budget_defaults_to_off():
    from cgx_hip.solver import SolverKNPEMI
    cfg = ci_config(N=16, steps=1)
    p = _problem(cfg)
    assert SolverKNPEMI.save_ion_budget is False
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    assert s.save_ion_budget is False
    cfg2 = copy.deepcopy(cfg)
    cfg2["solver"]["output"]["save_ion_budget"] = True
    p2 = _problem(cfg2)
    assert SolverKNPEMI(p2, solver_config=p2.solver_config).save_ion_budget is True


def test_diagnostic_program_keeps_the_field_table():
    """the stimulus expression compiles against the mechanism programs' field roles and adds no auxiliary field"""
    from cgx_hip import fem
    from cgx_hip.configs import make_problem
    from cgx_hip.diagnostics import membrane_program
    p = make_problem(tissue_config(2, 16, 2, stimulus=True), "ci")
    n_aux = len(p.aux_functions)
    spec = membrane_program(p, p.stim_ufl_expr)
    assert len(p.aux_functions) == n_aux
    ops = {v: k for k, v in fem.OPS.items()}
    outs = [r for r in spec.code.tolist() if r[0] == 27]           # OUT
    assert len(outs) == 1 and outs[0][2] == 0
    assert all(ops[r[0]] != "AUX" for r in spec.code.tolist())
    with pytest.raises(ValueError):
        membrane_program(p, fem.Function(p.V, "not_read_by_any_mechanism") * 1.0)
