"""Host side of the trans-membrane ion fluxes (cgx_hip/fluxes.py, cgx_hip/diagnostics.py): the NumPy checker of the GPU tests
(tests/flux_ref.py) against the divergence theorem, the ``CGx.utils.calc_fluxes`` import path, the ``save_fluxes`` output key and
the facet-group maps.  CPU only."""
import copy

import numpy as np
import pytest

from flux_ref import TOL, flux_ref, intra_volume, region_box
from parity_utils import ci_config, tissue_config


def _problem(cfg):
    from cgx_hip.problem import ProblemKNPEMI
    return ProblemKNPEMI(cfg)


def _config(case, **kw):
    if case == "square16":
        return ci_config(N=16, steps=1)
    if case == "cube8":
        return ci_config(N=8, steps=1, kind="cube")
    if case == "tissue2d_18_3":
        return tissue_config(2, 18, 3, **kw)
    return tissue_config(3, 12, 2, **kw)


@pytest.mark.parametrize("case,n_facets", [("square16", 32), ("cube8", 192), ("tissue2d_18_3", 144), ("tissue3d_12_2", 1536)])
def test_reference_obeys_the_divergence_theorem_on_affine_fields(case, n_facets):
    """c = g.x, phi = h.x on both sides, D = 1: the flux density -(g + (z/psi) (g.x) h) has divergence -(z/psi) g.h, so the closed
    membranes of the intracellular cells pass -(z/psi) (g.h) V_intra out of the intracellular side and the opposite amount out
    of the extracellular side (its normal is reversed, the affine fields are the same)."""
    p = _problem(_config(case, stimulus=False) if case.startswith("tissue") else _config(case))
    lm = p.local_mesh
    assert lm.gamma.shape[0] == n_facets
    d = lm.coords.shape[1]
    rng = np.random.default_rng(5)
    g, h = rng.uniform(0.5, 2.0, d) * 1e7, rng.uniform(0.5, 2.0, d) * 1e4
    c, ph = lm.coords @ g, lm.coords @ h
    zpsi = np.array([38.7, 38.7, -38.7])
    fields = {"k_i": [c, 2.0 * c, 3.0 * c], "k_e": [c, 2.0 * c, 3.0 * c], "phi_i": ph, "phi_e": ph}
    flux, S, cover = flux_ref(p, fields, np.ones(3), zpsi, [list(p.gamma_tags)])
    assert len(cover[0]) == n_facets and np.allclose(cover[0], 1.0, rtol=1e-14)
    V = intra_volume(p)
    for k, mult in enumerate((1.0, 2.0, 3.0)):
        want = -zpsi[k] * mult * float(g @ h) * V
        assert abs(want) > 1e3 * TOL * S[0, 0, k], "the expected value drowns in the bound: the check would be vacuous"
        assert abs(flux[0, 0, k] - want) <= TOL * S[0, 0, k]
        assert abs(flux[0, 1, k] + want) <= TOL * S[0, 1, k]
    # pure diffusion (z = 0): nothing leaves a closed surface in a constant gradient
    flux0, S0, _ = flux_ref(p, fields, np.ones(3), np.zeros(3), [list(p.gamma_tags)])
    assert np.all(np.abs(flux0) <= TOL * S0) and np.all(S0 > 0)


def test_reference_mask_counts_quadrature_points_strictly_inside():
    p = _problem(tissue_config(2, 18, 3, stimulus=True))
    assert region_box(p) == [(0, 0.0, 0.5e-6)]
    lm = p.local_mesh
    one = np.ones(lm.coords.shape[0])
    fields = {"k_i": [one] * 3, "k_e": [one] * 3, "phi_i": one, "phi_e": one}
    _, _, cover = flux_ref(p, fields, np.ones(3), np.ones(3), [[t] for t in p.gamma_tags], box=[(0, 0.0, 0.47e-6)])
    allc = np.concatenate(cover)
    assert (allc == 0).any() and np.isclose(allc, 1.0).any() and ((allc > 0) & (allc < 1 - 1e-12)).any()


def test_calc_fluxes_import_path_and_handle_order():
    from CGx.utils.calc_fluxes import compute_fluxes, create_flux_forms
    from cgx_hip import fluxes
    from cgx_hip.configs import make_problem
    assert create_flux_forms is fluxes.create_flux_forms and compute_fluxes is fluxes.compute_fluxes
    p = make_problem(tissue_config(2, 18, 3, stimulus=True), "ci")
    forms = create_flux_forms(p)
    assert len(forms) == 2 * p.N_ions == 6
    assert [f.name for f in forms] == ["Na_i", "K_i", "Cl_i", "Na_e", "K_e", "Cl_e"]
    assert [f.index for f in forms] == list(range(6))
    ev = forms[0].evaluator
    assert all(f.evaluator is ev for f in forms)              # one device pass serves all six
    assert ev.groups == ((int(p.membrane_data_tag),),)
    lo, hi = ev.box
    assert lo[0] == 0.0 and hi[0] == pytest.approx(0.5e-6) and np.all(np.isinf(lo[1:])) and np.all(np.isinf(hi[1:]))
    q = make_problem(ci_config(N=16, steps=1), "ci")          # no stimulus region: no mask
    assert create_flux_forms(q)[0].evaluator.box is None
    assert compute_fluxes([], None).shape == (0,)


def test_stimulus_box_of_several_directions():
    from cgx_hip.diagnostics import stimulus_box
    cfg = tissue_config(3, 12, 2, stimulus=True)
    cfg["stimulus_region"] = {"multiple": True, "direction": ["x", "z"], "range": [[0.0, 0.47], [0.1, 0.8]]}
    lo, hi = stimulus_box(_problem(cfg))
    assert np.allclose(lo, [0.0, -np.inf, 0.1e-6]) and np.allclose(hi, [0.47e-6, np.inf, 0.8e-6])
    assert stimulus_box(_problem(tissue_config(2, 18, 3, stimulus=False))) is None


def test_save_fluxes_defaults_to_off():
    from cgx_hip.solver import SolverKNPEMI
    cfg = ci_config(N=16, steps=1)
    p = _problem(cfg)
    assert SolverKNPEMI.save_fluxes is False
    assert SolverKNPEMI(p, solver_config=p.solver_config).save_fluxes is False
    cfg2 = copy.deepcopy(cfg)
    cfg2["solver"]["output"]["save_fluxes"] = True
    p2 = _problem(cfg2)
    assert SolverKNPEMI(p2, solver_config=p2.solver_config).save_fluxes is True


def test_facet_group_map_merges_tags_and_keeps_empty_groups():
    from cgx_hip.diagnostics import facet_areas, facet_group_map
    p = _problem(tissue_config(2, 18, 3, stimulus=False))
    tags = np.asarray(p.gamma_facet_tags)
    groups = [[3], [99], [2, 5], [3, 4]]                      # 99: no such facet; the second 3 is already taken by group 0
    seg_ptr, facets = facet_group_map(p, groups)
    assert seg_ptr.dtype == np.int32 and facets.dtype == np.int32
    assert list(np.diff(seg_ptr)) == [16, 0, 32, 16]
    assert set(tags[facets[seg_ptr[0]:seg_ptr[1]]]) == {3}
    assert set(tags[facets[seg_ptr[2]:seg_ptr[3]]]) == {2, 5}
    assert set(tags[facets[seg_ptr[3]:seg_ptr[4]]]) == {4}
    assert len(np.unique(facets)) == len(facets)
    area = facet_areas(p, seg_ptr, facets)
    side = 4.0 / 18.0 * 1e-6
    assert np.allclose(area, [4 * side, 0.0, 8 * side, 4 * side], rtol=1e-12)
    seg_ptr, facets = facet_group_map(p, [])
    assert list(seg_ptr) == [0] and facets.size == 0
