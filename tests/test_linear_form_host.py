"""The inputs of tests/test_gpu_linear_form.py, pinned without a GPU: the NumPy restatement of the linear forms
(tests/linear_form_ref.py) meets closed forms, every case the GPU test runs has a rounding floor <= 1e-10 (the table of DESIGN.md
section 14), the step hooks refuse what they must before they need a device, and the new entry points are declared and loadable."""
import math
import os
import re
import types

import numpy as np
import pytest

import functional_ref
import functionals_irregular as FI
import linear_form_ref as LR
import membrane_functional_ref as mref
from functional_ref import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["knp_functional_eval_load", "knp_membrane_functional_eval_load", "knp_scatter_create", "knp_scatter_apply",
               "knp_scatter_get_info", "knp_scatter_destroy", "knp_rhs_add_load"]


@pytest.fixture(scope="module")
def probs(tmp_path_factory):
    cache = {}
    tmp = tmp_path_factory.mktemp("linear_form_host")

    def get(name):
        if name not in cache:
            cache[name] = FI.Prob(tmp, name)
        return cache[name]
    return get


# ---------------------------------------------------------------------------------------------- closed forms of the restatement
@pytest.mark.parametrize("name", ["delaunay2d_12_cw", "delaunay3d_5", FI.TWO_TAG])
def test_the_constant_one_gives_a_share_of_every_measure(probs, name):
    P = probs(name)
    p, d = P.p, P.dim
    lm = p.local_mesh
    nco = int(lm.n_cells_owned)
    cells = np.asarray(lm.cells)[:nco]
    vec, scale, on = LR.volume_form(p, 1.0, 1.0, degree=1)
    vol = functional_ref.cell_volumes(lm.coords[cells])
    intra = np.isin(np.asarray(lm.cell_tags[:nco]), [int(t) for t in p.intra_tags])
    for s, sel in enumerate((intra, ~intra)):
        want = np.zeros(lm.coords.shape[0])
        np.add.at(want, cells[sel].ravel(), np.repeat(vol[sel] / (d + 1), d + 1))
        assert np.all(np.abs(vec[s, 0] - want) <= TOL * want) and np.array_equal(on[s], want > 0) and np.all(vec[s, 0][~on[s]] == 0.0)
    mvec, _, mon = LR.membrane_form(p, 1.0, degree=1)
    fv, meas = np.asarray(p._fv), np.asarray(p._fmeas)
    want = np.zeros(lm.coords.shape[0])
    np.add.at(want, fv.ravel(), np.repeat(meas / d, d))
    assert np.all(np.abs(mvec[0] - want) <= TOL * want) and np.array_equal(mon, want > 0) and mon.any() and not mon.all()


@pytest.mark.parametrize("name", ["delaunay2d_12_cw", "delaunay3d_5"])
def test_a_p1_function_at_degree_two_gives_the_mass_matrix_times_it(probs, name):
    P = probs(name)
    p = P.p
    lm = p.local_mesh
    nco, n_v = int(lm.n_cells_owned), lm.coords.shape[0]
    cells = np.asarray(lm.cells)[:nco]
    intra = np.isin(np.asarray(lm.cell_tags[:nco]), [int(t) for t in p.intra_tags])
    vec, scale, on = LR.volume_form(p, P.user, P.user, degree=2)
    f = P.user.numpy()
    rng = np.random.default_rng(5)
    tests = [np.eye(n_v)[v] for v in rng.permutation(n_v)[:12]] + [rng.uniform(-1.0, 1.0, n_v)]
    for s, sel in enumerate((intra, ~intra)):
        for v in tests:
            want, sc = functional_ref.mass_form(lm.coords, cells[sel], f, v)
            assert abs(float(vec[s, 0] @ v) - want) <= TOL * sc


@pytest.mark.parametrize("name", ["hub2d_12_48m_cw", FI.TWO_TAG])
def test_the_vector_sums_to_the_functional(probs, name):
    P = probs(name)
    p = P.p
    fi, fe, deg = LR.volume_case(P, "nonlinear")
    vec, scale, _ = LR.volume_form(p, fi, fe, degree=deg)
    tags, side, val, sc = functional_ref.reference(p, fi, fe, degree=deg)
    for s in range(2):
        for j in range(3):
            assert abs(math.fsum(vec[s, j]) - math.fsum(val[side == s, j])) <= TOL * sc[side == s, j].sum()
            assert abs(scale[s, j].sum() - sc[side == s, j].sum()) <= 1e-9 * sc[side == s, j].sum()      # sum_a lambda_a = 1
    outs, tg, mdeg = LR.membrane_case(P, "random_plus")
    mvec, mscale, _ = LR.membrane_form(p, outs, tg, degree=mdeg)
    _, mval, msc = mref.reference(p, outs, tags=tg, degree=mdeg)
    for j in range(3):
        assert abs(math.fsum(mvec[j]) - math.fsum(mval[:, j])) <= TOL * msc[:, j].sum()
    # some tags only, one side only: the other side and the vertices away from the listed cells stay 0
    part, _, on = LR.volume_form(p, fi, None, tags=[int(p.intra_tags[0])], degree=deg)
    assert np.all(part[1] == 0.0) and not on[1].any() and np.all(part[0][:, ~on[0]] == 0.0) and on[0].any()


def test_the_entries_of_a_vertex_ascend_in_the_item():
    iv = np.array([[4, 1, 2], [2, 1, 0], [1, 3, 2]])
    ptr, flat = LR.entries(6, iv)
    assert ptr.tolist() == [0, 1, 4, 7, 8, 9, 9]
    assert flat.tolist() == [5, 1, 4, 6, 2, 3, 8, 7, 0]      # i nv + a; vertex 5 has none
    vals = np.arange(18.0).reshape(3, 3, 2)
    out, _ = LR.gather(6, iv, vals)
    assert out[:, 1].tolist() == [2.0 + 8.0 + 12.0, 3.0 + 9.0 + 13.0] and np.all(out[:, 5] == 0.0)


# ---------------------------------------------------------------------------------------------- the tolerance of every GPU case
def test_floor_table(probs):
    for name in FI.VOLUME_MESHES:
        for case in FI.VOLUME_CASES:
            LR.volume_floor(probs(name), case)
    for name in FI.MEMBRANE_MESHES:
        for case in FI.MEMBRANE_CASES:
            LR.membrane_floor(probs(name), case)
    table = LR.floor_table()
    print("\n".join(table))
    assert len(table) == len(FI.VOLUME_MESHES) * len(FI.VOLUME_CASES) + len(FI.MEMBRANE_MESHES) * len(FI.MEMBRANE_CASES)
    for f in LR._FLOORS.values():
        assert np.isfinite(f) and f <= FI.BOUND and FI.tolerance(f) <= FI.BOUND


def test_the_nodal_source_and_its_form_agree_on_the_host():
    src, plain = LR.step_problems()
    assert len(src.injection_cells) > 0
    f = src.ion_list[1]["f_e"].numpy()
    nodal, form, scale = LR.nodal_and_form(plain, f)
    on = scale > 0
    floor = float(np.max(np.abs(nodal - form)[on] / scale[on]))
    print(f"nodal dt M f against the degree-2 form: floor {floor:.2e} over {int(on.sum())} vertices")
    assert on.any() and floor <= FI.BOUND and np.all(form[~on] == 0.0)


# ---------------------------------------------------------------------------------------------- refusals that need no device
def test_the_step_hooks_refuse_before_they_need_a_device():
    from parity_utils import ci_config, make_problem
    from cgx_hip import fem
    cfg = ci_config(N=8, steps=1)
    cfg["quiet"] = True
    p = make_problem(cfg, "ci")
    one = fem.Constant(p.mesh, 1.0)
    for bad in ("Ca", "k", 4, -1, None, 1.5):
        with pytest.raises(ValueError, match="unknown field"):
            p.add_source(bad, expr_e=one)
        with pytest.raises(ValueError, match="unknown field"):
            p.add_membrane_source(bad, "i", one)
    with pytest.raises(ValueError, match="other side"):
        p.add_source("K", expr_e=p.wh[0][1])
    with pytest.raises(ValueError, match="other side"):
        p.add_source("phi", expr_i=one * p.wh[1][3])
    with pytest.raises(ValueError, match="one expression per side"):
        p.add_source("K", expr_e=[one, one])
    with pytest.raises(ValueError, match="one expression per side"):
        p.add_membrane_source("phi", "i", [one, one])
    with pytest.raises(ValueError, match="unknown side"):
        p.add_membrane_source("phi", "x", one)
    with pytest.raises(ValueError):
        p.add_source("K")                                  # no expression at all: the functionals' refusal
    with pytest.raises(ValueError):
        p.add_source("K", expr_e=one, tags=[99])           # an unknown tag: likewise
    comm = p.comm
    p.comm = types.SimpleNamespace(size=2, rank=0)
    try:
        with pytest.raises(NotImplementedError, match="run on one rank"):
            p.add_source("K", expr_e=one)
        with pytest.raises(NotImplementedError, match="run on one rank"):
            p.add_membrane_source("phi", "e", one)
    finally:
        p.comm = comm
    assert not getattr(p, "_sources", [])                  # nothing was registered on the way


# ---------------------------------------------------------------------------------------------- header and loader
def test_the_new_entry_points_are_declared_and_loadable():
    import __graft_entry__ as g
    g.build()
    from cgx_hip import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "knpemi_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(knp_[a-z0-9_]+)\s*\(", txt))
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert n in declared, n
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert _lib.SIGNATURES["knp_rhs_add_load"][1][3] is __import__("ctypes").c_double
    assert lib.knp_rhs_add_load(None, 0, 0, 1.0, None, None) < 0 and lib.knp_scatter_get_info(None, 0, None, 0) < 0
