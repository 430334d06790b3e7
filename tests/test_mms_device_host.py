"""The device path of the manufactured-solution runs (``MMS_test: {..., device: true}``, cgx_hip/mms.py) without a device:

* the SymPy -> fem converter: every source term and every exact solution, evaluated through ``fem.evaluate_numpy`` at random points,
  times and unit normals, equals the ``lambdify`` value to 1e-14 of the term's magnitude (its largest value over the sample: the
  terms are products of sines and pass through zero, so a bound relative to each value would be a bound on nothing);
* the sixteen registered expressions against the host assembler ``MMSAssembler.rhs_vector`` on square 8 (81 vertices, 128 cells, 16
  membrane facets) and cube 4 (125 vertices, 384 cells, 48 facets), with random concentrations so that the alpha weights vary:
  dt times the sum of the forms of tests/linear_form_ref.py equals what the host adds, per side, vertex and field, to 1e-12 of the
  reference's own scale of the entry (both sides are fp64 NumPy on the same rules; 1e-12 is the project's figure for assembled
  vectors); the signs on the 'phi' rows are checked on their own;
* the compiled programs stay inside the limits of the bytecode, and the error integrands are the squared errors.
"""
import numpy as np
import pytest
import torch

import linear_form_ref as LR
from parity_utils import mms_config

from cgx_hip import _lib, fem, mms

SHAPES = {2: 8, 3: 4}


def _problem(dim, device=True):
    from CGx.KNPEMI.KNPEMIx_ionic_model import PassiveModel
    from CGx.KNPEMI.KNPEMIx_problem import ProblemKNPEMI
    cfg = mms_config(dim, SHAPES[dim])
    cfg["MMS_test"]["device"] = device
    p = ProblemKNPEMI(cfg)
    p.set_initial_conditions()
    p.init_ionic_models([PassiveModel(p)])
    p.setup_variational_form()
    return p


@pytest.fixture(scope="module")
def problems():
    out = {}
    for dim in SHAPES:
        p = _problem(dim)
        rng = np.random.default_rng(11 + dim)
        for r in range(2):
            for j in range(p.N_ions):
                p.wh[r][j].x.array[:] = torch.as_tensor(rng.uniform(0.5, 1.5, p.wh[r][j].x.array.numel()), device=p.wh[r][j].x.array.device)
        p.t.value = float(p.dt.value)
        out[dim] = p
    return out


def test_the_key_is_opt_in_and_the_shim_imports():
    from CGx.utils.setup_mms import ExactSolutionsKNPEMI
    assert ExactSolutionsKNPEMI is mms.ExactSolutionsKNPEMI
    p = _problem(2, device=False)
    assert p.MMS_test and not p.mms_device and not hasattr(p, "mms_source_terms")
    cfg = mms_config(2, 8)
    assert "device" not in cfg["MMS_test"]


@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_converter_matches_lambdify(problems, dim):
    p = problems[dim]
    rng = np.random.default_rng(5)
    n = 400
    x = rng.uniform(0.0, 1.0, (n, dim))
    nrm = rng.normal(size=(n, dim))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    env = {"x": [x[:, a] for a in range(dim)], "fields": {}, "normal": [nrm[:, a] for a in range(dim)]}
    names = [k for k in p.src_terms if not k.startswith("J_")]
    assert len(names) == 13
    saved = p.t.value
    try:
        for t in (0.0, 1.0e-5, 0.73):
            p.t.value = t
            for key, expr in [(k, p.src_terms[k]) for k in names] + [(k, v) for k, v in p.exact_sols.items()]:
                want = p.M.evaluate(expr, x, t, nrm)
                got = np.broadcast_to(np.asarray(fem.evaluate_numpy(mms.to_fem(expr, p), env), dtype=np.float64), want.shape)
                mag = np.max(np.abs(want))
                assert mag > 0 and np.max(np.abs(got - want)) <= 1e-14 * mag, (key, t, np.max(np.abs(got - want)) / mag)
    finally:
        p.t.value = saved


@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_programs_fit_the_bytecode(problems, dim):
    """every registered expression compiles under the roles of its kind, far below 48 registers, 64 constants and 8 aux slots"""
    from cgx_hip.functionals import compile_functional, compile_membrane_functional
    p = problems[dim]
    terms = p.mms_source_terms
    assert [t["kind"] for t in terms].count("volume") == 4 and [t["kind"] for t in terms].count("membrane") == 8
    assert sum(2 if t["kind"] == "volume" else 1 for t in terms) == 16
    for tm in terms:
        if tm["kind"] == "volume":
            specs = [sp.spec for sp in compile_functional(p, tm["expr_i"], tm["expr_e"], degree=mms.VOLUME_DEGREE).sides]
            assert len(specs) == 2
        else:
            specs = [compile_membrane_functional(p, tm["expr"], degree=mms.MEMBRANE_DEGREE).spec]
        for spec in specs:
            regs = 1 + max(max(r[1], r[2] if r[0] > 5 else 0) for r in spec.code.tolist())
            assert regs <= 24 and len(spec.const_sources) <= 24 and len(spec.aux_functions) <= dim, (tm["field"], regs)
            assert spec.code.shape[0] <= 200
            ops = {r[0] for r in spec.code.tolist()}
            assert ops & {_lib.FUNC_OPS["SIN"], _lib.FUNC_OPS["COS"]}
            assert any(c is p.t for c in spec.const_sources)                 # the time is the problem's Constant: read at every step


def _device_sum(p):
    """(dt x the sum of the registered forms [2, n_v, 4], the reference's scale of every entry)"""
    n_v = p.local_mesh.coords.shape[0]
    dt = float(p.dt.value)
    total, scale = np.zeros((2, n_v, 4)), np.zeros((2, n_v, 4))
    from cgx_hip.linear_forms import field_index
    for tm in p.mms_source_terms:
        f = field_index(tm["field"])
        if tm["kind"] == "volume":
            v, s, _ = LR.volume_form(p, tm["expr_i"], tm["expr_e"], degree=mms.VOLUME_DEGREE)
            total[:, :, f] += dt * v[:, 0, :]
            scale[:, :, f] += dt * s[:, 0, :]
        else:
            v, s, _ = LR.membrane_form(p, tm["expr"], degree=mms.MEMBRANE_DEGREE)
            side = 0 if tm["side"] == "i" else 1
            total[side, :, f] += dt * v[0]
            scale[side, :, f] += dt * s[0]
    return total, scale


@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_registered_expressions_match_the_host_assembler(problems, dim):
    p = problems[dim]
    n_v = p.local_mesh.coords.shape[0]
    assert (n_v, p.local_mesh.cells.shape[0], p._fv.shape[0]) == {2: (81, 128, 16), 3: (125, 384, 48)}[dim]
    want = mms.MMSAssembler(p).rhs_vector(np.arange(n_v), n_v + np.arange(n_v), 8 * n_v).reshape(2, n_v, 4)
    got, scale = _device_sum(p)
    assert np.all(got[scale == 0] == 0) and np.all(want[scale == 0] == 0)
    on = scale > 0
    err = np.abs(got - want)[on] / scale[on]
    print(f"MMS forms vs host assembler dim={dim}: largest error / scale {err.max():.2e}")
    assert err.max() <= 1e-12
    for s in range(2):
        for f in range(4):
            assert np.max(np.abs(want[s, :, f])) > 0, (s, f)                     # every block of both sides is exercised


@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_phi_signs(problems, dim):
    """'phi' volume sources are MINUS f_phi (the reference's form carries the sign, the hook adds); ('phi', 'i') is +f_phi_m and
    ('phi', 'e') is -(f_phi_m + f_gamma); the extracellular ion terms carry the minus of KNPEMIx_problem.py:623"""
    p = problems[dim]
    rng = np.random.default_rng(9)
    x = rng.uniform(0.0, 1.0, (64, dim))
    nrm = rng.normal(size=(64, dim))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    t = float(p.t.value)
    env = {"x": [x[:, a] for a in range(dim)], "fields": {}, "normal": [nrm[:, a] for a in range(dim)]}
    ev = lambda e: np.asarray(fem.evaluate_numpy(e, env), dtype=np.float64)
    ex = lambda key: p.M.evaluate(p.src_terms[key], x, t, nrm)
    by = {(tm["kind"], tm["field"], tm.get("side")): tm for tm in p.mms_source_terms}
    vol = by[("volume", "phi", None)]
    for got, want in ((ev(vol["expr_i"]), -ex("f_phi_i")), (ev(vol["expr_e"]), -ex("f_phi_e")),
                      (ev(by[("membrane", "phi", "i")]["expr"]), ex("f_phi_m")),
                      (ev(by[("membrane", "phi", "e")]["expr"]), -(ex("f_phi_m") + ex("f_gamma")))):
        mag = np.max(np.abs(want))
        assert mag > 1e-3 and np.max(np.abs(got - want)) <= 1e-13 * mag          # the wrong sign would be off by 2 mag
    # the ion rows: constant fields make alpha a number, so the expression is a multiple of the analytic term
    env["fields"] = {id(p.wh[r][j]): np.full(64, 1.0 + 0.5 * j + 0.25 * r) for r in range(2) for j in range(p.N_ions)}
    for j, ion in enumerate(p.ion_list):
        z = float(ion["z"].value)
        al = [(1.0 + 0.5 * j + 0.25 * r) / sum(1.0 + 0.5 * k + 0.25 * r for k in range(p.N_ions)) for r in range(2)]
        gi, ge = ev(by[("membrane", ion["name"], "i")]["expr"]), ev(by[("membrane", ion["name"], "e")]["expr"])
        wi, we = al[0] / z * ex(f"f_phi_{ion['name']}"), -al[1] / z * (ex(f"f_phi_{ion['name']}") + ex("f_gamma"))
        assert np.max(np.abs(gi - wi)) <= 1e-13 * np.max(np.abs(wi)) and np.max(np.abs(ge - we)) <= 1e-13 * np.max(np.abs(we))
        vi = by[("volume", ion["name"], None)]
        assert np.max(np.abs(ev(vi["expr_i"]) - ex(f"f_{ion['name']}_i"))) <= 1e-13 * np.max(np.abs(ex(f"f_{ion['name']}_i")))


@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_error_integrands_are_the_squared_errors(problems, dim):
    p = problems[dim]
    (ci, ce), (pi_, pe) = mms.error_integrands(p)
    assert len(ci) == len(ce) == 3
    rng = np.random.default_rng(2)
    x = rng.uniform(0.0, 1.0, (50, dim))
    t = float(p.t.value)
    names = [ion["name"] for ion in p.ion_list] + ["phi"]
    vals = {id(p.wh[r][k]): rng.uniform(0.0, 2.0, 50) for r in range(2) for k in range(4)}
    env = {"x": [x[:, a] for a in range(dim)], "fields": vals}
    for r, exprs in enumerate((list(ci) + [pi_], list(ce) + [pe])):
        for k, e in enumerate(exprs):
            want = (vals[id(p.wh[r][k])] - p.M.evaluate(p.exact_sols[f"{names[k]}_{'ie'[r]}"], x, t)) ** 2
            assert np.allclose(fem.evaluate_numpy(e, env), want, rtol=1e-13, atol=1e-15)
