"""The manufactured-solution run with its sources and error norms on the device (``MMS_test: {..., device: true}``, cgx_hip/mms.py):

1. source form vectors: on square 8 and cube 4, at t = dt with random concentrations, the form vector of every registered source
   against tests/linear_form_ref.py under ``functionals_irregular.tolerance(floor)`` (the rule of test_gpu_linear_form.py), and their
   dt-weighted sum against ``MMSAssembler.rhs_vector`` at 1e-12 of each field block's largest entry.  The form vectors are compared,
   not the difference of two right-hand sides: the sources are dt ~ 1e-5 of b, and the subtraction would cost five digits;
2. error norms: on the state after one step, ``p.errors`` from the two functionals agrees with ``MMSAssembler.l2_errors()`` to 1e-10
   relative.  Both use the same 5-point-per-axis rule; the pointwise difference u_h - u is >= 1e-3 on these meshes and the two
   evaluations of u differ by a few ulp of values <= 2, which gives ~1e-12: the bound leaves a factor 100 over that;
3. end-to-end parity of (dim, N) = (2, 8) and (3, 8) with the tolerances of test_gpu_mms.py: against the oracle's run (1e-6
   concentrations, 1e-5 potentials), the reference's record (2e-5 potentials, 5e-3 concentrations) and the same run with
   ``device: false`` (the oracle's tolerances); every solve converges;
4. the user's example: ``p.add_source('K', expr_e=A sin(omega t) cos(k x), tags=[...])`` on a CI problem, its form vector at two
   times (the Constant is re-read) and bit-identical repeats.

Measured on MI355X: form vectors at most 1.3e-15 (volume) and 6.6e-16 (membrane) of the scale, their sum 8.4e-16 of a block's largest
entry; error norms 9.8e-16 relative to the host's; end to end against the oracle at most 1.8e-10 (concentrations) and 1.2e-07
(potentials), against the host path 6.3e-11 and 1.7e-08; the user's source 1.1e-15 of the scale.
"""
import numpy as np
import pytest
import torch

import functionals_irregular as FI
import linear_form_ref as LR
from parity_utils import ci_config, make_problem, mms_config

from cgx_hip import fem, mms

pytestmark = pytest.mark.gpu


def _problem(dim, N, device=True):
    from CGx.KNPEMI.KNPEMIx_ionic_model import PassiveModel
    from CGx.KNPEMI.KNPEMIx_problem import ProblemKNPEMI
    cfg = mms_config(dim, N)
    cfg["MMS_test"]["device"] = device
    p = ProblemKNPEMI(cfg)
    p.set_initial_conditions()
    p.init_ionic_models([PassiveModel(p)])
    p.setup_variational_form()
    return p


# ------------------------------------------------------------------------------------------ 1. the sources' form vectors
@pytest.mark.parametrize("dim,N", [(2, 8), (3, 4)])
def test_source_form_vectors(dim, N):
    from cgx_hip.linear_forms import MembraneLinearForm, VolumeLinearForm, field_index
    p = _problem(dim, N)
    rng = np.random.default_rng(11 + dim)
    for r in range(2):
        for j in range(p.N_ions):
            a = p.wh[r][j].x.array
            a[:] = torch.as_tensor(rng.uniform(0.5, 1.5, a.numel()), device=a.device)
    dt = float(p.dt.value)
    p.t.value = dt
    p.create_backend()
    assert len(p.mms_sources) == len(p.mms_source_terms) == 12 and p._sources == p.mms_sources
    n_v = p.local_mesh.coords.shape[0]
    total = np.zeros((2, n_v, 4))
    for h, tm in zip(p.mms_sources, p.mms_source_terms):
        f = field_index(tm["field"])
        assert h.field == f
        got = h.form().cpu().numpy()
        if tm["kind"] == "volume":
            assert isinstance(h.form, VolumeLinearForm) and h.sides == (0, 1) and h.form.degree == 9
            ref = lambda ld: LR.volume_form(p, tm["expr_i"], tm["expr_e"], degree=mms.VOLUME_DEGREE, longdouble=ld)
            total[:, :, f] += dt * got[:, 0, :]
        else:
            assert isinstance(h.form, MembraneLinearForm) and h.sides == ((0,) if tm["side"] == "i" else (1,)) and h.form.degree == 10
            ref = lambda ld: LR.membrane_form(p, tm["expr"], degree=mms.MEMBRANE_DEGREE, longdouble=ld)
            total[0 if tm["side"] == "i" else 1, :, f] += dt * got[0]
        want, scale, _ = ref(False)
        tol = FI.tolerance(LR.floor(ref))
        err = np.abs(got - want)
        pos = scale > 0
        print(f"ERR form dim={dim} {tm['kind']} {tm['field']} {tm.get('side', 'i+e')}: max |device - host| / scale = "
              f"{np.max(err[pos] / scale[pos]):.2e} (tol {tol:.1e})")
        assert np.isfinite(got).all() and np.all(err <= tol * scale)
    want = mms.MMSAssembler(p).rhs_vector(np.arange(n_v), n_v + np.arange(n_v), 8 * n_v).reshape(2, n_v, 4)
    for f in range(4):
        big = np.max(np.abs(want[:, :, f]))
        err = np.max(np.abs(total[:, :, f] - want[:, :, f])) / big
        print(f"ERR sum of forms vs host assembler dim={dim} field {f}: {err:.2e} of the block's largest entry {big:.3e}")
        assert big > 0 and err <= 1e-12


# ------------------------------------------------------------------------------------------ 2., 3. runs
_RUNS = {}


def _run(dim, N, device):
    if (dim, N, device) not in _RUNS:
        from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
        p = _problem(dim, N, device)
        p.solver_config["view_ksp"] = False
        s = SolverKNPEMI(p, solver_config=p.solver_config)
        s.solve()
        _RUNS[(dim, N, device)] = (np.array(p.errors), list(s.reasons), p, s)
    return _RUNS[(dim, N, device)]


@pytest.mark.parametrize("dim,N", [(2, 8), (3, 8)])
def test_error_norms_from_the_functionals(dim, N):
    e, reasons, p, _ = _run(dim, N, True)
    assert hasattr(p, "_mms_errors") and not hasattr(p, "_mms_asm")          # no host assembler in a device run
    host = np.array(mms.MMSAssembler(p).l2_errors())
    rel = np.abs(e - host) / host
    print(f"ERR l2 errors dim={dim} N={N}: device vs host relative " + " ".join(f"{v:.2e}" for v in rel))
    assert np.all(host > 1e-5) and rel.max() <= 1e-10


@pytest.mark.parametrize("dim,N,level", [(2, 8, 0), (3, 8, 0)])
def test_end_to_end_parity(dim, N, level):
    import mms_oracle as M
    e, reasons, p, s = _run(dim, N, True)
    eh, reasons_h, ph, _ = _run(dim, N, False)
    assert all(r > 0 for r in reasons) and all(r > 0 for r in reasons_h), (reasons, reasons_h)
    assert p.mms_device and len(p._sources) == 12 and not ph.mms_device and not getattr(ph, "_sources", None)
    eo = M.run_mms(dim, N)
    print(f"ERR end to end dim={dim} N={N}: device vs oracle " + " ".join(f"{v:.1e}" for v in np.abs(e - eo) / eo)
          + " | device vs host path " + " ".join(f"{v:.1e}" for v in np.abs(e - eh) / eh))
    assert np.allclose(e[:6], eo[:6], rtol=1e-6) and np.allclose(e[6:], eo[6:], rtol=1e-5), (e, eo)
    rec = (M.RECORDED_2D if dim == 2 else M.RECORDED_3D)[level]
    assert np.allclose(e[6:], rec[6:], rtol=2e-5) and np.allclose(e[:6], rec[:6], rtol=5e-3), (e, rec)
    assert np.allclose(e[:6], eh[:6], rtol=1e-6) and np.allclose(e[6:], eh[6:], rtol=1e-5), (e, eh)


# ------------------------------------------------------------------------------------------ 4. the user's example
def test_sinusoidal_user_source():
    p = make_problem(ci_config(N=8, steps=1))
    x = fem.SpatialCoordinate(p.mesh)
    A, omega, k = 3.0e-2, 2.0 * fem.pi * 50.0, 4.0e6
    expr = A * fem.sin(omega * p.t) * fem.cos(k * x[0])
    tags = [int(t) for t in np.ravel(p.extra_tag)]
    h = p.add_source("K", expr_e=expr, tags=tags)
    seen = []
    for time in (3.0e-3, 7.5e-3):
        p.t.value = time
        got = h.form().cpu().numpy()
        again = h.form().cpu().numpy()
        assert np.array_equal(got.view(np.int64), again.view(np.int64))          # identical bits
        ref = lambda ld: LR.volume_form(p, None, expr, tags=tags, degree=2, longdouble=ld)
        want, scale, on = ref(False)
        tol = FI.tolerance(LR.floor(ref))
        err = np.abs(got - want)
        print(f"ERR user source t={time}: max |device - host| / scale = {np.max(err[scale > 0] / scale[scale > 0]):.2e} (tol {tol:.1e})")
        assert np.all(err <= tol * scale) and np.all(got[0] == 0.0) and np.max(np.abs(got[1])) > 0
        seen.append(got)
    # the second call shows the new time: sin(omega t) went from sin(0.3 pi) to sin(0.75 pi) and the vector scales with it.  Both
    # vectors are within tol * scale of their references; on the entries above 1e-3 of the largest one that is below 1e-6 relative
    ratio = np.sin(omega * 7.5e-3) / np.sin(omega * 3.0e-3)
    on = np.abs(seen[0][1, 0]) > 1e-3 * np.max(np.abs(seen[0][1, 0]))
    assert abs(ratio - 1.0) > 0.1 and on.sum() > 10
    assert np.allclose(seen[1][1, 0][on], ratio * seen[0][1, 0][on], rtol=1e-6, atol=0.0)
    h.remove()
