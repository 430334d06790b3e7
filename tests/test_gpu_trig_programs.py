"""KNP_OP_SIN / COS / TANH on every GPU engine that executes the membrane bytecode, with the suite of tests/trig_program_ref.py against
its long-double host reference (``fem.interpret_program``, assembled by the oracle), as test_gpu_membrane_programs.py does for the
base opcodes and with that file's shapes and tolerances:

1. the ahead-of-time interpreter in the right-hand-side facet kernel (``KNP_JIT=0``; the FUNCS instantiation of ``k_gamma_facets``):
   every program as a single-program table and the mixed table;
2. the run-time compiled kernels ``knp_gamma_vec_2d``, ``knp_gamma_vec_3d_q1``, ``knp_gamma_vec_3d_many`` (``KNP_GAMMA_QV=9``) and, in
   a child process, ``knp_gamma_vec_3d`` (``KNP_GAMMA_MANY=0``): constant-only SIN / COS / TANH are hoisted there;
3. new constants (the time of sin(omega t)) without new programs, on the interpreter and on the compiled code;
4. the diagnostic interpreter ``k_diag_facets`` through ``membrane_integral``;
5. one volume and one membrane functional (``k_functional`` / ``k_membrane_functional``) with ``fem.sin`` / ``cos`` / ``tanh``
   integrands, against tests/functional_ref.py and tests/membrane_functional_ref.py under the tolerance rule of the functionals;
6. one state program with ``sin``, ``cos`` and ``tanh`` through ``k_state_update``, against tests/state_program_ref.py (long double).

Tolerances: 1e-12 of the block's largest mechanism term against the long-double reference, 1e-13 between engines; shapes: square 11
(20 facets, 242 cells, partial last blocks) and cube 7 (108 facets).  A program without these opcodes launches the kernels it
launched before; test_gpu_membrane_programs.py keeps checking those.

Largest errors measured on MI355X, in these units (2D / 3D): interpreter 6.2e-16 / 6.0e-16; run-time compiled 6.2e-16 / 5.2e-16 (3D:
each of the three kernels, the 16-lane one 4.6e-16); run-time compiled against interpreter 1.9e-16 / 4.1e-16; after new constants
4.3e-16 / 3.5e-16 on both engines; diagnostic integral 4.1e-16 / 2.2e-16; volume functional 3.0e-15 / 2.5e-15 and membrane functional
6.5e-16 / 2.2e-16 of the scale (tolerance 1e-12); state program 2.6e-16 of max |y|.  ROCm's fp64 sin / cos / tanh, the large
arguments included, stay three orders of magnitude inside the 1e-12 on every engine.
"""
from __future__ import annotations

import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import functional_ref
import functionals_irregular as FI
import membrane_functional_ref as mref
import membrane_program_ref as R
import state_program_ref as SR
import trig_program_ref as T
from parity_utils import ci_config, make_oracle, make_problem

from cgx_hip import fem
from cgx_hip.ionic_models import IonicModel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, TOL_ENGINES = 1e-12, 1e-13
ENGINES = {"interp": {"KNP_JIT": "0"}, "jit": {"KNP_JIT": "1"}, "jit_qv9": {"KNP_JIT": "1", "KNP_GAMMA_QV": "9"}}
NAMES = list(T.NAMES)
JIT_TABLES = ["mixed", "uniform", "large"]      # every program runs in the mixed table; the singles are the ones with hoisted functions


@contextlib.contextmanager
def _environ(values):
    keys = ("KNP_JIT", "KNP_GAMMA_QV")
    saved = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(values)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


_ORACLES, _REFS = {}, {}


def oracle(dim):
    if dim not in _ORACLES:
        kind, N = R.MESHES[dim]
        _ORACLES[dim] = R.fill_fields(make_oracle(N, kind))
    return _ORACLES[dim]


def reference(dim, name, variant=0):
    """(b, mechanism term of b, currents at the quadrature points) of a table; computed once, never changed"""
    key = (dim, name, variant)
    if key not in _REFS:
        o = oracle(dim)
        Iq = R.currents(o, T.tables(dim, variant)[name])
        b, mech, _ = R.rhs_reference(o, Iq)
        for a in (b, mech, Iq):
            a.setflags(write=False)
        _REFS[key] = (b, mech, Iq)
    return _REFS[key]


class Rig:
    """One native context on the mesh of ``dim``: the CI problem with the suite's fields, the membrane tag of a facet = its program id
    in the table of all programs.  ``mixed``: tag k runs program k; otherwise every tag runs program 0, which ``rhs`` replaces."""

    def __init__(self, dim, mixed):
        kind, N = R.MESHES[dim]
        self.dim, self.mixed = dim, mixed
        o = oracle(dim)
        p = make_problem(ci_config(N=N, steps=1, kind=kind))
        R.copy_fields_to_problem(o, p)
        K = len(NAMES)
        tags = R.facet_programs(p._fv, K)
        p.gamma_tags = tuple(range(K))
        p.local_mesh.gamma_tags = tags
        p.gamma_facet_tags = tags
        p.tag_program = {k: (k if mixed else 0) for k in range(K)}
        p.programs = self._specs("mixed" if mixed else NAMES[0], 0)
        self.p, self.be = p, p.create_backend()
        self.results = {}

    def _specs(self, name, variant):
        assert (name == "mixed") == self.mixed
        return {i: R.spec_of(e) for i, e in enumerate(T.tables(self.dim, variant)[name])}

    def status(self):
        return self.be.lib.knp_jit_status(self.be.ctx).decode()

    def assemble(self):
        self.be.assemble_matrix()
        self.be.assemble_rhs()
        return self.be.b.cpu().numpy().copy()

    def rhs(self, engine, name, variant=0, fresh=False):
        key = (engine, name, variant)
        if fresh or key not in self.results:
            with _environ(ENGINES[engine]):
                self.p.programs = self._specs(name, variant)
                self.be.upload_programs()
                b = self.assemble()
                self.results[key] = (b, self.status())
        return self.results[key]


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(dim, mixed):
        if (dim, mixed) not in made:
            made[(dim, mixed)] = Rig(dim, mixed)
        return made[(dim, mixed)]
    return get


def _check_status(engine, status):
    if engine == "interp":
        assert "KNP_JIT=0" in status, status
    else:
        assert status == "native", status          # a compile failure silently falls back to the interpreter


def _compare(label, b, dim, name, variant=0, tol=TOL):
    b_ref, mech, _ = reference(dim, name, variant)
    err = R.block_errors(b, b_ref, mech)
    print(f"ERR {label} dim={dim} table={name} variant={variant} " + " ".join(f"{e:.2e}" for e in err))
    assert np.isfinite(b).all() and max(err) <= tol, (label, name, err)


@pytest.mark.parametrize("name", NAMES + ["mixed"])
@pytest.mark.parametrize("dim", [2, 3])
def test_interpreter_matches_reference(rigs, dim, name):
    b, status = rigs(dim, name == "mixed").rhs("interp", name)
    _check_status("interp", status)
    _compare("interp", b, dim, name)


@pytest.mark.parametrize("name", JIT_TABLES)
@pytest.mark.parametrize("dim,engine", [(2, "jit"), (3, "jit"), (3, "jit_qv9")])
def test_runtime_compiled_code_matches_reference_and_interpreter(rigs, dim, engine, name):
    rig = rigs(dim, name == "mixed")
    (b, status), (b_int, st_int) = rig.rhs(engine, name), rig.rhs("interp", name)
    _check_status(engine, status)
    _check_status("interp", st_int)
    _compare(engine, b, dim, name)
    err = R.block_errors(b, b_int, reference(dim, name)[1])
    print(f"ERR {engine}-vs-interp dim={dim} table={name} " + " ".join(f"{e:.2e}" for e in err))
    assert max(err) <= TOL_ENGINES, err


CHILD = """
import sys; sys.path[:0] = ['tests', 'oracle', 'knp-emi-cgx_amd']; import conftest, json, numpy as np
import test_gpu_trig_programs as G
path = sys.argv[1]
b, status = G.Rig(3, True).rhs('jit', 'mixed')
np.savez(path, mixed=b)
print('RESULT' + json.dumps(status))
"""


def test_runtime_compiled_16_lane_kernel(tmp_path, rigs):
    """KNP_GAMMA_MANY=0 keeps the 16 lanes x 3 points kernel knp_gamma_vec_3d; the switch is read once per process: a fresh child"""
    path = str(tmp_path / "many0.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("KNP_JIT", "KNP_GAMMA_QV")}
    out = subprocess.run([sys.executable, "-c", CHILD, path], cwd=ROOT, env=dict(env, KNP_GAMMA_MANY="0"), capture_output=True, text=True,
                         timeout=300)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
    assert out.returncode == 0 and line, f"exit status {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    _check_status("jit", json.loads(line[0][6:]))
    b = np.load(path)["mixed"]
    _compare("jit_many0", b, 3, "mixed")
    b_int, _ = rigs(3, True).rhs("interp", "mixed")
    err = R.block_errors(b, b_int, reference(3, "mixed")[1])
    print("ERR jit_many0-vs-interp dim=3 table=mixed " + " ".join(f"{e:.2e}" for e in err))
    assert max(err) <= TOL_ENGINES, err


@pytest.mark.parametrize("engine", ["interp", "jit"])
@pytest.mark.parametrize("dim", [2, 3])
def test_new_constants_are_followed_without_new_programs(rigs, dim, engine):
    """knp_set_program_constants after a first assembly -- among them the time of the hoisted sin(omega t): the next right-hand side
    follows it, and the native code stays in place"""
    rig = rigs(dim, True)
    b0, status = rig.rhs(engine, "mixed", fresh=True)
    _check_status(engine, status)
    _compare(engine + " before", b0, dim, "mixed", 0)
    with _environ(ENGINES[engine]):
        rig.p.programs = rig._specs("mixed", 1)
        rig.be.refresh_program_constants()                 # knp_set_program_constants only: no knp_set_program
        b1 = rig.assemble()
        _check_status(engine, rig.status())
    mech0, mech1 = reference(dim, "mixed", 0)[1], reference(dim, "mixed", 1)[1]
    assert min(R.block_errors(mech1, mech0, mech0)) > 1e-3            # the two sets of constants do differ in every block
    _compare(engine + " after", b1, dim, "mixed", 1)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dim", [2, 3])
def test_diagnostic_interpreter_matches_reference(rigs, dim, name):
    """k_diag_facets (its FUNCS instantiation): constants as kernel arguments, code from global memory, one point at a time"""
    rig, o = rigs(dim, False), oracle(dim)
    be = rig.be
    tags = R.facet_programs(o.fv, len(NAMES))
    group = np.where(np.isin(tags, T.GROUPS[0]), 0, 1)
    be.set_facet_groups([list(g) for g in T.GROUPS])
    out = torch.zeros(2, dtype=torch.float64, device=be.device)
    for variant in (0, 1):
        spec = R.spec_of(T.tables(dim, variant)[name][0])
        if variant == 0:
            be.set_diag_program(spec)
        else:
            be.refresh_diag_constants(spec)
        got = be.membrane_integral(out).cpu().numpy().copy()
        want, mag = R.integral_reference(o, reference(dim, name, variant)[2], group, 2)
        err = np.abs(got - want) / mag
        print(f"ERR diag dim={dim} table={name} variant={variant} " + " ".join(f"{e:.2e}" for e in err))
        assert np.isfinite(got).all() and err.max() <= TOL, (variant, got, want)
    w0 = R.integral_reference(o, reference(dim, name, 0)[2], group, 2)[0]
    assert np.all(np.abs(want - w0) > 1e-3 * np.abs(w0))                # the constants did change the answer


# ------------------------------------------------------------------------------------------ functionals
def _integrands(p):
    """three outputs per kind: a standing wave times a sinusoidal stimulus, a smooth tanh switch of a solution field, and large
    arguments straight from Constants"""
    x = fem.SpatialCoordinate(p.mesh)
    u = [1.0e6 * c for c in x]
    t, big = fem.Constant(p.mesh, 0.0137), fem.Constant(p.mesh, T.LARGE[4])
    wave = fem.sin(300.0 * t) * fem.cos(4.0 * u[0]) * fem.sin(3.0 * u[-1])
    vol_i = [2.0 + wave, fem.tanh(0.05 * (p.wh[0][1] - 100.0)) + fem.cos(u[1]), fem.sin(big) + fem.cos(fem.Constant(p.mesh, T.LARGE[1])) * u[0]]
    vol_e = [2.0 - wave, fem.tanh(0.3 * (p.wh[1][1] - 4.0)) + fem.cos(u[1]), fem.cos(big) + fem.sin(fem.Constant(p.mesh, T.LARGE[3])) * u[0]]
    n = fem.FacetNormal(p.mesh)
    mem = [2.0 + wave * n[0]("+"), fem.tanh(-80.0 * p.phi_m_prev - 5.0) + fem.sin(0.05 * p.wh[0][1]) * fem.cos(0.3 * p.wh[1][1]),
           fem.sin(big) * n[1]("-") + fem.tanh(20.0 + 30.0 * u[0])]
    return vol_i, vol_e, mem, t


@pytest.mark.parametrize("dim", [2, 3])
def test_volume_and_membrane_functional(rigs, dim):
    from cgx_hip.functionals import MembraneFunctional, VolumeFunctional
    p = rigs(dim, False).p
    vol_i, vol_e, mem, t = _integrands(p)
    FV, FM = VolumeFunctional(p, vol_i, vol_e, degree=6), MembraneFunctional(p, mem, degree=10)
    try:
        for time in (0.0137, 0.0211):                                   # the second call reads the Constant anew
            t.value = time
            _, _, want, scale = functional_ref.reference(p, vol_i, vol_e, degree=6)
            _, _, wl, _ = functional_ref.reference(p, vol_i, vol_e, degree=6, longdouble=True)
            tol = FI.tolerance(float(np.max(np.abs(want - wl) / scale)))
            got = FV.value()
            err = np.abs(got - want) / scale
            print(f"ERR volume functional dim={dim} t={time} " + " ".join(f"{e:.2e}" for e in err.max(axis=0)) + f" tolerance {tol:.1e}")
            assert np.isfinite(got).all() and err.max() <= tol
            _, want, scale = mref.reference(p, mem, degree=10)
            _, wl, _ = mref.reference(p, mem, degree=10, longdouble=True)
            tol = FI.tolerance(float(np.max(np.abs(want - wl) / scale)))
            got = FM.value()
            err = np.abs(got - want) / scale
            print(f"ERR membrane functional dim={dim} t={time} " + " ".join(f"{e:.2e}" for e in err.max(axis=0)) + f" tolerance {tol:.1e}")
            assert np.isfinite(got).all() and err.max() <= tol
    finally:
        FV.close()
        FM.close()


# ------------------------------------------------------------------------------------------ a state program
class Oscillator(IonicModel):
    """a passive current and one general state driven by a travelling sine wave: dw/dt = A sin(omega t - k x) cos(80 phi_m) - B tanh(w)"""

    def __str__(self):
        return "sine-driven state"

    def _init(self):
        p = self.problem
        x = fem.SpatialCoordinate(p.mesh)
        self.time = fem.Constant(p.mesh, 0.0137)
        self.w = self.add_state("w", np.linspace(-0.5, 0.5, p.mesh.num_vertices),
                                rhs=lambda w: 4000.0 * fem.sin(300.0 * self.time - 4.0e6 * x[0]) * fem.cos(80.0 * p.phi_m_prev) - 2500.0 * fem.tanh(3.0 * w))

    def _eval(self, ion_idx):
        return self.problem.phi_m_prev * (1.0 + 0.1 * self.w)


@pytest.mark.parametrize("kind,N", [("square", 11), ("cube", 6)])      # 144 and 343 vertices (cube 7 has 512: no partial block)
def test_state_program_with_sin(kind, N):
    p = make_problem(ci_config(N=N, steps=1, kind=kind), lambda q: [Oscillator(q)])
    rng = np.random.default_rng(4)
    n = p.mesh.num_vertices
    assert n % 128 != 0 and n > 128                                        # several blocks and a partial last one
    p.phi_m_prev.x.array[:] = torch.as_tensor(rng.uniform(-0.1, 0.05, n), device=p.mesh.device)
    p.state_rush_larsen, p.state_substeps = False, 5
    model = p.ionic_models[0]
    ops = {T.INV[r[0]] for r in p.state_variables[0].spec.code.tolist()}
    assert {"SIN", "COS", "TANH"} <= ops
    be = p.create_backend()
    y = [st.function.numpy().copy() for st in p.state_variables]
    xs = p.mesh.geometry.x
    seen = []
    for time in (0.0137, 0.0211):
        model.time.value = time
        be.state_update()
        got = p.state_variables[0].function.numpy().copy()
        y = SR.state_step(p.state_variables, y, p.phi_m_prev.numpy(), float(p.dt.value), False, 5, x=[xs[:, d] for d in range(xs.shape[1])])
        scale = float(np.max(np.abs(y[0])))
        err = float(np.max(np.abs(got - y[0].astype(np.float64)))) / scale
        print(f"ERR state {kind}{N} t={time}: max |y| = {scale:.3e}, relative error {err:.2e}")
        assert np.isfinite(got).all() and err <= TOL
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1])
