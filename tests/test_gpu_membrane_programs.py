"""Every opcode of the membrane-program bytecode on the three GPU engines that execute it, against the host reference of
tests/membrane_program_ref.py (``fem.interpret_program`` in long double, assembled by the oracle):

1. the ahead-of-time interpreter in the right-hand-side facet kernel (``run_program`` in csrc/knp_gamma_facets.inc, ``KNP_JIT=0``):
   every program as a single-program table (the LDS-resident path) and the mixed table (a block serialises over its programs);
2. the run-time compiled kernels of csrc/knp_jit.cpp: ``knp_gamma_vec_2d``, ``knp_gamma_vec_3d_q1`` (3D default),
   ``knp_gamma_vec_3d_many`` (``KNP_GAMMA_QV=9``) and ``knp_gamma_vec_3d`` (``KNP_GAMMA_MANY=0``, read once per process: a child);
3. the diagnostic interpreter ``k_diag_facets`` (csrc/knp_diagnostics.inc) through ``membrane_integral``.

The right-hand side is compared on every row, per field block, relative to the largest MECHANISM term of the block (the host test
test_membrane_program_ref_host.py shows that this term dominates the block): 1e-12, the project's tolerance for assembled vectors.
It is more than 100 times the long-double / fp64 agreement the host test asserts (1e-14) and more than 10 times a worst case of
36 points x ~10 operations x 2 ulp.  The run-time compiled code and the interpreter agree to 1e-13 of the same scale.

Shapes: square 11 (20 facets: blocks of 8, 8, 4) and cube 7 (108 facets: blocks of 16 end with 12).  The 16-lane 3D kernels take
4 facets per block and a closed box surface always has a multiple of 4 facets: their idle-lane path is exempt.

Largest errors measured on MI355X, in these units: interpreter 1.4e-15 (2D) / 9.2e-16 (3D); run-time compiled 1.4e-15 (2D),
9.2e-16 (3D, each of the three kernels); run-time compiled against interpreter 4.0e-16 / 4.3e-16; diagnostic integral 5.6e-16 / 2.9e-16.
The more-than-64-KiB LDS request is granted, also after another context has launched the kernel with a small request.
"""
from __future__ import annotations

import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import membrane_program_ref as R
from parity_utils import ci_config, make_oracle, make_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, TOL_ENGINES = 1e-12, 1e-13
ENGINES = {"interp": {"KNP_JIT": "0"}, "jit": {"KNP_JIT": "1"}, "jit_qv9": {"KNP_JIT": "1", "KNP_GAMMA_QV": "9"}}
NAMES = [f.__name__[1:] for f in R.BUILDERS]
JIT_TABLES = ["mixed"] + list(R.JIT_SINGLES)


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
        Iq = R.currents(o, R.tables(dim, variant)[name])
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
        per = 8 if dim == 2 else 16
        assert p._fv.shape[0] % per != 0 and p._fv.shape[0] > 2 * per          # several blocks and a partial last one
        p.gamma_tags = tuple(range(K))
        p.local_mesh.gamma_tags = tags
        p.gamma_facet_tags = tags
        p.tag_program = {k: (k if mixed else 0) for k in range(K)}
        p.programs = self._specs("mixed" if mixed else NAMES[0], 0)
        self.p, self.be = p, p.create_backend()
        self.results = {}

    def _specs(self, name, variant):
        assert (name == "mixed") == self.mixed
        return {i: R.spec_of(e) for i, e in enumerate(R.tables(self.dim, variant)[name])}

    def status(self):
        return self.be.lib.knp_jit_status(self.be.ctx).decode()

    def assemble(self):
        self.be.assemble_matrix()
        self.be.assemble_rhs()
        return self.be.b.cpu().numpy().copy()

    def rhs(self, engine, name, variant=0, fresh=False):
        """(b, jit status) of table ``name`` on ``engine``: uploads the programs (which rebuilds the native code or switches it off)"""
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
def test_runtime_compiled_code_matches_reference(rigs, dim, engine, name):
    b, status = rigs(dim, name == "mixed").rhs(engine, name)
    _check_status(engine, status)
    _compare(engine, b, dim, name)


@pytest.mark.parametrize("name", JIT_TABLES)
@pytest.mark.parametrize("dim,engine", [(2, "jit"), (3, "jit"), (3, "jit_qv9")])
def test_runtime_compiled_code_equals_interpreter(rigs, dim, engine, name):
    rig = rigs(dim, name == "mixed")
    (b_jit, st_jit), (b_int, st_int) = rig.rhs(engine, name), rig.rhs("interp", name)
    _check_status(engine, st_jit)
    _check_status("interp", st_int)
    mech = reference(dim, name)[1]
    err = R.block_errors(b_jit, b_int, mech)
    print(f"ERR {engine}-vs-interp dim={dim} table={name} " + " ".join(f"{e:.2e}" for e in err))
    assert max(err) <= TOL_ENGINES, err


CHILD = """
import sys; sys.path[:0] = ['tests', 'oracle', 'knp-emi-cgx_amd']; import conftest, json, numpy as np
import test_gpu_membrane_programs as T
names, path = json.loads(sys.argv[1]), sys.argv[2]
rigs, out, status = {}, {}, {}
for name in names:
    mixed = name == 'mixed'
    if mixed not in rigs:
        rigs[mixed] = T.Rig(3, mixed)
    out[name], status[name] = rigs[mixed].rhs('jit', name)
np.savez(path, **out)
print('RESULT' + json.dumps(status))
"""


@pytest.fixture(scope="module")
def many0_leg(tmp_path_factory):
    """KNP_GAMMA_MANY=0 keeps the 16 lanes x 3 points kernel knp_gamma_vec_3d; the switch is read once per process: a fresh child"""
    path = str(tmp_path_factory.mktemp("membrane_programs") / "many0.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("KNP_JIT", "KNP_GAMMA_QV")}
    out = subprocess.run([sys.executable, "-c", CHILD, json.dumps(JIT_TABLES), path], cwd=ROOT, env=dict(env, KNP_GAMMA_MANY="0"),
                         capture_output=True, text=True, timeout=300)
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
    assert out.returncode == 0 and line, f"exit status {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(line[0][6:]), dict(np.load(path))


@pytest.mark.parametrize("name", JIT_TABLES)
def test_runtime_compiled_16_lane_kernel_matches_reference(many0_leg, rigs, name):
    status, b = many0_leg
    _check_status("jit", status[name])
    _compare("jit_many0", b[name], 3, name)
    b_int, _ = rigs(3, name == "mixed").rhs("interp", name)
    err = R.block_errors(b[name], b_int, reference(3, name)[1])
    print(f"ERR jit_many0-vs-interp dim=3 table={name} " + " ".join(f"{e:.2e}" for e in err))
    assert max(err) <= TOL_ENGINES, err


@pytest.mark.parametrize("engine", ["interp", "jit"])
@pytest.mark.parametrize("dim", [2, 3])
def test_new_constants_are_followed_without_new_programs(rigs, dim, engine):
    """knp_set_program_constants after a first assembly -- among them constants that feed hoisted instructions: the next
    right-hand side follows them; the native code stays in place (constants are run-time data)"""
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
    """k_diag_facets: constants as kernel arguments, code from global memory, one quadrature point at a time"""
    import torch
    rig, o = rigs(dim, False), oracle(dim)
    be = rig.be
    tags = R.facet_programs(o.fv, len(NAMES))
    group = np.where(np.isin(tags, R.GROUPS[0]), 0, 1)
    sizes = np.bincount(group, minlength=2)
    assert sizes[0] != sizes[1] and sizes.min() > 0 and (sizes % 128 != 0).any()
    be.set_facet_groups([list(g) for g in R.GROUPS])
    out = torch.zeros(2, dtype=torch.float64, device=be.device)
    for variant in (0, 1):
        spec = R.spec_of(R.tables(dim, variant)[name][0])
        if variant == 0:
            be.set_diag_program(spec)
        else:
            be.refresh_diag_constants(spec)                 # knp_diag_set_program_constants: the next call follows
        got = be.membrane_integral(out).cpu().numpy().copy()
        want, mag = R.integral_reference(o, reference(dim, name, variant)[2], group, 2)
        err = np.abs(got - want) / mag
        print(f"ERR diag dim={dim} table={name} variant={variant} " + " ".join(f"{e:.2e}" for e in err))
        assert np.isfinite(got).all() and err.max() <= TOL, (variant, got, want)
    w0 = R.integral_reference(o, reference(dim, name, 0)[2], group, 2)[0]
    assert np.all(np.abs(want - w0) > 1e-3 * np.abs(w0))                # the constants did change the answer


def test_large_register_file_3d_and_a_second_context(rigs):
    """The 48-register program on the 3D interpreter asks for more than 64 KiB of dynamic LDS (hipFuncSetAttribute, cached per
    context in gamma_lds_set).  A second context with a small program then launches the same kernel with a small request, and
    the first context assembles again without any new upload: both must still match their references."""
    a = rigs(3, False)
    regs = R.n_regs(R.tables(3)["regs48"][0][1])
    assert regs == 48 and regs * 3 * 64 * 8 > 64 * 1024          # [n_regs][QV = 3][64 threads] doubles
    b, status = a.rhs("interp", "regs48", fresh=True)
    _check_status("interp", status)
    _compare("interp large-lds", b, 3, "regs48")
    other = Rig(3, False)
    b2, status2 = other.rhs("interp", "tiny")
    _check_status("interp", status2)
    _compare("interp second-context", b2, 3, "tiny")
    with _environ(ENGINES["interp"]):
        b3 = a.assemble()
    _compare("interp large-lds again", b3, 3, "regs48")
    assert np.array_equal(b3, b)
