"""``fem.sin`` / ``fem.cos`` / ``fem.tanh`` and their opcodes KNP_OP_SIN / COS / TANH (30..32) without a GPU: the Python side of the
language (compiler, both host evaluators, the opcode tables and the header), and the properties of the conformance suite
tests/trig_program_ref.py that the GPU comparison (test_gpu_trig_programs.py) relies on, on the meshes the GPU tests use:

* the programs are valid, compile for gfx950 and hold every function with d == a and d != a, constant-only (hoisted by the run-time
  compiler) and per point, on all three channels, with an even and an odd constant count;
* arguments computed in a program stay below 8; the large arguments of SIN / COS are exactly the constants of ``LARGE`` (or their
  negatives), so the long-double reference sees the numbers the device sees; TANH meets tiny, moderate and saturating arguments;
* scaling and conditioning as in test_membrane_program_ref_host.py: the mechanism term dominates every field block on the membrane
  rows, and the fp64 and long-double evaluations agree to 1e-14 of its per-block maximum (1e-13 with inputs one rounding away).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import membrane_program_ref as R
import trig_program_ref as T
from parity_utils import ci_config, make_oracle, make_problem

from cgx_hip import _lib, fem

DIMS = (2, 3)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the language
def test_opcode_tables_and_header_agree():
    assert len(_lib.OPS) == 30 and max(_lib.OPS.values()) == 29              # the base table stays what the existing suite pins
    assert _lib.FUNC_OPS == dict(SIN=30, COS=31, TANH=32)
    assert _lib.ALL_OPS == {**_lib.OPS, **_lib.FUNC_OPS} and len(set(_lib.ALL_OPS.values())) == 33
    text = open(os.path.join(ROOT, "include", "knpemi_hip.h")).read()
    enum = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bKNP_OP_([A-Z]+)\s*=\s*(\d+)", text)}
    assert enum == _lib.ALL_OPS


def _mesh2():
    class G:
        dim = 2

    class M:
        geometry = G()
    return M()


def test_functions_compile_to_their_opcodes():
    x = fem.SpatialCoordinate(_mesh2())
    for f, name in ((fem.sin, "SIN"), (fem.cos, "COS"), (fem.tanh, "TANH")):
        spec = fem.compile_program([f(x[0]), f(2.0), 0.0], {})
        rows = [r for r in spec.code.tolist() if r[0] == _lib.FUNC_OPS[name]]
        assert len(rows) == 2 and all(r[3] == 0 for r in rows), (name, spec.code.tolist())
        assert not any(r[0] in _lib.FUNC_OPS.values() and r[0] != _lib.FUNC_OPS[name] for r in spec.code.tolist())
    assert fem.pi == np.pi
    # a number is taken as a literal, as by the other UFL-named helpers
    assert isinstance(fem.sin(1.0), fem.Op) and fem.sin(1.0).op == "SIN"


def test_compiler_interpreter_and_numpy_agree_on_random_points():
    rng = np.random.default_rng(3)
    x = fem.SpatialCoordinate(_mesh2())
    t = fem.Constant(None, 0.37)
    A, omega, k = 2.5, 2.0 * fem.pi * 3.0, 1.7
    outs = [A * fem.sin(omega * t) * fem.cos(k * x[0]) + fem.tanh(x[1] - 0.5),
            fem.sin(x[0]) ** 2 + fem.cos(x[0]) ** 2,
            fem.conditional(fem.gt(x[0], 0.0), fem.tanh(4.0 * x[0]), fem.sin(-x[1])) / (2.0 + fem.cos(x[0] * x[1]))]
    spec = fem.compile_program(outs, {})
    X = [rng.uniform(-3.0, 3.0, 257), rng.uniform(-3.0, 3.0, 257)]
    for time in (0.37, 1.91):
        t.value = time
        got = fem.interpret_program(spec, [0.0] * 3, [0.0] * 3, 0.0, [], X)
        want = [A * np.sin(omega * time) * np.cos(k * X[0]) + np.tanh(X[1] - 0.5),
                np.sin(X[0]) ** 2 + np.cos(X[0]) ** 2,
                np.where(X[0] > 0.0, np.tanh(4.0 * X[0]), np.sin(-X[1])) / (2.0 + np.cos(X[0] * X[1]))]
        for j in range(3):
            ev = fem.evaluate_numpy(outs[j], {"x": X, "fields": {}})
            assert np.array_equal(np.asarray(got[j]), np.asarray(ev))                 # the same NumPy calls in the same order
            assert np.allclose(got[j], want[j], rtol=1e-14, atol=1e-14), j
    assert np.allclose(got[1], 1.0, rtol=0, atol=4e-16)


def test_state_programs_take_the_functions():
    """compile_state_program goes through the same compiler: a rate with sin() of another field and tanh() of the state itself"""
    p = make_problem(ci_config(N=4, steps=1))
    y = fem.Function(p.V, "osc")
    st = fem.StateVariable("osc", y, 1, lambda: (fem.sin(3.0 * p.phi_m_prev) - fem.tanh(y) + fem.cos(0.5),), None)
    spec = fem.compile_state_program(st, {id(p.phi_m_prev): ("PHIM", 0)}, [])
    ops = [T.INV[r[0]] for r in spec.code.tolist()]
    assert {"SIN", "COS", "TANH"} <= set(ops) and st.aux_index == 0
    got = fem.interpret_program(spec, [0.0] * 3, [0.0] * 3, -0.07, [0.2], [0.0] * 3)
    assert got[0] == pytest.approx(np.sin(3.0 * -0.07) - np.tanh(0.2) + np.cos(0.5), rel=1e-15)


# ------------------------------------------------------------------------------------------ the suite
@pytest.fixture(scope="module")
def world():
    out = {}
    for dim in DIMS:
        kind, N = R.MESHES[dim]
        o = R.fill_fields(make_oracle(N, kind))
        out[dim] = (o, R.point_inputs(o, np.longdouble), R.point_inputs(o, np.float64))
    return out


def _cases():
    return [(dim, v, name) for dim in DIMS for v in (0, 1) for name in T.tables(dim, v)]


@pytest.mark.parametrize("dim", DIMS)
def test_programs_are_valid_and_cover_the_function_block(dim):
    s = T.suite(dim)
    assert [e[0] for e in s] == list(T.NAMES)
    where = {f: {"alias": 0, "fresh": 0, "uniform": 0, "point": 0} for f in T.FUNCS}
    for name, code, consts, _ in s:
        assert code.dtype == np.int32 and code.shape[1] == 4
        assert T.check_program(code, len(consts), dim) is None, name
        uni = T.uniform_trace(code)
        for (op, d, a, b), u in zip(code.tolist(), uni):
            nm = T.INV[op]
            if nm in T.FUNCS:
                assert b == 0
                where[nm]["alias" if d == a else "fresh"] += 1
                where[nm]["uniform" if u else "point"] += 1
        assert {r[2] for r in code.tolist() if T.INV[r[0]] == "OUT"} == {0, 1, 2}, name          # all three channels
    assert all(n > 0 for w in where.values() for n in w.values()), where
    assert {len(e[2]) % 2 for e in s} == {0, 1}
    for key in (lambda e: len(e[1]), lambda e: T.n_regs(e[1]), lambda e: len(e[2])):             # the mixed table: all different
        assert len({key(e) for e in s}) == len(s), [key(e) for e in s]
    for e0, e1 in zip(s, T.suite(dim, 1)):                                                       # variant 1: other constants, same code
        assert np.array_equal(e0[1], e1[1]) and len(e0[2]) == len(e1[2]) and not np.array_equal(e0[2], e1[2])
        big = np.abs(e0[2]) >= 700.0
        assert np.array_equal(e0[2][big][1:], e1[2][big][1:])                                    # the scale S apart, no large argument moves
    assert all(float(np.float64(v)) == v and float(np.longdouble(v)) == v for v in T.LARGE)


@pytest.mark.parametrize("dim", DIMS)
def test_arguments_are_small_where_computed_and_exact_where_large(world, dim):
    o, inp, _ = world[dim]
    exact = {v for c in T.LARGE for v in (c, -c)} | {750.0, -1.0e4}
    seen_large, tanh_args = set(), []
    for entry in T.suite(dim):
        for i, (op, d, a, b) in enumerate(entry[1].tolist()):
            nm = T.INV[op]
            if nm not in T.FUNCS:
                continue
            arg = np.asarray(T.probe(entry, i, a, inp), dtype=np.longdouble)
            assert np.isfinite(arg).all()
            if nm == "TANH":
                tanh_args.append(np.abs(arg).astype(np.float64).ravel())
            small = np.abs(arg) < 8.0
            if nm == "TANH":
                small |= np.abs(arg) <= 50.0 + 1e-9            # saturated: tanh' is zero there, the argument's rounding does not show
            vals = {float(v) for v in np.unique(arg[~small])}
            assert vals <= exact, (entry[0], i, nm, sorted(vals)[:4])
            if nm != "TANH":
                seen_large |= vals
                if len(vals) > 1:                              # a per-point SEL: both values among the points of one facet
                    lo = arg == min(vals)
                    assert np.any(lo.any(axis=1) & (~lo).any(axis=1)), (entry[0], i)
    assert {abs(v) for v in seen_large} == set(map(abs, T.LARGE)) and min(seen_large) < 0 < max(seen_large)
    t = np.concatenate(tanh_args)
    assert (t < 1e-6).any() and ((t > 0.1) & (t < 3.0)).any() and ((t > 20.0) & (t <= 50.0)).any() and (t == 750.0).any() and (t == 1.0e4).any()


def test_suite_compiles_for_gfx950():
    lib = _lib.load()
    seen = set()
    for dim in DIMS:
        for name, code, consts, _ in T.suite(dim):
            if code.tobytes() in seen:
                continue
            seen.add(code.tobytes())
            code = np.ascontiguousarray(code, dtype=np.int32)
            log = C.create_string_buffer(4096)
            rc = lib.knp_jit_compile_check(code.ctypes.data_as(C.POINTER(C.c_int32)), code.shape[0], b"gfx950", log, 4096)
            assert rc == 0 and log.value.decode().startswith("ok"), (name, log.value.decode())


@pytest.mark.parametrize("dim", DIMS)
def test_every_block_of_the_mixed_table_is_mixed(dim):
    kind, N = R.MESHES[dim]
    p = make_problem(ci_config(N=N, steps=1, kind=kind))
    K = len(T.NAMES)
    prog = R.facet_programs(p._fv, K)
    assert set(prog.tolist()) == set(range(K))
    for per in {2: (8,), 3: (16, 4)}[dim]:
        assert sum(len(set(prog[lo:lo + per].tolist())) > 1 for lo in range(0, len(prog), per)) >= 2, per
    sizes = [int(np.isin(prog, g).sum()) for g in T.GROUPS]
    assert min(sizes) > 0 and sum(sizes) == len(prog)


@pytest.mark.parametrize("dim,variant,name", _cases())
def test_scaling_conditioning_and_no_nan(world, dim, variant, name):
    o, inp_ld, inp_d = world[dim]
    table = T.tables(dim, variant)[name]
    Iq = R.currents(o, table, np.longdouble, inp_ld)
    assert np.isfinite(Iq).all()
    b, mech, rows = R.rhs_reference(o, Iq)
    rest = b - mech
    mem = np.zeros(b.shape[0] // 4, dtype=bool)
    mem[rows] = True
    for f in range(4):
        assert np.max(np.abs(mech[f::4])) >= np.max(np.abs(rest[f::4][mem])), (f, np.max(np.abs(mech[f::4])), np.max(np.abs(rest[f::4][mem])))
    # fp64 against long double: the bound the existing suite holds
    _, mech_d, _ = R.rhs_reference(o, R.currents(o, table, np.float64, inp_d))
    err = [float(np.max(np.abs(mech_d[f::4] - mech[f::4])) / np.max(np.abs(mech[f::4]))) for f in range(4)]
    print(f"LD-vs-fp64 dim={dim} variant={variant} table={name} " + " ".join(f"{e:.2e}" for e in err))
    assert max(err) <= 1e-14, err
    # inputs one rounding away (what another summation order of the interpolation gives): the same bound times 10
    rng = np.random.default_rng(7)
    jig = lambda a: a if a is None else a * (1 + np.finfo(np.float64).eps * rng.choice([-1.0, 0.0, 1.0], size=a.shape))
    inp_j = {k: [jig(a) for a in v] if isinstance(v, list) else jig(v) for k, v in inp_ld.items()}
    _, mech_j, _ = R.rhs_reference(o, R.currents(o, table, np.longdouble, inp_j))
    for f in range(4):
        assert np.max(np.abs(mech_j[f::4] - mech[f::4])) <= 1e-13 * np.max(np.abs(mech[f::4])), f
