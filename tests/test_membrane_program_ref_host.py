"""The conformance suite of the membrane bytecode (tests/membrane_program_ref.py) really has the properties the GPU comparison
(test_gpu_membrane_programs.py) relies on -- checked here without a GPU, on the meshes the GPU tests use:

* the programs are valid, compile for gfx950, use all 30 opcodes, register 47, 64 constants, an even and an odd constant count, and the
  hoisting table of the code generator overflows;
* scaling: per field block the mechanism term of ``b`` is at least as large as the rest of ``b`` on the membrane rows;
* conditioning: the fp64 and the long-double evaluation of the programs agree to 1e-14 of the mechanism term's per-block maximum,
  and so do two evaluations whose inputs differ by one rounding (no cancellation inside a program or at a guard);
* comparisons: no operand pair of LT/GT/LE/GE is closer than 1e-9 relative -- except a register compared with itself, which is
  exact and the one input at which LT/LE and GT/GE differ; EQ only where the answer is exact;
* both outcomes of every per-point comparison and logical operation and both arms of every per-point SEL occur among the
  quadrature points of one facet -- hence of one facet block of every kernel, whatever the facet order.  Constant-only
  instructions have one outcome by construction (the hoisting program has two constant-only SELs, one for each arm);
* no NaN reaches an output.
"""
import ctypes as C

import numpy as np
import pytest

import membrane_program_ref as R
from parity_utils import ci_config, make_oracle, make_problem

DIMS = (2, 3)
FACETS_PER_BLOCK = {2: (8,), 3: (16, 4)}     # 64 threads; 8 lanes per facet in 2D, 4 or 16 lanes per facet in 3D


@pytest.fixture(scope="module")
def world():
    out = {}
    for dim in DIMS:
        kind, N = R.MESHES[dim]
        o = R.fill_fields(make_oracle(N, kind))
        out[dim] = (o, R.point_inputs(o, np.longdouble), R.point_inputs(o, np.float64))
    return out


def _cases():
    return [(dim, v, name) for dim in DIMS for v in (0, 1) for name in R.tables(dim, v)]


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


@pytest.mark.parametrize("dim", DIMS)
def test_programs_are_valid_and_cover_the_language(dim):
    s = R.suite(dim)
    names = [e[0] for e in s]
    assert len(set(names)) == len(s) >= 6 and set(R.JIT_SINGLES) <= set(names)
    ops, x_axes, aux, ki, ke, powi = set(), set(), set(), set(), set(), set()
    for name, code, consts, _ in s:
        assert code.dtype == np.int32 and code.shape[1] == 4
        assert R.check_program(code, len(consts), dim) is None, name
        for op, d, a, b in code.tolist():
            nm = R.INV[op]
            ops.add(nm)
            {"X": x_axes, "AUX": aux, "KI": ki, "KE": ke}.get(nm, set()).add(a)
            if nm == "POWI":
                powi.add(b)
    assert ops == set(R.OPS) and len(ops) == 30
    assert x_axes == set(range(dim)) and {0, R.KNP_MAX_AUX - 1} <= aux and ki == ke == {0, 1, 2} and {-3, 0, 1, 7} <= powi
    by = {e[0]: e for e in s}
    assert R.n_regs(by["regs48"][1]) == R.KNP_MAX_PROG_REGS == 48 and 47 in by["regs48"][1][:, 1]
    code = by["regs48"][1].tolist()
    first = code[0]
    assert R.INV[first[0]] == "KI" and first[1] == 47
    last_use = max(i for i, r in enumerate(code) if R.INV[r[0]] != "OUT" and 47 in r[2:4])
    assert last_use >= 40 and not any(r[1] == 47 and R.INV[r[0]] != "OUT" for r in code[1:last_use])     # live across 40 instructions
    assert any(R.INV[r[0]] == "ADD" and r[1] == r[2] == r[3] for r in code)                             # d == a == b
    assert any(R.INV[r[0]] == "SEL" and r[1] == r[3] for r in code)                                     # SEL with d == b
    assert len(by["c64"][2]) == R.KNP_DIAG_MAX_CONSTS == 64 and any(R.INV[r[0]] == "CONST" and r[2] == 63 for r in by["c64"][1].tolist())
    assert {len(e[2]) % 2 for e in s} == {0, 1}
    # OUT twice to one channel inside one program
    assert any(sum(1 for r in e[1].tolist() if R.INV[r[0]] == "OUT" and r[2] == 0) >= 2 for e in s)
    # the mixed table: all different in length, register count and constant count
    for key in (lambda e: len(e[1]), lambda e: R.n_regs(e[1]), lambda e: len(e[2])):
        assert len({key(e) for e in s}) == len(s), [key(e) for e in s]
    # variant 1 is the same code with other constants, none of them a threshold
    for e0, e1 in zip(s, R.suite(dim, 1)):
        assert np.array_equal(e0[1], e1[1]) and len(e0[2]) == len(e1[2])
    assert sum(not np.array_equal(e0[2], e1[2]) for e0, e1 in zip(s, R.suite(dim, 1))) >= 6


@pytest.mark.parametrize("dim", DIMS)
def test_hoisting_table_overflows(dim):
    """more constant-only instructions than KNP_JIT_UNIFORMS = 16 (csrc/knp_jit.cpp): slots 0..15 fill, later ones are evaluated per
    point, and one of those is an operand afterwards; a constant-only SEL, a DIV and an EXP sit in the table"""
    code = {e[0]: e for e in R.suite(dim)}["hoist"][1]
    kinds = R.uniform_trace(code)
    rows = code.tolist()
    assert kinds.count("slot") == 16 and kinds.count("overflow") >= 1
    over = [rows[i][1] for i, k in enumerate(kinds) if k == "overflow"]
    first = kinds.index("overflow")
    assert any(R.INV[r[0]] != "OUT" and (r[2] in over or r[3] in over) for r in rows[first + 1:])
    slot_ops = [R.INV[rows[i][0]] for i, k in enumerate(kinds) if k == "slot"]
    assert {"DIV", "EXP", "SEL"} <= set(slot_ops) and slot_ops.count("SEL") == 2
    # no shipped-size program without overflow hides it: with a larger table nothing would overflow
    assert R.uniform_trace(code, table=64).count("overflow") == 0
    # a register that is hoisted, then per-point, then a constant again -- and constant, per-point, hoisted
    hist = {}
    for r, k in zip(rows, kinds):
        nm = R.INV[r[0]]
        if nm != "OUT":
            hist.setdefault(r[1], []).append("const" if nm == "CONST" else "slot" if k == "slot" else "point")
    seqs = ["".join(h[0] for h in v) for v in hist.values()]      # c(onst) s(lot) p(oint)
    assert any("spc" in q for q in seqs) and any("cps" in q for q in seqs), seqs


def test_suite_compiles_for_gfx950():
    from cgx_hip import _lib
    lib = _lib.load()
    seen = set()
    for dim in DIMS:
        for name, code, consts, _ in R.suite(dim):
            if code.tobytes() in seen:
                continue
            seen.add(code.tobytes())
            code = np.ascontiguousarray(code, dtype=np.int32)
            log = C.create_string_buffer(4096)
            rc = lib.knp_jit_compile_check(code.ctypes.data_as(C.POINTER(C.c_int32)), code.shape[0], b"gfx950", log, 4096)
            assert rc == 0 and log.value.decode().startswith("ok"), (name, log.value.decode())


@pytest.mark.parametrize("dim", DIMS)
def test_native_problem_sees_the_same_facets_and_every_block_is_mixed(dim):
    kind, N = R.MESHES[dim]
    o = make_oracle(N, kind)
    p = make_problem(ci_config(N=N, steps=1, kind=kind))
    n_g = p._fv.shape[0]
    assert n_g == o.fv.shape[0] and np.array_equal(p.local_mesh.coords, o.coords)
    assert sorted(map(tuple, np.sort(p._fv, axis=1).tolist())) == sorted(map(tuple, np.sort(o.fv, axis=1).tolist()))
    assert [f.name for f in p.aux_functions] == list(R.AUX_NAMES[:3])
    # a partial last block where the geometry allows one (a closed box surface always has a multiple of 4 facets: the 16-lane 3D
    # kernels, 4 facets per block, have no idle lanes here)
    assert n_g % FACETS_PER_BLOCK[dim][0] != 0 and n_g > 2 * FACETS_PER_BLOCK[dim][0]
    K = len(R.suite(dim))
    prog = R.facet_programs(p._fv, K)
    assert set(prog.tolist()) == set(range(K))
    for per in FACETS_PER_BLOCK[dim]:
        for lo in range(0, n_g, per):
            assert len(set(prog[lo:lo + per].tolist())) > 1, (per, lo)
    # two facet groups of unequal size, one of them no multiple of 128
    sizes = [int(np.isin(prog, g).sum()) for g in R.GROUPS]
    assert sizes[0] != sizes[1] and min(sizes) > 0 and any(n % 128 for n in sizes) and sum(sizes) == n_g


@pytest.mark.parametrize("dim,variant,name", _cases())
def test_scaling_conditioning_and_no_nan(world, dim, variant, name):
    o, inp_ld, inp_d = world[dim]
    table = R.tables(dim, variant)[name]
    Iq = R.currents(o, table, np.longdouble, inp_ld)
    assert np.isfinite(Iq).all()
    b, mech, rows = R.rhs_reference(o, Iq)
    rest = b - mech
    mem = np.zeros(b.shape[0] // 4, dtype=bool)
    mem[rows] = True
    for f in range(4):
        assert np.max(np.abs(mech[f::4])) >= np.max(np.abs(rest[f::4][mem])), (f, np.max(np.abs(mech[f::4])), np.max(np.abs(rest[f::4][mem])))
        assert np.max(np.abs(mech[f::4][~mem])) == 0.0
    # fp64 against long double
    _, mech_d, _ = R.rhs_reference(o, R.currents(o, table, np.float64, inp_d))
    for f in range(4):
        assert np.max(np.abs(mech_d[f::4] - mech[f::4])) <= 1e-14 * np.max(np.abs(mech[f::4])), f
    # inputs one rounding away (what another summation order of the interpolation gives): the same bound times 10
    rng = np.random.default_rng(7)
    jig = lambda a: a if a is None else a * (1 + np.finfo(np.float64).eps * rng.choice([-1.0, 0.0, 1.0], size=a.shape))
    inp_j = {k: [jig(a) for a in v] if isinstance(v, list) else jig(v) for k, v in inp_ld.items()}
    _, mech_j, _ = R.rhs_reference(o, R.currents(o, table, np.longdouble, inp_j))
    for f in range(4):
        assert np.max(np.abs(mech_j[f::4] - mech[f::4])) <= 1e-13 * np.max(np.abs(mech[f::4])), f


@pytest.mark.parametrize("dim", DIMS)
def test_comparisons_keep_their_distance_and_take_both_branches(world, dim):
    o, inp, _ = world[dim]
    seen = {nm: 0 for nm in R.COMPARES + ("AND", "OR", "NOT", "SEL", "EQ")}
    same_reg = set()
    one_facet = lambda flag: bool(np.any(flag.any(axis=1) & (~flag).any(axis=1)))       # both values among one facet's points
    for entry in R.suite(dim):
        name, code = entry[0], entry[1]
        kinds = R.uniform_trace(code, table=1 << 30)
        eq = []
        for i, (op, d, a, b) in enumerate(code.tolist()):
            nm = R.INV[op]
            if nm not in seen:
                continue
            uniform = kinds[i] == "slot"
            va, vb = R.probe(entry, i, a, inp), R.probe(entry, i, b, inp)
            if nm in R.COMPARES and a == b:                 # a register against itself: exact, like EQ
                out = R.probe(entry, i + 1, d, inp)
                assert np.all(out == (1.0 if nm in ("LE", "GE") else 0.0)), (name, i, nm)
                same_reg.add(nm)
                continue
            if nm in R.COMPARES:
                gap = np.min(np.abs(va - vb) / np.maximum(np.abs(va), np.abs(vb)))
                assert gap >= 1e-9, (name, i, nm, float(gap))
            if nm == "EQ":
                exact = a == b or (uniform and np.all(va == vb))
                differ = bool(np.all(np.abs(va - vb) >= 1e-9 * np.maximum(np.abs(va), np.abs(vb))))
                assert exact or differ, (name, i)
                eq.append(1 if exact else 0)
            elif not uniform:
                out = R.probe(entry, i + 1, d, inp)
                flag = (va != 0) if nm == "SEL" else (out != 0)
                assert one_facet(flag), (name, i, nm)
            seen[nm] += 1
        if eq:
            assert sorted(set(eq)) == [0, 1], name
    assert all(n > 0 for n in seen.values()), seen
    assert same_reg == set(R.COMPARES)             # equality, the one input at which LT/LE and GT/GE differ
    # the guard pattern: the untaken arm of a SEL is NaN at some points and the output is finite everywhere
    entry = {e[0]: e for e in R.suite(dim)}["logic"]
    rows = entry[1].tolist()
    guards = [i for i, r in enumerate(rows) if R.INV[r[0]] == "SEL" and np.isnan(R.probe(entry, i, r[3], inp)).any()]
    assert guards
    for i in guards:
        cond, arm = R.probe(entry, i, rows[i][2], inp), R.probe(entry, i, rows[i][3], inp)
        assert not np.isnan(arm[cond != 0]).any() and np.isnan(arm[cond == 0]).any()
