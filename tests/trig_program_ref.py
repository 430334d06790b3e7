"""Conformance suite of the function block of the membrane bytecode (``KNP_OP_SIN`` / ``COS`` / ``TANH``, include/knpemi_hip.h), in the
conventions of tests/membrane_program_ref.py, whose meshes, fields, evaluator and references it reuses: raw bytecode, every output
scaled by ``S`` so that the mechanism term dominates every field block of ``b``, an even and an odd constant count.  Shared by
test_trig_host.py (no GPU) and test_gpu_trig_programs.py.

Where the arguments come from decides what a comparison against the long-double reference can show:

* an argument COMPUTED in the program stays below 8 in magnitude: the reference rounds it differently from fp64, and through sin' that
  difference reaches the result at the size of the argument's ulp;
* large arguments (1e3 .. 1e15, negative too) reach SIN / COS straight from a load of a constant that holds an exactly representable
  value -- or from a SEL between two such constants, which makes the value differ from point to point without computing it: the
  reference sees the same number, and the engines' range reduction is what is compared;
* TANH at tiny arguments (tanh(t) / t), moderate ones and saturating ones (|x| > 20, and 750, where exp(2 x) overflows).
"""
from __future__ import annotations

import numpy as np

import membrane_program_ref as R

from cgx_hip._lib import ALL_OPS, FUNC_OPS

INV = {v: k for k, v in ALL_OPS.items()}
S = R.S
FUNCS = tuple(FUNC_OPS)
UNARY = R.UNARY + FUNCS
GROUPS = ((0, 1), (2, 3))          # membrane tag of a facet = its program id; the diagnostic integrals are taken over these two groups
LARGE = (1.0e3, -1.0e6, 1.0e9 + 0.5, -7.25e12, 1.0e15, 2.0 ** 40 + 1.0, -3.0e14)      # exactly representable in fp64, hence the same numbers in long double


def I(name, d=0, a=0, b=0):
    return (ALL_OPS[name], d, a, b)


def _point(dim, v):
    """the three functions per quadrature point with computed arguments below 8, d == a and d != a, coordinates of the first and the
    last axis, PHIM and an aux field as arguments, all three channels"""
    consts = [S * (1.5 if v else 1.0), 1.0e6, 6.0, -80.0, 0.3, 12.0 if v else 10.0, 2.0, 3.0, 0.5]          # odd count
    code = [I("CONST", 0, 0), I("CONST", 1, 1),
            I("X", 2, 0), I("MUL", 2, 2, 1), I("CONST", 3, 2), I("MUL", 2, 2, 3), I("SIN", 2, 2),               # sin(6 u), d == a
            I("PHIM", 4), I("CONST", 5, 3), I("MUL", 4, 4, 5), I("COS", 4, 4),                                  # cos(-80 phi_m) ~ cos(5.6 .. 6.8)
            I("AUX", 6, 3), I("CONST", 7, 4), I("SUB", 6, 6, 7), I("CONST", 8, 5), I("MUL", 6, 6, 8),
            I("TANH", 9, 6),                                                                                    # d != a, |x| <= 2.4
            I("CONST", 10, 6),
            I("X", 11, dim - 1), I("MUL", 11, 11, 1), I("CONST", 12, 7), I("MUL", 11, 11, 12), I("COS", 13, 11), I("SIN", 11, 11),
            I("CONST", 14, 8), I("MUL", 13, 13, 14), I("MUL", 11, 11, 14),
            I("ADD", 2, 2, 10), I("ADD", 2, 2, 13), I("MUL", 2, 2, 0), I("OUT", 0, 0, 2),
            I("ADD", 4, 4, 10), I("ADD", 4, 4, 11), I("MUL", 4, 4, 0), I("OUT", 0, 1, 4),
            I("TANH", 6, 6), I("ADD", 9, 9, 6), I("ADD", 9, 9, 10), I("ADD", 9, 9, 10), I("MUL", 9, 9, 0), I("OUT", 0, 2, 9)]
    return "point", code, consts, _point.__doc__


def _uniform(dim, v):
    """a sinusoidal stimulus A sin(omega t) cos(k x): SIN, COS and TANH of constants only (hoisted to once per thread by the run-time
    compiler) next to the same functions per point"""
    consts = [S * (0.75 if v else 1.0), 300.0, 0.0211 if v else 0.0137, 1.0e6, 4.0, 0.5, 1.5, 2.0]                # even count
    code = [I("CONST", 0, 0), I("CONST", 1, 1), I("CONST", 2, 2), I("MUL", 3, 1, 2),                          # omega t = 4.11 (6.33): slot
            I("SIN", 4, 3), I("COS", 5, 3), I("CONST", 6, 5), I("MUL", 7, 3, 6), I("TANH", 7, 7),              # slots; TANH with d == a
            I("X", 8, 0), I("CONST", 9, 3), I("MUL", 8, 8, 9), I("CONST", 9, 4), I("MUL", 8, 8, 9),            # k x = 4 u
            I("SIN", 10, 8), I("COS", 11, 8), I("CONST", 12, 7), I("SUB", 8, 8, 12), I("TANH", 8, 8),
            I("CONST", 13, 6),
            I("MUL", 11, 11, 4), I("ADD", 11, 11, 13), I("MUL", 11, 11, 0), I("OUT", 0, 0, 11),
            I("MUL", 10, 10, 5), I("ADD", 10, 10, 13), I("MUL", 10, 10, 0), I("OUT", 0, 1, 10),
            I("MUL", 8, 8, 7), I("ADD", 8, 8, 13), I("MUL", 8, 8, 0), I("OUT", 0, 2, 8)]
    return "uniform", code, consts, _uniform.__doc__


def _large(dim, v):
    """SIN and COS of 1e3, -1e6, 1e9 + 0.5, -7.25e12, 1e15, 2^40 + 1 and -3e14 straight from constant loads (constant-only: hoisted) and from SELs between
    two of them on a per-point condition (the same exact values, per point): the range reduction of every engine"""
    consts = [S * (2.0 if v else 1.0), 1.0e6, R.C_LO, 3.0] + list(LARGE)                                       # odd count
    c = lambda k: 4 + k
    code = [I("CONST", 0, 0), I("CONST", 1, 1), I("X", 2, 0), I("MUL", 2, 2, 1), I("CONST", 3, 2), I("LT", 2, 2, 3),   # u < C_LO, per point
            I("CONST", 4, c(0)), I("SIN", 5, 4), I("CONST", 6, c(1)), I("COS", 6, 6),                            # slots; COS with d == a
            I("CONST", 7, c(4)), I("SIN", 8, 7), I("COS", 9, 7),
            I("CONST", 10, c(2)), I("CONST", 11, c(3)), I("MOV", 12, 10), I("SEL", 12, 2, 11),                   # 1e9 + 0.5 | -7.25e12
            I("SIN", 13, 12), I("COS", 12, 12),
            I("MOV", 14, 7), I("SEL", 14, 2, 4), I("NEG", 14, 14),                                               # -1e15 | -1e3
            I("SIN", 15, 14), I("COS", 14, 14),
            I("CONST", 16, 3), I("CONST", 17, c(5)), I("SIN", 17, 17), I("CONST", 18, c(6)), I("COS", 19, 18), I("ADD", 17, 17, 19),
            I("ADD", 8, 8, 17),
            I("ADD", 5, 5, 6), I("ADD", 5, 5, 13), I("ADD", 5, 5, 16), I("MUL", 5, 5, 0), I("OUT", 0, 0, 5),
            I("ADD", 8, 8, 12), I("ADD", 8, 8, 16), I("MUL", 8, 8, 0), I("OUT", 0, 1, 8),
            I("ADD", 9, 9, 15), I("ADD", 9, 9, 14), I("ADD", 9, 9, 16), I("MUL", 9, 9, 0), I("OUT", 0, 2, 9)]
    return "large", code, consts, _large.__doc__


def _tanh(dim, v):
    """TANH at tiny arguments (tanh(t) / t with t ~ 1e-8), moderate ones, saturating ones per point (20 .. 50, positive and negative), 750
    from a constant and 750 | -1e4 from a per-point SEL"""
    consts = [S * (1.25 if v else 1.0), 1.0e-9, 1.0e6, R.C_HI, 0.3, 8.0, 20.0, 30.0, 750.0, -1.0e4, 2.0, 1.0]    # even count
    code = [I("CONST", 0, 0),
            I("KI", 1, 0), I("CONST", 2, 1), I("MUL", 1, 1, 2), I("TANH", 3, 1), I("DIV", 3, 3, 1),            # ~ 1 - t^2 / 3
            I("AUX", 4, 4), I("CONST", 5, 4), I("SUB", 4, 4, 5), I("CONST", 5, 5), I("MUL", 4, 4, 5), I("TANH", 4, 4),   # |x| <= 1.6
            I("X", 6, 1), I("CONST", 7, 2), I("MUL", 6, 6, 7),                                                   # u_1
            I("CONST", 8, 7), I("MUL", 9, 6, 8), I("CONST", 8, 6), I("ADD", 9, 9, 8), I("TANH", 10, 9),         # tanh(20 + 30 u) = 1
            I("NEG", 9, 9), I("TANH", 9, 9),                                                                     # -1
            I("CONST", 11, 8), I("TANH", 12, 11),                                                                # tanh(750): slot
            I("CONST", 13, 3), I("GT", 6, 6, 13), I("CONST", 14, 9), I("MOV", 15, 14), I("SEL", 15, 6, 11), I("TANH", 15, 15),   # 750 | -1e4
            I("CONST", 16, 10), I("CONST", 17, 11),
            I("ADD", 3, 3, 17), I("MUL", 3, 3, 0), I("OUT", 0, 0, 3),
            I("ADD", 4, 4, 16), I("MUL", 4, 4, 0), I("OUT", 0, 1, 4),
            I("SUB", 10, 10, 9), I("ADD", 10, 10, 12), I("SUB", 10, 10, 15), I("ADD", 10, 10, 17), I("MUL", 10, 10, 0), I("OUT", 0, 2, 10)]
    return "tanh", code, consts, _tanh.__doc__


BUILDERS = (_point, _uniform, _large, _tanh)
NAMES = tuple(f.__name__[1:] for f in BUILDERS)


def suite(dim, variant=0):
    """[(name, code int32[n, 4], consts float64[n_consts], description)]; ``variant`` 1 changes constants that are neither thresholds
    nor large arguments (among them the time of the hoisted sin(omega t))"""
    out = []
    for f in BUILDERS:
        name, code, consts, doc = f(dim, variant)
        out.append((name, np.array(code, dtype=np.int32).reshape(-1, 4), np.array(consts, dtype=np.float64), " ".join(doc.split())))
    return out


def tables(dim, variant=0):
    """name -> list of programs: every program as a single-program table and the mixed table of all of them"""
    s = suite(dim, variant)
    t = {e[0]: [e] for e in s}
    t["mixed"] = s
    return t


def n_regs(code):
    m = -1
    for op, d, a, b in code.tolist():
        nm = INV[op]
        m = max(m, *([b] if nm == "OUT" else [d] if nm in R.LOADS else [d, a] if nm in UNARY else [d, a, b]))
    return m + 1


def check_program(code, n_consts, dim):
    """validate_program (csrc/knp_kernels.hip) with the function block among the unary opcodes; the first offending instruction or None"""
    base = np.array([[ALL_OPS["NEG"] if INV.get(r[0]) in FUNCS else r[0]] + r[1:] for r in code.tolist()], dtype=np.int32).reshape(-1, 4)
    return R.check_program(base, n_consts, dim)


def uniform_trace(code):
    """per instruction: True where the run-time compiler computes it once per thread (emit_program, csrc/knp_jit.cpp: constant-only)"""
    base = np.array([[ALL_OPS["NEG"] if INV.get(r[0]) in FUNCS else r[0]] + r[1:] for r in code.tolist()], dtype=np.int32).reshape(-1, 4)
    kinds = R.uniform_trace(base)
    assert "overflow" not in kinds
    return [k == "slot" for k in kinds]


def probe(entry, i, reg, inp, dtype=np.longdouble):
    """value of register ``reg`` just before instruction ``i``"""
    code = np.array([r for r in entry[1][:i].tolist() if INV[r[0]] != "OUT"] + [list(I("OUT", 0, 0, reg))], dtype=np.int32).reshape(-1, 4)
    return R.run(entry, inp, dtype, code)[0]

