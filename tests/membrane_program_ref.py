"""Conformance suite of the membrane-program bytecode (``KNP_OP_*``, include/knpemi_hip.h): hand-written programs and their host
reference, shared by test_membrane_program_ref_host.py (no GPU) and test_gpu_membrane_programs.py.

The programs are written directly as bytecode -- not through ``fem.compile_program`` -- so that they control register numbers,
aliasing and instruction order.  The evaluator is ``fem.interpret_program`` (pinned on the host by test_host_logic.py) on arrays
of shape (n_g, n_q), in ``np.longdouble``.  Two observables come out of it:

* the right-hand side: an ``OracleKNPEMI`` whose ``channel_currents_q`` returns the suite's currents; the mechanism term alone is
  ``assemble_b()`` minus ``assemble_b()`` with all-zero currents;
* the diagnostic integral ``out[t] = sum_F sum_q qw[q] fmeas[F] (I0 + I1 + I2)(F, q)`` over the facets of group ``t``.

Every program multiplies its outputs by the constant ``S`` so that the mechanism term dominates every field block of ``b`` on the
membrane rows (the host test asserts it): an error of the mechanism currents is then an error of ``b`` of the same relative size.
A facet's program in a table of K programs is a function of the facet's vertex ids alone (``facet_programs``): the oracle and the
native problem number vertices identically (test_gpu_parity.py::test_layout_and_pattern), so both sides get the same map whatever
their facet order.
"""
from __future__ import annotations

import numpy as np

from parity_utils import make_oracle  # noqa: F401  (also puts the package and the oracle on sys.path)

from cgx_hip import fem
from cgx_hip._lib import KNP_DIAG_MAX_CONSTS, KNP_MAX_AUX, KNP_MAX_PROG_REGS, OPS

INV = {v: k for k, v in OPS.items()}
S = 1.0e6                                   # output scale, constant 0 of every program
MESHES = {2: ("square", 11), 3: ("cube", 7)}   # 20 facets (partial last block of 8) and 108 facets (partial last block of 16)
AUX_NAMES = ("m", "h", "n", "cs3", "cs4", "cs5", "cs6", "cs7")   # slots 0..2: the CI model's gating variables, 3..7: the suite's own
LOADS = ("CONST", "KI", "KE", "PHIM", "AUX", "X")
UNARY = ("NEG", "LN", "EXP", "SQRT", "ABS", "NOT", "MOV", "POWI")
COMPARES = ("LT", "GT", "LE", "GE")
# thresholds on the scaled coordinates (unit box): strictly inside a facet of both meshes (facets end at k/11 and k/7)
C_LO, C_HI, C_SUM = 0.437, 0.562, 1.013
# Membrane tag of a facet = its program id in the table of all programs; the diagnostic integrals are taken over these two groups of tags
GROUPS = ((0, 1, 2), (3, 4, 5, 6))


def I(name, d=0, a=0, b=0):
    return (OPS[name], d, a, b)


def _arith(dim, v):
    """every arithmetic opcode, KI/KE 0..2, PHIM, POWI -3/0/1/7, POW with a non-integer exponent, two OUTs to channel 0"""
    consts = [S * (1.5 if v else 1.0), 1000.0, 0.0125 if v else 0.01, 1.37]          # even count
    code = [I("CONST", 0, 0), I("KI", 1, 0), I("KE", 2, 0), I("KI", 3, 1), I("KE", 4, 1), I("KI", 5, 2), I("KE", 6, 2), I("PHIM", 7),
            I("DIV", 8, 2, 1), I("LN", 8, 8),                      # ln(ke0 / ki0) ~ 2.5, d == a
            I("CONST", 9, 1), I("MUL", 10, 7, 9), I("NEG", 10, 10),   # -1000 phi_m ~ 70
            I("CONST", 11, 2), I("MUL", 11, 10, 11),               # ~ 0.7, d == b
            I("EXP", 12, 11), I("SQRT", 13, 3),
            I("CONST", 14, 3), I("POW", 14, 4, 14),                # ke1 ^ 1.37
            I("SUB", 15, 5, 6), I("ADD", 15, 15, 8),
            I("POWI", 16, 4, -3), I("MUL", 16, 16, 9), I("POWI", 17, 1, 0), I("ADD", 16, 16, 17),
            I("POWI", 18, 12, 1), I("POWI", 19, 12, 7), I("ADD", 18, 18, 19),
            I("ADD", 20, 8, 12), I("ADD", 20, 20, 13), I("MUL", 20, 20, 0), I("OUT", 0, 0, 20),
            I("MUL", 14, 14, 0), I("OUT", 0, 0, 14),               # accumulates into channel 0
            I("SUB", 16, 16, 15), I("MUL", 16, 16, 0), I("OUT", 0, 1, 16),
            I("MUL", 18, 18, 0), I("OUT", 0, 2, 18)]
    return "arith", code, consts, _arith.__doc__


def _logic(dim, v):
    """comparisons, logic, SEL, MAX/MIN/ABS/MOV, EQ where the answer is exact, X on every axis, AUX 0 and 7, the guard pattern"""
    consts = [S * (0.5 if v else 1.0), 1.0e6, C_LO, C_HI, C_SUM, 2.0, 1000.0, 3000.0 if v else 1000.0, 10.0]   # odd count
    last = dim - 1
    code = [I("CONST", 0, 0), I("CONST", 1, 1),
            I("X", 2, 0), I("MUL", 2, 2, 1), I("X", 3, 1), I("MUL", 3, 3, 1), I("X", 4, last), I("MUL", 4, 4, 1),
            I("AUX", 5, 0), I("AUX", 6, KNP_MAX_AUX - 1),
            I("CONST", 7, 2), I("LT", 8, 2, 7),
            I("CONST", 9, 3), I("GT", 10, 3, 9),
            I("LE", 11, 4, 7),
            I("ADD", 12, 2, 3), I("CONST", 13, 4), I("GE", 14, 12, 13),
            I("AND", 15, 8, 10), I("OR", 16, 11, 14), I("NOT", 17, 16),
            I("EQ", 18, 2, 2),                                     # a register against itself: 1
            I("CONST", 19, 2), I("EQ", 19, 19, 7),                 # two loads of the same constant: 1
            I("KI", 20, 0), I("KE", 21, 0), I("EQ", 20, 20, 21),   # 0
            # equal operands, where LT/GT and LE/GE differ: a register against itself is exact
            I("LE", 33, 2, 2), I("GE", 34, 3, 3), I("LT", 35, 2, 2), I("GT", 36, 3, 3),
            # the flags as the binary digits of one number (Horner)
            I("CONST", 22, 5), I("MOV", 23, 8)]
    for r in (10, 11, 14, 15, 16, 17, 18, 19, 20, 33, 34, 35, 36):
        code += [I("MUL", 23, 23, 22), I("ADD", 23, 23, r)]
    code += [I("MUL", 23, 23, 0), I("OUT", 0, 0, 23),
             I("MAX", 24, 5, 6), I("MIN", 25, 5, 6), I("CONST", 26, 6), I("MUL", 24, 24, 26), I("MUL", 25, 25, 26),
             I("PHIM", 27), I("ABS", 27, 27), I("CONST", 28, 7), I("MUL", 27, 27, 28), I("ADD", 24, 24, 27),
             I("MUL", 24, 24, 0), I("OUT", 0, 1, 24),
             # guard: x0 > c ? ln(x0 - c) : x1, the untaken arm is NaN where x0 < c
             I("SUB", 29, 2, 7), I("LN", 29, 29), I("GT", 30, 2, 7), I("MOV", 31, 3), I("SEL", 31, 30, 29),
             I("CONST", 32, 8), I("MUL", 31, 31, 32), I("ADD", 25, 25, 31),
             I("MUL", 25, 25, 0), I("OUT", 0, 2, 25)]
    return "logic", code, consts, _logic.__doc__


def _regs48(dim, v):
    """register 47 (n_regs == 48), d == a == b, SEL with d == b, a value that stays live across more than 40 instructions"""
    consts = [S * (2.0 if v else 1.0), -12.0 if v else -10.0, C_LO * 1.0e-6]
    code = [I("KI", 47, 1), I("CONST", 46, 0), I("KE", 0, 0), I("PHIM", 1), I("CONST", 2, 1), I("MUL", 1, 1, 2)]
    for r in range(3, 44):                                         # a chain through registers 3..43
        code.append(I("ADD", r, r - 1 if r > 3 else 0, 1))
    code += [I("ADD", 43, 43, 43),                                 # d == a == b
             I("X", 44, 0), I("CONST", 45, 2), I("LT", 44, 44, 45),
             I("SEL", 43, 44, 43),                                 # d == b: leaves r43 as it is
             I("MOV", 42, 47), I("SEL", 42, 44, 43),
             I("MUL", 42, 42, 46), I("OUT", 0, 0, 42),
             I("MUL", 47, 47, 46), I("OUT", 0, 1, 47),            # loaded by the first instruction
             I("MUL", 43, 43, 46), I("OUT", 0, 2, 43)]
    return "regs48", code, consts, _regs48.__doc__


def _hoist(dim, v):
    """more than 16 constant-only instructions (the table U of knp_jit.cpp overflows; an overflowed result is an operand later),
    constant-only SELs, registers that change between hoisted, per-point and constant values, a DIV and an EXP among the hoisted"""
    consts = [S * (0.75 if v else 1.0), 2.0, 0.625 if v else 0.5, 3.0, 2.5 if v else 4.0, 0.25]   # even count
    code = [I("CONST", 0, 0), I("CONST", 1, 1), I("CONST", 2, 2), I("CONST", 3, 3),
            I("DIV", 4, 1, 3), I("EXP", 5, 2),                                            # slots 0, 1
            # hoisted -> per point -> constant
            I("ADD", 6, 4, 5), I("KI", 7, 0), I("MUL", 7, 7, 6), I("KE", 6, 1), I("MUL", 8, 6, 5), I("CONST", 6, 1), I("ADD", 9, 6, 2),
            # constant -> per point -> hoisted
            I("CONST", 10, 2), I("KI", 10, 1), I("MUL", 11, 10, 4), I("ADD", 10, 4, 9), I("MUL", 12, 10, 11),
            I("ADD", 7, 7, 8), I("ADD", 7, 7, 12),                                         # per point; 5 slots so far
            # constant-only SELs, one takes each arm
            I("GT", 20, 1, 2), I("MOV", 21, 4), I("SEL", 21, 20, 5),                        # slots 5, 6, 7: then-arm
            I("LT", 22, 1, 2), I("MOV", 23, 4), I("SEL", 23, 22, 5),                        # slots 8, 9, 10: else-arm
            I("MUL", 13, 9, 5), I("SUB", 14, 13, 4), I("NEG", 15, 14), I("ABS", 15, 15), I("SQRT", 16, 15),   # slots 11..15: the table is full
            I("POWI", 17, 16, 3),                                                          # overflow: per point
            I("MAX", 18, 17, 13), I("MIN", 19, 17, 13),                                    # an overflowed result as an operand
            I("ADD", 24, 18, 19), I("MUL", 25, 24, 21), I("ADD", 25, 25, 23),
            I("CONST", 26, 4), I("LN", 27, 26), I("MUL", 25, 25, 27),
            I("KE", 28, 2), I("MUL", 28, 28, 25), I("CONST", 29, 5), I("MUL", 28, 28, 29),
            I("MUL", 7, 7, 29), I("MUL", 7, 7, 0), I("OUT", 0, 0, 7),
            I("MUL", 28, 28, 0), I("OUT", 0, 1, 28),
            I("PHIM", 30), I("DIV", 30, 30, 25), I("CONST", 31, 3), I("POWI", 31, 31, 7), I("MUL", 30, 30, 31),
            I("MUL", 30, 30, 0), I("OUT", 0, 2, 30)]
    return "hoist", code, consts, _hoist.__doc__


def _c64(dim, v):
    """64 constants (KNP_DIAG_MAX_CONSTS), reads consts[63] and the constants around the middle and the end"""
    consts = [S] + [0.5 + 0.01 * k for k in range(1, KNP_DIAG_MAX_CONSTS)]
    consts[31], consts[32], consts[62], consts[63] = 7.5, 0.125, 0.25, (4.5 if v else 3.25)
    code = [I("KI", 0, 0), I("CONST", 1, 63), I("MUL", 2, 0, 1), I("CONST", 3, 0), I("MUL", 2, 2, 3), I("OUT", 0, 0, 2),
            I("CONST", 4, 31), I("KE", 5, 1), I("MUL", 5, 5, 4), I("MUL", 5, 5, 3), I("OUT", 0, 1, 5),
            I("CONST", 6, 62), I("CONST", 7, 32), I("ADD", 6, 6, 7), I("KE", 7, 2), I("MUL", 7, 7, 6), I("MUL", 7, 7, 3), I("OUT", 0, 2, 7)]
    return "c64", code, consts, _c64.__doc__


def _tiny(dim, v):
    """three registers, one constant (odd count), ten instructions"""
    consts = [S * (3.0 if v else 1.0)]
    code = [I("KI", 0, 1), I("CONST", 1, 0), I("MUL", 0, 0, 1), I("OUT", 0, 0, 0),
            I("KE", 2, 2), I("MUL", 2, 2, 1), I("OUT", 0, 1, 2), I("KE", 0, 0), I("MUL", 0, 0, 1), I("OUT", 0, 2, 0)]
    return "tiny", code, consts, _tiny.__doc__


def _nernst(dim, v):
    """Nernst-like currents of the three ions with the remaining auxiliary slots: 25 aux_k ln(ke_k / ki_k)"""
    consts = [S, 40.0 if v else 25.0]
    code = [I("CONST", 0, 0), I("CONST", 1, 1), I("MUL", 1, 1, 0)]
    for j in range(3):
        code += [I("KE", 2, j), I("KI", 3, j), I("DIV", 2, 2, 3), I("LN", 2, 2), I("AUX", 4, 3 + j), I("MUL", 2, 2, 4),
                 I("AUX", 5, 6 - j), I("ADD", 2, 2, 5), I("MUL", 2, 2, 1), I("OUT", 0, j, 2)]
    return "nernst", code, consts, _nernst.__doc__


BUILDERS = (_arith, _logic, _regs48, _hoist, _c64, _tiny, _nernst)
JIT_SINGLES = ("logic", "regs48", "hoist", "c64")     # single-program tables of the run-time compiled legs (one translation unit each)


def suite(dim, variant=0):
    """[(name, code int32[n, 4], consts float64[n_consts], description)]; ``variant`` 1 changes constants that are no thresholds
    (among them constants that feed hoisted instructions): the constants-refresh legs upload them into a live context."""
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


class _Spec(fem.ProgramSpec):
    """``ProgramSpec`` whose constants the evaluator reads in the working precision"""

    def __init__(self, code, consts, dtype=np.float64):
        super().__init__(code, list(consts), [])
        self.dtype = dtype

    def constants(self):
        return np.array(self.const_sources, dtype=self.dtype)


def spec_of(entry, dtype=np.float64):
    return _Spec(entry[1], [float(c) for c in entry[2]], dtype)


def n_regs(code):
    """register count as the library's validate_program computes it"""
    m = -1
    for op, d, a, b in code.tolist():
        nm = INV[op]
        regs = [b] if nm == "OUT" else [d] if nm in LOADS else [d, a] if nm in UNARY else [d, a, b]
        m = max(m, *regs)
    return m + 1


def check_program(code, n_consts, dim):
    """the rules of validate_program (csrc/knp_kernels.hip); returns the first offending instruction or None"""
    for i, (op, d, a, b) in enumerate(code.tolist()):
        nm = INV.get(op)
        reg = lambda r: 0 <= r < KNP_MAX_PROG_REGS
        if nm is None: ok = False
        elif nm == "CONST": ok = reg(d) and 0 <= a < n_consts
        elif nm in ("KI", "KE"): ok = reg(d) and 0 <= a < 3
        elif nm == "PHIM": ok = reg(d)
        elif nm == "AUX": ok = reg(d) and 0 <= a < KNP_MAX_AUX
        elif nm == "X": ok = reg(d) and 0 <= a < dim
        elif nm in UNARY: ok = reg(d) and reg(a)
        elif nm == "OUT": ok = 0 <= a < 3 and reg(b)
        else: ok = reg(d) and reg(a) and reg(b)
        if not ok:
            return i
    return None


def uniform_trace(code, table=16):
    """The hoisting rule of emit_program (csrc/knp_jit.cpp) again: per instruction 'slot' (constant-only, computed once per thread),
    'overflow' (constant-only, but the table is full: computed per point, its result counts as per-point) or None."""
    uni, n, kinds = {}, 0, []
    for op, d, a, b in code.tolist():
        nm = INV[op]
        kind = None
        if nm == "OUT":
            kinds.append(None)
            continue
        if nm == "CONST": u = True
        elif nm in LOADS: u = False
        else:
            src = [a] if nm in UNARY else [a, b, d] if nm == "SEL" else [a, b]
            u = all(uni.get(s, False) for s in src)
            if u:
                if n < table: n, kind = n + 1, "slot"
                else: u, kind = False, "overflow"
        uni[d] = u
        kinds.append(kind)
    return kinds


# ------------------------------------------------------------------------------------------ fields
def fill_fields(o):
    """Smooth non-uniform nodal fields on the oracle (every value differs from quadrature point to quadrature point); the suite's
    own auxiliary fields go to ``o.cs_aux`` (slots 3..7)."""
    X = o.coords / o.coords.max()
    z = X[:, 2] if o.dim == 3 else 0.0 * X[:, 0]
    s = 1.0 + 0.2 * np.sin(3.0 * X[:, 0] + 1.0) * np.cos(2.0 * X[:, 1] + 0.5) * np.cos(1.5 * z + 0.2)
    for side in range(2):
        for j in range(3):
            o.k[side][j] = o.k[side][j] * (s if (side + j) % 2 == 0 else 2.0 - s)
    o.phi_m = o.phi_m * (2.0 - s)
    for name in ("n", "m", "h"):
        setattr(o, name, getattr(o, name) * s)
    o.cs_aux = [0.3 + 0.2 * np.sin(k + 2.0 * X[:, 0] + 3.0 * X[:, 1] + z) for k in range(3, KNP_MAX_AUX - 1)]
    o.cs_aux.append(0.04 + 0.03 * np.sin(7.0 + 2.0 * X[:, 0] + 3.0 * X[:, 1] + z))       # crosses aux 0 (m ~ 0.04)
    return o


def aux_nodal(o):
    return [getattr(o, nm) if len(nm) == 1 else o.cs_aux[int(nm[2:]) - 3] for nm in AUX_NAMES]


def copy_fields_to_problem(o, p):
    """the oracle's fields on the native problem; appends the suite's auxiliary functions (before the first ``be.fields()`` call)"""
    import torch
    dev = p.mesh.device
    assert [f.name for f in p.aux_functions] == list(AUX_NAMES[:3]), [f.name for f in p.aux_functions]
    for side in range(2):
        for j in range(3):
            p.wh[side][j].x.array[:] = torch.as_tensor(o.k[side][j], device=dev)
    p.phi_m_prev.x.array[:] = torch.as_tensor(o.phi_m, device=dev)
    for name in ("n", "m", "h"):
        getattr(p, name).x.array[:] = torch.as_tensor(getattr(o, name), device=dev)
    for nm in AUX_NAMES[3:]:
        f = fem.Function(p.V, nm)
        f.x.array[:] = torch.as_tensor(o.cs_aux[int(nm[2:]) - 3], device=dev)
        p.aux_functions.append(f)


def point_inputs(o, dtype=np.longdouble):
    """the programs' inputs at the quadrature points, (n_g, n_q) each"""
    at = lambda nodal: nodal[o.fv].astype(dtype) @ o.lamq.T.astype(dtype)
    return {"ki": [at(o.k[0][j]) for j in range(3)], "ke": [at(o.k[1][j]) for j in range(3)], "phim": at(o.phi_m),
            "aux": [at(a) for a in aux_nodal(o)], "xq": [at(o.coords[:, d]) for d in range(o.dim)] + [None] * (3 - o.dim)}


def run(entry, inp, dtype=np.longdouble, code=None):
    spec = spec_of(entry, dtype)
    if code is not None:
        spec.code = code
    with np.errstate(invalid="ignore", divide="ignore"):
        out = fem.interpret_program(spec, inp["ki"], inp["ke"], inp["phim"], inp["aux"], inp["xq"])
    return [np.broadcast_to(np.asarray(x, dtype=dtype), inp["phim"].shape) for x in out]


def probe(entry, i, reg, inp, dtype=np.longdouble):
    """value of register ``reg`` just before instruction ``i``"""
    code = np.array([r for r in entry[1][:i].tolist() if INV[r[0]] != "OUT"] + [list(I("OUT", 0, 0, reg))], dtype=np.int32).reshape(-1, 4)
    return run(entry, inp, dtype, code)[0]


def facet_programs(fv, n_programs):
    """Program of every facet in a table of ``n_programs``: a sum over the facet's vertex ids (so it depends neither on the facet
    order nor on the vertex order inside a facet) of a multiplicative hash of the id -- the plain sum of the ids is periodic on the
    structured meshes and leaves whole blocks with one program."""
    v = np.asarray(fv, dtype=np.int64)
    return ((((v * 2654435761) & 0xFFFFFFFF) >> 16).sum(axis=1) % n_programs).astype(np.int32)


def currents(o, table, dtype=np.longdouble, inp=None):
    """(3, n_g, n_q) float64: every facet's currents from its program of ``table``"""
    inp = inp if inp is not None else point_inputs(o, dtype)
    prog = facet_programs(o.fv, len(table))
    out = np.zeros((3,) + inp["phim"].shape, dtype=dtype)
    for pid, entry in enumerate(table):
        cur = run(entry, inp, dtype)
        for j in range(3):
            out[j][prog == pid] = cur[j][prog == pid]
    return out.astype(np.float64)


def rhs_reference(o, Iq):
    """(b, mechanism term of b, rows of the membrane vertices)"""
    saved = o.channel_currents_q
    try:
        o.channel_currents_q = lambda: Iq
        b = o.assemble_b()
        o.channel_currents_q = lambda: np.zeros_like(Iq)
        b0 = o.assemble_b()
    finally:
        o.channel_currents_q = saved
    rows = np.unique(np.concatenate([o.fnode_i.ravel(), o.fnode_e.ravel()]))
    return b, b - b0, rows


def integral_reference(o, Iq, group_of_facet, n_groups):
    """(out[t], sum of |terms| of group t)"""
    terms = o.qw[None, :] * o.fmeas[:, None] * Iq.sum(axis=0)
    out = np.array([terms[group_of_facet == t].sum() for t in range(n_groups)])
    mag = np.array([np.abs(terms[group_of_facet == t]).sum() for t in range(n_groups)])
    return out, mag


def block_errors(b, b_ref, mech):
    """per field block: max |b - b_ref| over all rows, relative to the largest mechanism term of the block"""
    return [float(np.max(np.abs(b[f::4] - b_ref[f::4])) / np.max(np.abs(mech[f::4]))) for f in range(4)]
