"""Light array-backed stand-ins for the DOLFINx / UFL objects that the reference's problem and
membrane-mechanism code manipulates (dfx.fem.Function, dfx.fem.Constant, UFL expressions), plus the
compiler that turns a mechanism's ``_eval`` expression into the register bytecode interpreted by
the HIP membrane kernel (include/knpemi_hip.h, KNP_OP_*).

Replaces: UFL expression building + FFCx JIT of the Gamma integrands
(reference src/CGx/KNPEMI/KNPEMIx_problem.py:504-555,609-610,641-642, 654-655).

Semantics kept from UFL on purpose:
  * ``bool(expr)`` is True for every expression (UFL ``Expr.__bool__``) -- this is what makes the
    reference's ``IonicModel.f_NKCC1`` return zero (KNPEMIx_ionic_model.py:62-69).
  * ``expr('+')`` / ``expr('-')`` restrictions are accepted and are no-ops: all coefficients are
    continuous P1 fields, only facet-vertex values enter a Gamma integral.  The exceptions are the nodes that have two
    values on a membrane facet -- ``Derivative``, ``NormalComponent``, ``NormalDerivative`` -- which keep the side for the
    integrands of membrane functionals (cgx_hip/functionals.py).
"""
from __future__ import annotations

import math
import numbers

import numpy as np
import torch

from ._lib import ALL_OPS, FUNC_OPS, KNP_MAX_AUX, KNP_MAX_PROG_REGS, OPS  # noqa: F401  (OPS: the base opcode table, part of this module's interface)


# ------------------------------------------------------------------------------------------
# expressions
# ------------------------------------------------------------------------------------------
class Expr:
    __array_priority__ = 1000          # make numpy scalars defer to our operators

    def _bin(self, op, other, swap=False):
        other = as_expr(other)
        return Op(op, (other, self) if swap else (self, other))

    def __add__(self, o): return self._bin("ADD", o)
    def __radd__(self, o): return self._bin("ADD", o, True)
    def __sub__(self, o): return self._bin("SUB", o)
    def __rsub__(self, o): return self._bin("SUB", o, True)
    def __mul__(self, o): return self._bin("MUL", o)
    def __rmul__(self, o): return self._bin("MUL", o, True)
    def __truediv__(self, o): return self._bin("DIV", o)
    def __rtruediv__(self, o): return self._bin("DIV", o, True)
    def __neg__(self): return Op("NEG", (self,))
    def __pos__(self): return self
    def __abs__(self): return Op("ABS", (self,))

    def __pow__(self, e):
        if isinstance(e, numbers.Integral) and not isinstance(e, bool) and abs(int(e)) <= 64:
            return Op("POWI", (self,), int(e))
        return Op("POW", (self, as_expr(e)))

    def __rpow__(self, base):
        return Op("POW", (as_expr(base), self))

    def __bool__(self):                 # UFL: every Expr is truthy
        return True

    def __call__(self, restriction=None):
        return self


class Literal(Expr):
    def __init__(self, value):
        self.value = float(value)


class Constant(Expr):
    """dfx.fem.Constant stand-in: a mutable scalar (``.value``)."""

    def __init__(self, mesh, value):
        self.mesh = mesh
        self._value = float(np.asarray(value))

    @property
    def value(self):
        return self._value

    @value.setter
    def value(self, v):
        self._value = float(np.asarray(v))

    def __float__(self):
        return self._value

    def __repr__(self):
        return f"Constant({self._value})"


class _Vector:
    """``function.x``: owns the nodal array (a torch tensor on the problem's device)."""

    def __init__(self, n, device):
        self.array = torch.zeros(n, dtype=torch.float64, device=device)

    def scatter_forward(self):          # ghosts are refreshed by the library's halo hook
        return None

    @property
    def petsc_vec(self):
        raise AttributeError("no PETSc in the MI355X-native path; use .array")


class FunctionSpace:
    def __init__(self, mesh, name="P1"):
        self.mesh = mesh
        self.name = name
        self.num_dofs = mesh.num_vertices

    def clone(self):
        return FunctionSpace(self.mesh, self.name)


class Function(Expr):
    """dfx.fem.Function stand-in for a P1 nodal field (one value per mesh vertex)."""

    def __init__(self, V, name="f"):
        self.function_space = V
        self.name = name
        self.x = _Vector(V.mesh.num_vertices, V.mesh.device)

    def numpy(self):
        return self.x.array.detach().cpu().numpy()

    def data_ptr(self):
        return self.x.array.data_ptr()


class Coordinate(Expr):
    def __init__(self, axis):
        self.axis = int(axis)


class Op(Expr):
    def __init__(self, op, args, imm=0):
        self.op, self.args, self.imm = op, tuple(args), imm


def _restriction(r):
    if r not in ("+", "-"):
        raise ValueError(f"a restriction is '+' (the intracellular cell of the facet) or '-' (the extracellular one), not {r!r}")
    return r


class Derivative(Expr):
    """d/dx_axis of a P1 ``Function``: constant on every cell.  The integrands of volume functionals may hold one
    (cgx_hip/functionals.py), and so may those of membrane functionals: on a membrane facet the two adjacent cells give two
    values, and ``d('+')`` / ``d('-')`` is the restricted copy that takes the one of the intracellular / extracellular cell (UFL's
    restriction; ``side`` None: unrestricted).  A volume functional ignores the restriction.  Membrane and state programs are
    evaluated at vertices, where a derivative has no value at all, and refuse it."""

    def __init__(self, function, axis, side=None):
        if not isinstance(function, Function):
            raise TypeError("grad() takes a Function (a P1 nodal field)")
        self.function, self.axis, self.side = function, int(axis), side

    def __call__(self, restriction=None):
        return self if restriction is None else Derivative(self.function, self.axis, _restriction(restriction))


class NormalComponent(Expr):
    """Component ``axis`` of the unit normal of a membrane facet (``FacetNormal``): ``n[a]('+')`` points out of the intracellular
    cell, ``n[a]('-')`` is its negative.  Only membrane functionals take it, and only restricted."""

    def __init__(self, axis, side=None):
        self.axis, self.side = int(axis), side

    def __call__(self, restriction=None):
        return self if restriction is None else NormalComponent(self.axis, _restriction(restriction))


class NormalDerivative(Expr):
    """d f / d n_side of a P1 ``Function`` on a membrane facet: the gradient on that side's cell times that side's outward normal.
    One aux slot of a membrane functional, where ``inner(grad(f)(side), n(side))`` takes ``dim`` slots for the gradient and
    ``dim`` for the normal.  ``side`` None: the function's own side (a solution function of the problem)."""

    def __init__(self, function, side=None):
        if not isinstance(function, Function):
            raise TypeError("NormalDerivative() takes a Function (a P1 nodal field)")
        self.function, self.side = function, None if side is None else _restriction(side)

    def __call__(self, restriction=None):
        return self if restriction is None else NormalDerivative(self.function, restriction)


def as_expr(v):
    if isinstance(v, Expr):
        return v
    if isinstance(v, (numbers.Real, np.floating, np.integer)):
        return Literal(float(v))
    if isinstance(v, np.ndarray) and v.ndim == 0:
        return Literal(float(v))
    raise TypeError(f"cannot use {type(v)} in a membrane expression")


# UFL-named helpers (what mechanism code imports as ``ufl.<name>``)
def ln(x): return Op("LN", (as_expr(x),))
def exp(x): return Op("EXP", (as_expr(x),))
def sqrt(x): return Op("SQRT", (as_expr(x),))
def sin(x): return Op("SIN", (as_expr(x),))
def cos(x): return Op("COS", (as_expr(x),))
def tanh(x): return Op("TANH", (as_expr(x),))
def max_value(a, b): return Op("MAX", (as_expr(a), as_expr(b)))
def min_value(a, b): return Op("MIN", (as_expr(a), as_expr(b)))
def lt(a, b): return Op("LT", (as_expr(a), as_expr(b)))
def gt(a, b): return Op("GT", (as_expr(a), as_expr(b)))
def le(a, b): return Op("LE", (as_expr(a), as_expr(b)))
def ge(a, b): return Op("GE", (as_expr(a), as_expr(b)))
def eq(a, b): return Op("EQ", (as_expr(a), as_expr(b)))
def And(a, b): return Op("AND", (as_expr(a), as_expr(b)))
def Or(a, b): return Op("OR", (as_expr(a), as_expr(b)))
def Not(a): return Op("NOT", (as_expr(a),))
def conditional(c, t, f): return Op("SEL", (as_expr(c), as_expr(t), as_expr(f)))
def SpatialCoordinate(mesh): return [Coordinate(d) for d in range(mesh.geometry.dim)]


def grad(f):
    """``ufl.grad`` of a P1 Function: the list of its ``dim`` partial derivatives"""
    if not isinstance(f, Function):
        raise TypeError("grad() takes a Function (a P1 nodal field)")
    return [Derivative(f, a) for a in range(f.function_space.mesh.geometry.dim)]


def inner(a, b):
    """``ufl.inner`` of two scalars, or of two lists of equally many components (``grad``)"""
    va, vb = isinstance(a, (list, tuple)), isinstance(b, (list, tuple))
    if va != vb or (va and (len(a) != len(b) or not len(a))):
        raise ValueError("inner() takes two scalars or two lists of the same length")
    if not va:
        return as_expr(a) * as_expr(b)
    total = as_expr(a[0]) * as_expr(b[0])
    for x, y in zip(a[1:], b[1:]):
        total = total + as_expr(x) * as_expr(y)
    return total


def FacetNormal(mesh):
    """``ufl.FacetNormal``: the list of the ``dim`` components of a membrane facet's unit normal, to be restricted"""
    return [NormalComponent(a) for a in range(mesh.geometry.dim)]


def dot(a, b):
    """``ufl.dot``: ``inner`` for two scalars or two lists -- and where one list is ``grad(f)`` restricted to r (all components, axes in
    order) and the other the facet normal restricted to r', the single node +-``NormalDerivative(f, r)``, + for r == r'"""
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b) and len(a):
        for g, n in ((a, b), (b, a)):
            if (all(isinstance(x, Derivative) for x in g) and all(isinstance(x, NormalComponent) for x in n)
                    and all(x.function is g[0].function and x.side == g[0].side and x.axis == k for k, x in enumerate(g))
                    and all(x.side == n[0].side and x.axis == k for k, x in enumerate(n))
                    and g[0].side is not None and n[0].side is not None
                    and len(g) == g[0].function.function_space.mesh.geometry.dim):
                d = NormalDerivative(g[0].function, g[0].side)
                return d if g[0].side == n[0].side else -d
    return inner(a, b)


pi = math.pi
max = max_value      # noqa: A001  (the reference spells it ufl.max / ufl.min)
min = min_value      # noqa: A001


class ZeroBaseForm(Expr):
    """``ufl.ZeroBaseForm(None)``: additive identity used to start sums."""

    def __init__(self, *_):
        pass

    def __add__(self, o): return as_expr(o)
    def __radd__(self, o): return as_expr(o)


# ------------------------------------------------------------------------------------------
# compilation to bytecode
# ------------------------------------------------------------------------------------------
class ProgramSpec:
    """Compiled membrane program: ``code`` int32[n,4], constant table and the Python objects
    behind the table (so that time-dependent Constants can be refreshed every step)."""

    def __init__(self, code, const_sources, aux_functions, aux_derivs=None):
        self.code = code
        self.const_sources = const_sources      # list of Constant | float
        self.aux_functions = aux_functions      # list of Function, index = aux slot
        self.aux_derivs = aux_derivs            # None, or per aux slot -1 (the Function's value) | axis (its derivative)

    def constants(self):
        return np.array([float(c.value) if isinstance(c, Constant) else float(c) for c in self.const_sources],
                        dtype=np.float64)


class AuxSlotsExhausted(ValueError):
    """the expressions of one program read more than KNP_MAX_AUX nodal fields (and derivatives) that need an aux slot"""


# aux_derivs codes of a membrane functional besides -1 and the axes 0..2 (there: on the intracellular cell of the facet)
MODE_GRAD_E, MODE_DN_I, MODE_NORMAL = 3, 6, 8


def compile_program(outputs, field_roles, aux_functions=None, aux_derivs=None, facet_sides=None):
    """outputs: list of 3 expressions (I_ch^k).  field_roles: dict id(Function) -> ('KI', j) |
    ('KE', j) | ('PHIM', 0).  Other Functions get aux slots (shared list ``aux_functions``).
    ``aux_derivs``: a list that runs parallel to ``aux_functions`` (-1: the slot holds the Function's value, a: its derivative
    d/dx_a) lets the expressions hold ``Derivative`` nodes: each (Function, axis) pair takes one slot.  Without it a
    ``Derivative`` is refused, as in every membrane and state program.
    ``facet_sides`` (with ``aux_derivs``): dict id(Function) -> 0 | 1, the side a solution function lives on, asks for the programs
    of membrane functionals.  The codes of ``aux_derivs`` are then a + 3 s for d/dx_a on the cell of side s (0 intracellular '+',
    1 extracellular '-'), 6 + s for ``NormalDerivative`` on side s, 8 + a for component a of the intracellular outward normal
    (such a slot has no Function: None in ``aux_functions``; ``n[a]('-')`` negates it).  A function listed in ``facet_sides``
    defaults to its side and refuses the other; anything else must be restricted.  Without ``facet_sides`` a restriction on a
    ``Derivative`` is ignored and normals and normal derivatives are a ValueError."""
    aux_functions = aux_functions if aux_functions is not None else []
    if aux_derivs is not None and len(aux_derivs) != len(aux_functions):
        raise ValueError("aux_derivs must have one entry per aux function")

    def aux_slot(f, axis):
        for k, g in enumerate(aux_functions):
            if g is f and (aux_derivs is None or aux_derivs[k] == axis):
                return k
        if len(aux_functions) >= KNP_MAX_AUX:
            raise AuxSlotsExhausted(f"more than {KNP_MAX_AUX} auxiliary nodal fields in membrane expressions")
        aux_functions.append(f)
        if aux_derivs is not None:
            aux_derivs.append(axis)
        return len(aux_functions) - 1

    def side_of(e):
        """0 | 1: the cell of the facet a derivative node of a membrane functional is taken on"""
        own = facet_sides.get(id(e.function))
        if e.side is None:
            if own is None:
                raise ValueError(f"a derivative of '{e.function.name}' on a membrane facet must be restricted, ('+') for the "
                                 "intracellular cell or ('-') for the extracellular one: only the solution functions have a side of their own")
            return own
        s = 0 if e.side == "+" else 1
        if own is not None and own != s:
            raise ValueError(f"'{e.function.name}' lives on the {'intra' if own == 0 else 'extra'}cellular side: its derivative "
                             f"cannot be restricted to ('{e.side}')")
        return s
    nodes = []                # SSA list: (opname, argidx tuple, imm)
    index = {}                # structural key -> ssa id
    consts = []
    const_index = {}

    def const_slot(src):
        key = ("C", id(src)) if isinstance(src, Constant) else ("L", float(src))
        if key not in const_index:
            const_index[key] = len(consts)
            consts.append(src)
        return const_index[key]

    def emit(key, rec):
        if key in index:
            return index[key]
        nodes.append(rec)
        index[key] = len(nodes) - 1
        return index[key]

    def visit(e):
        e = as_expr(e)
        if isinstance(e, ZeroBaseForm):
            s = const_slot(0.0)
            return emit(("CONST", s), ("CONST", (), s))
        if isinstance(e, Literal):
            s = const_slot(e.value)
            return emit(("CONST", s), ("CONST", (), s))
        if isinstance(e, Constant):
            s = const_slot(e)
            return emit(("CONST", s), ("CONST", (), s))
        if isinstance(e, Coordinate):
            return emit(("X", e.axis), ("X", (), e.axis))
        if isinstance(e, Function):
            role = field_roles.get(id(e))
            if role is None:
                role = ("AUX", aux_slot(e, -1))
            return emit(role, (role[0], (), role[1]))
        if isinstance(e, Derivative) and aux_derivs is not None:
            role = ("AUX", aux_slot(e.function, e.axis + (MODE_GRAD_E * side_of(e) if facet_sides is not None else 0)))
            return emit(role, (role[0], (), role[1]))
        if isinstance(e, (NormalDerivative, NormalComponent)) and aux_derivs is not None:
            if facet_sides is None:
                raise ValueError("a facet normal or a normal derivative has a value on membrane facets only: "
                                 "volume functionals, membrane and state programs do not take it")
            if isinstance(e, NormalDerivative):
                role = ("AUX", aux_slot(e.function, MODE_DN_I + side_of(e)))
                return emit(role, (role[0], (), role[1]))
            if e.side is None:
                raise ValueError("the facet normal must be restricted: n[a]('+') points out of the intracellular cell, n[a]('-') out "
                                 "of the extracellular one")
            role = ("AUX", aux_slot(None, MODE_NORMAL + e.axis))
            n = emit(role, (role[0], (), role[1]))
            return n if e.side == "+" else emit(("NEG", (n,), 0), ("NEG", (n,), 0))
        if isinstance(e, Op):
            args = tuple(visit(a) for a in e.args)
            return emit((e.op, args, e.imm), (e.op, args, e.imm))
        raise TypeError(type(e))

    out_ids = [visit(o) for o in outputs]

    # liveness + linear-scan register allocation
    last_use = [-1] * len(nodes)
    for i, (_, args, _) in enumerate(nodes):
        for a in args:
            last_use[a] = i
    for oid in out_ids:
        last_use[oid] = len(nodes) + 1
    free = list(range(KNP_MAX_PROG_REGS - 1, -1, -1))
    reg = [-1] * len(nodes)
    code = []
    for i, (op, args, imm) in enumerate(nodes):
        # registers of operands whose last use is this instruction can be reused for the result,
        # except for SEL whose destination must not alias its operands before the MOV
        releasable = [a for a in set(args) if last_use[a] == i]
        if op != "SEL":
            for a in releasable:
                free.append(reg[a])
        if not free:
            raise ValueError(f"membrane expression needs more than {KNP_MAX_PROG_REGS} registers")
        r = free.pop()
        reg[i] = r
        if op in ("CONST", "KI", "KE", "AUX", "X"):
            code.append((ALL_OPS[op], r, imm, 0))
        elif op == "PHIM":
            code.append((ALL_OPS[op], r, 0, 0))
        elif op == "POWI":
            code.append((ALL_OPS[op], r, reg[args[0]], imm))
        elif op == "SEL":
            c, t, f = args
            code.append((ALL_OPS["MOV"], r, reg[f], 0))
            code.append((ALL_OPS["SEL"], r, reg[c], reg[t]))
            for a in releasable:
                free.append(reg[a])
        elif len(args) == 1:
            code.append((ALL_OPS[op], r, reg[args[0]], 0))
        else:
            code.append((ALL_OPS[op], r, reg[args[0]], reg[args[1]]))
        if last_use[i] == -1:          # dead value
            free.append(r)
    for k, oid in enumerate(out_ids):
        code.append((ALL_OPS["OUT"], 0, k, reg[oid]))
    return ProgramSpec(np.array(code, dtype=np.int32).reshape(-1, 4), consts, aux_functions, aux_derivs)


# ------------------------------------------------------------------------------------------
# state variables of membrane mechanisms (IonicModel.add_state)
# ------------------------------------------------------------------------------------------
RESERVED_STATE_NAMES = frozenset({"t", "step", "l2g", "coords", "phi_m"})      # keys of a checkpoint besides the solution functions


class StateVariable:
    """A nodal state that a membrane mechanism declares and the library advances after every solve (knp_state_update).
    ``kind`` 0: a gate dy/dt = alpha (1 - y) - beta y, ``exprs`` = (alpha, beta); ``kind`` 1: dy/dt = rhs, ``exprs`` = (rhs,).
    ``spec`` / ``aux_index``: the compiled program and the aux slot of ``function``, set by ``compile_state_program``."""

    def __init__(self, name, function, kind, build, model):
        self.name, self.function, self.kind, self.model = name, function, kind, model
        self._build, self._exprs = build, None
        self.spec = None
        self.aux_index = None

    @property
    def exprs(self):
        """built at the first use -- the compilation, after every model's ``_init()`` -- so that callables may name any state"""
        if self._exprs is None:
            self._exprs = tuple(self._build())
        return self._exprs


def declare_state(model, name, init, alpha=None, beta=None, inf=None, tau=None, rhs=None):
    """What ``IonicModel.add_state`` of both model families does: one of the forms (alpha, beta), (inf, tau) or rhs; the
    Function lives on the problem's space ``V`` and starts from ``init`` (a number or nodal values).  Each expression may be a
    callable ``y -> expression`` of the state's own Function instead.  It is called when the programs are compiled, so it may also
    name states that are declared later: that is how a state reads itself or two states read each other."""
    forms = {"alpha/beta": (alpha, beta), "inf/tau": (inf, tau), "rhs": (rhs,)}
    begun = [k for k, v in forms.items() if any(x is not None for x in v)]
    whole = [k for k, v in forms.items() if all(x is not None for x in v)]
    if len(begun) != 1 or begun != whole:
        raise ValueError(f"state '{name}': give exactly one of alpha= and beta=, inf= and tau=, or rhs= "
                         f"(got {', '.join(begun) if begun else 'none'}{'' if begun == whole else ', incomplete'})")
    p = model.problem
    taken = RESERVED_STATE_NAMES | {g.name for side in getattr(p, "wh", []) for g in (side if isinstance(side, (list, tuple)) else [side])}
    if str(name) in taken:
        raise ValueError(f"state '{name}': the name is a key of the checkpoints already ({', '.join(sorted(taken))})")
    f = Function(p.V, str(name))
    vals = np.broadcast_to(np.asarray(init, dtype=np.float64), (f.x.array.numel(),))
    f.x.array[:] = torch.as_tensor(vals.copy(), device=f.x.array.device)
    ex = lambda e: as_expr(e(f) if callable(e) and not isinstance(e, Expr) else e)
    if whole[0] == "alpha/beta":
        kind, build = 0, lambda: (ex(alpha), ex(beta))
    elif whole[0] == "inf/tau":      # the same gate: alpha = inf / tau, beta = (1 - inf) / tau; each expression built once
        def build():
            i, t = ex(inf), ex(tau)
            return i / t, (1.0 - i) / t
        kind = 0
    else:
        kind, build = 1, lambda: (ex(rhs),)
    st = StateVariable(str(name), f, kind, build, model)
    states = model.__dict__.setdefault("states", [])
    states[:] = [s for s in states if s.name != st.name] + [st]       # a second _init() declares anew
    return st


def collect_states(models):
    """The states of ``models`` in declaration order and the (use_Rush_Larsen, time_steps_ODE) their models agree on"""
    states, owners = [], []
    if sum(len(getattr(m, "states", [])) for m in models) > KNP_MAX_AUX:      # every state takes an aux slot
        raise ValueError(f"more than {KNP_MAX_AUX} auxiliary nodal fields in membrane expressions")
    for m in models:
        for st in getattr(m, "states", []):
            if any(st.name == o.name for o in states):
                raise ValueError(f"state '{st.name}' is declared twice")
            states.append(st)
            if m not in owners:
                owners.append(m)
    settings = {(bool(getattr(m, "use_Rush_Larsen", True)), int(getattr(m, "time_steps_ODE", 25))) for m in owners}
    if len(settings) > 1:
        raise ValueError("the models that declare states disagree on use_Rush_Larsen / time_steps_ODE: "
                         + ", ".join(f"{m}: {bool(getattr(m, 'use_Rush_Larsen', True))} / {int(getattr(m, 'time_steps_ODE', 25))}" for m in owners))
    rl, sub = settings.pop() if settings else (True, 25)
    if sub < 1:
        raise ValueError("time_steps_ODE must be at least 1")
    return states, rl, sub


def compile_state_program(state, field_roles, aux_functions):
    """One program per state through ``compile_program``: a gate writes KNP_OP_OUT 0 = alpha and KNP_OP_OUT 1 = beta, a general
    state KNP_OP_OUT 0 = dy/dt.  The state's Function takes (or already has) a slot of the shared list ``aux_functions``."""
    if not any(f is state.function for f in aux_functions):
        if len(aux_functions) >= KNP_MAX_AUX:
            raise ValueError(f"more than {KNP_MAX_AUX} auxiliary nodal fields in membrane expressions")
        aux_functions.append(state.function)
    state.aux_index = next(k for k, f in enumerate(aux_functions) if f is state.function)
    state.spec = compile_program(list(state.exprs), field_roles, aux_functions)
    return state.spec


# ------------------------------------------------------------------------------------------
# host evaluation (setup-time scalars such as the stimulus area; never on the timed path)
# ------------------------------------------------------------------------------------------
def evaluate_numpy(e, env):
    """Evaluate an expression with NumPy. env: {'x': [arrays per axis], 'fields': {id(Function): array}} and, for expressions
    with derivatives, 'grads': {(id(Function), axis): array}.  On membrane facets: 'grads' may also hold (id, axis, '+' | '-') for a
    restricted derivative (it falls back to the unrestricted key), 'normal_derivs': {(id(Function), '+' | '-' | None): array} and
    'normal': [arrays per axis], the intracellular outward normal n('+')."""
    e = as_expr(e)
    if isinstance(e, (Literal,)):
        return e.value
    if isinstance(e, ZeroBaseForm):
        return 0.0
    if isinstance(e, Constant):
        return e.value
    if isinstance(e, Coordinate):
        return env["x"][e.axis]
    if isinstance(e, Function):
        return env["fields"][id(e)]
    if isinstance(e, Derivative):
        key = (id(e.function), e.axis, e.side)
        return env["grads"][key if e.side is not None and key in env["grads"] else key[:2]]
    if isinstance(e, NormalDerivative):
        return env["normal_derivs"][(id(e.function), e.side)]
    if isinstance(e, NormalComponent):
        if e.side is None:
            raise ValueError("the facet normal must be restricted")
        return env["normal"][e.axis] if e.side == "+" else -env["normal"][e.axis]
    a = [evaluate_numpy(x, env) for x in e.args]
    op = e.op
    if op == "ADD": return a[0] + a[1]
    if op == "SUB": return a[0] - a[1]
    if op == "MUL": return a[0] * a[1]
    if op == "DIV": return a[0] / a[1]
    if op == "NEG": return -a[0]
    if op == "ABS": return np.abs(a[0])
    if op == "POW": return np.power(a[0], a[1])
    if op == "POWI": return np.power(a[0], e.imm)
    if op == "LN": return np.log(a[0])
    if op == "EXP": return np.exp(a[0])
    if op == "SQRT": return np.sqrt(a[0])
    if op == "SIN": return np.sin(a[0])
    if op == "COS": return np.cos(a[0])
    if op == "TANH": return np.tanh(a[0])
    if op == "MAX": return np.maximum(a[0], a[1])
    if op == "MIN": return np.minimum(a[0], a[1])
    if op == "LT": return (a[0] < a[1]) * 1.0
    if op == "GT": return (a[0] > a[1]) * 1.0
    if op == "LE": return (a[0] <= a[1]) * 1.0
    if op == "GE": return (a[0] >= a[1]) * 1.0
    if op == "EQ": return (a[0] == a[1]) * 1.0
    if op == "AND": return ((np.asarray(a[0]) != 0) & (np.asarray(a[1]) != 0)) * 1.0
    if op == "OR": return ((np.asarray(a[0]) != 0) | (np.asarray(a[1]) != 0)) * 1.0
    if op == "NOT": return (np.asarray(a[0]) == 0) * 1.0
    if op == "SEL": return np.where(np.asarray(a[0]) != 0, a[1], a[2])
    raise ValueError(op)


def interpret_program(spec: ProgramSpec, ki, ke, phim, aux, xq):
    """Pure-Python interpreter of the bytecode (host logic test of the compiler; scalars or arrays)."""
    consts = spec.constants()
    reg = [0.0] * KNP_MAX_PROG_REGS
    out = [0.0, 0.0, 0.0]
    inv = {v: k for k, v in ALL_OPS.items()}
    for op, d, a, b in spec.code.tolist():
        name = inv[op]
        if name == "CONST": reg[d] = consts[a]
        elif name == "KI": reg[d] = ki[a]
        elif name == "KE": reg[d] = ke[a]
        elif name == "PHIM": reg[d] = phim
        elif name == "AUX": reg[d] = aux[a]
        elif name == "X": reg[d] = xq[a]
        elif name == "ADD": reg[d] = reg[a] + reg[b]
        elif name == "SUB": reg[d] = reg[a] - reg[b]
        elif name == "MUL": reg[d] = reg[a] * reg[b]
        elif name == "DIV": reg[d] = reg[a] / reg[b]
        elif name == "NEG": reg[d] = -reg[a]
        elif name == "POW": reg[d] = np.power(reg[a], reg[b])
        elif name == "POWI": reg[d] = np.power(reg[a], b)
        elif name == "LN": reg[d] = np.log(reg[a])
        elif name == "EXP": reg[d] = np.exp(reg[a])
        elif name == "SQRT": reg[d] = np.sqrt(reg[a])
        elif name == "SIN": reg[d] = np.sin(reg[a])
        elif name == "COS": reg[d] = np.cos(reg[a])
        elif name == "TANH": reg[d] = np.tanh(reg[a])
        elif name == "MAX": reg[d] = np.maximum(reg[a], reg[b])
        elif name == "MIN": reg[d] = np.minimum(reg[a], reg[b])
        elif name == "ABS": reg[d] = np.abs(reg[a])
        elif name == "LT": reg[d] = (reg[a] < reg[b]) * 1.0
        elif name == "GT": reg[d] = (reg[a] > reg[b]) * 1.0
        elif name == "LE": reg[d] = (reg[a] <= reg[b]) * 1.0
        elif name == "GE": reg[d] = (reg[a] >= reg[b]) * 1.0
        elif name == "EQ": reg[d] = (reg[a] == reg[b]) * 1.0
        elif name == "AND": reg[d] = ((np.asarray(reg[a]) != 0) & (np.asarray(reg[b]) != 0)) * 1.0
        elif name == "OR": reg[d] = ((np.asarray(reg[a]) != 0) | (np.asarray(reg[b]) != 0)) * 1.0
        elif name == "NOT": reg[d] = (np.asarray(reg[a]) == 0) * 1.0
        elif name == "SEL": reg[d] = np.where(np.asarray(reg[a]) != 0, reg[b], reg[d])
        elif name == "MOV": reg[d] = reg[a]
        elif name == "OUT": out[a] = out[a] + reg[b]
        else: raise ValueError(name)
    return out
