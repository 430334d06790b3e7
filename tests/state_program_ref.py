"""One PDE step of the state variables that membrane mechanisms declare with ``IonicModel.add_state``, restated in NumPy on top of
``fem.interpret_program`` (long double by default), independently of the kernel that the GPU tests check against it.

Semantics (the reference's Hodgkin-Huxley update, KNPEMIx_ionic_model.py:605-671, for any mechanism):
  * a gate (kind 0) has rates alpha = OUT 0 and beta = OUT 1 of its program, evaluated ONCE from the values at the start of the
    step.  Rush-Larsen: y <- y_inf + (y - y_inf) exp(-dt (alpha + beta)) with y_inf = alpha / (alpha + beta), applied at the end
    of the step -- until then other programs read the start-of-step value; where alpha + beta == 0 the gate keeps its value.
    Forward Euler: ``substeps`` steps of dto = dt / substeps, y += dto alpha (1 - y) - dto beta y.
  * a general state (kind 1) takes ``substeps`` forward-Euler steps y += dto * OUT 0, its program evaluated in each.
  * within a sub-step every program reads the states as they stood at its beginning; all states advance at its end.
"""
from __future__ import annotations

import numpy as np

from cgx_hip import fem
from cgx_hip._lib import KNP_MAX_AUX


def outputs(state, y_of_slot, phim, ki, ke, x):
    """(OUT 0, OUT 1) of the state's program with the aux slots ``y_of_slot`` (list of KNP_MAX_AUX arrays)"""
    out = fem.interpret_program(state.spec, ki, ke, phim, y_of_slot, x)
    return out[0], out[1]


def state_step(states, y, phim, dt, rush_larsen, substeps, ki=None, ke=None, aux=None, x=None, dtype=np.longdouble):
    """New values of ``states`` (compiled ``fem.StateVariable``s) from the values ``y`` (one array per state).  ``phim``: nodal
    membrane potential; ``ki`` / ``ke``: three nodal concentrations each; ``aux``: {slot: array} of aux fields that are not states;
    ``x``: one coordinate array per axis.  Nothing is modified."""
    T = dtype
    n = np.asarray(phim).shape[0]
    cast = lambda a: np.array(a, dtype=T)
    y = [cast(v) for v in y]
    phim = cast(phim)
    zero = np.zeros(n, dtype=T)
    ki = [cast(a) for a in ki] if ki is not None else [zero] * 3
    ke = [cast(a) for a in ke] if ke is not None else [zero] * 3
    x = [cast(a) for a in x] if x is not None else [zero] * 3
    other = [zero] * KNP_MAX_AUX
    for k, a in (aux or {}).items():
        other[k] = cast(a)

    def slots(values):
        a = list(other)
        for st, v in zip(states, values):
            a[st.aux_index] = v
        return a

    dt_T = T(dt)
    dto = dt_T / T(substeps)
    start = slots(y)
    rates = {s: outputs(st, start, phim, ki, ke, x) for s, st in enumerate(states) if st.kind == 0}
    for _ in range(int(substeps)):
        now = slots(y)
        new = []
        for s, st in enumerate(states):
            if st.kind == 1:
                new.append(y[s] + dto * outputs(st, now, phim, ki, ke, x)[0])
            elif rush_larsen:
                new.append(y[s])
            else:
                al, be = rates[s]
                new.append(y[s] + dto * al * (1 - y[s]) - dto * be * y[s])
        y = new
    if rush_larsen:
        for s, (al, be) in rates.items():
            r = al + be + 0 * y[s]
            live = r != 0                   # both rates zero: dy/dt = 0, the gate stays
            safe = np.where(live, r, 1)
            y[s] = np.where(live, al / safe + (y[s] - al / safe) * np.exp(-dt_T * r), y[s])
    return y
