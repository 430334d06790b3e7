"""Membrane models of the EMI problem (reference src/CGx/EMI/EMIx_ionic_model.py): ``Passive_model`` (I_ch = phi_M) and ``HH_model``
(Hodgkin-Huxley with a stimulus conductance added to g_Na).  ``_eval`` returns the channel current as an expression over phi_M and
the nodal gating variables; ``ProblemEMI.setup_linear_form`` compiles it to a membrane bytecode program (KNP_OP_PHIM, KNP_OP_AUX
0..2, constants, KNP_OP_OUT 0).  The stimulus value is a program constant that is refreshed at every step.  The gating update is the
library's ``knp_hh_update`` (same rates as EMIx_ionic_model.py:154-159), 25 sub-steps with V_rest = -0.065."""
from __future__ import annotations

from abc import ABC, abstractmethod

import numpy as np

from . import fem
from .fem import Constant, Function


def g_syn_none(t: float) -> float:
    """zero stimulus (default)"""
    return 0.0


def g_syn(t: float) -> float:
    """EMIx_ionic_model.py:15-23"""
    a_syn = 0.002
    g_syn_bar = 40
    return g_syn_bar * np.exp(-np.mod(t, 0.01) / a_syn)


class IonicModel(ABC):
    # integration of the states a model declares with ``add_state``
    use_Rush_Larsen = True
    time_steps_ODE = 25

    def __init__(self, EMIx_problem, tags=None):
        self.problem = EMIx_problem
        self.tags = tags
        if self.tags is None:
            self.tags = self.problem.gamma_tags
        if isinstance(self.tags, int):
            self.tags = (self.tags,)
        self.tags = tuple(self.tags)

    def _init(self):
        pass

    @abstractmethod
    def _eval(self):
        ...

    def add_state(self, name, init, alpha=None, beta=None, inf=None, tau=None, rhs=None):
        """Declare a nodal state of this mechanism, from ``_init()``; returns its Function (filled with ``init``, a number or nodal
        values) for use in ``_eval`` and in rate expressions.  One of
          ``alpha=, beta=``  gate, dy/dt = alpha (1 - y) - beta y (where alpha + beta == 0 the gate keeps its value);
          ``inf=, tau=``     the same gate with alpha = inf / tau, beta = (1 - inf) / tau;
          ``rhs=``           general, dy/dt = rhs.
        An expression may be a callable of the state's own Function (``rhs=lambda y: -y / tau``); it is called when the programs
        are compiled, so it may name states that are declared later.
        The expressions may read phi_M, SpatialCoordinate, Constants and any state.  ``update()`` advances the states on the GPU
        (knp_state_update): gates with frozen rates, by the Rush-Larsen step or ``time_steps_ODE`` forward-Euler sub-steps
        (``use_Rush_Larsen``); general states by forward-Euler sub-steps.  It is this class's ``update()`` that does so: a model
        that overrides ``update()`` calls ``super().update()``, or its declared states never advance."""
        return fem.declare_state(self, name, init, alpha=alpha, beta=beta, inf=inf, tau=tau, rhs=rhs).function

    def refresh(self, t: float):
        """time-dependent constants of the program, before the right-hand side of the step ending at ``t``"""

    def update(self):
        """after the solve: advance the model's state with the new phi_M -- the declared states of all models in one launch.
        An override keeps the declared states moving by calling ``super().update()`` (``HH_model`` declares none)."""
        if getattr(self, "states", None):
            self.problem.advance_states(self)


class Passive_model(IonicModel):
    def __str__(self):
        return "Passive"

    def _eval(self):
        return self.problem.phi_M


class HH_model(IonicModel):
    # initial gating variables
    n_init_val = 0.27622914792
    m_init_val = 0.03791834627
    h_init_val = 0.68848921811
    # conductivities (S/m**2) and reversal potentials (V), EMIx_ionic_model.py:70-79
    g_Na_bar = 1200
    g_K_bar = 360
    g_Na_leak = 2.0 * 0.5
    g_K_leak = 8.0 * 0.5
    g_Cl_leak = 0.0
    V_rest = -0.065
    E_Na = 54.8e-3
    E_K = -88.98e-3
    E_Cl = 0
    # numerics
    use_Rush_Lar = True
    time_steps_ODE = 25
    save_png_file = True

    def __init__(self, EMIx_problem, tags=None, stim_fun=g_syn_none):
        super().__init__(EMIx_problem, tags)
        self.g_Na_stim = stim_fun

    def __str__(self):
        return "Hodgkin-Huxley"

    def _init(self):
        p = self.problem
        if not hasattr(p, "n"):
            p.n, p.m, p.h = Function(p.V, "n"), Function(p.V, "m"), Function(p.V, "h")
            p.n.x.array[:] = self.n_init_val
            p.m.x.array[:] = self.m_init_val
            p.h.x.array[:] = self.h_init_val
        self.g_stim = Constant(p.mesh, self.g_Na_stim(float(p.t.value)))

    def _eval(self):
        p = self.problem
        if not hasattr(self, "g_stim"):
            self._init()
        g_Na = self.g_Na_leak + self.g_Na_bar * p.m ** 3 * p.h
        g_K = self.g_K_leak + self.g_K_bar * p.n ** 4
        g_Cl = self.g_Cl_leak
        g_Na = g_Na + self.g_stim
        I_ch_Na = g_Na * (p.phi_M - self.E_Na)
        I_ch_K = g_K * (p.phi_M - self.E_K)
        I_ch_Cl = g_Cl * (p.phi_M - self.E_Cl)
        return I_ch_Na + I_ch_K + I_ch_Cl

    def refresh(self, t):
        self.g_stim.value = float(self.g_Na_stim(float(t)))

    def update(self):
        self.update_gating_variables()

    def update_gating_variables(self):
        p = self.problem
        p.backend.hh_update(p.phi_M, p.n, p.m, p.h, float(p.dt.value), self.V_rest, bool(self.use_Rush_Lar), int(self.time_steps_ODE))
