"""Mechanisms that declare their gates and states through ``IonicModel.add_state``, shared by test_state_programs_host.py and
test_gpu_state_update.py: the Hodgkin-Huxley model restated that way for both model families (its closed forms are those of
``k_hh_update``, csrc/knp_kernels.hip), and small mechanisms that exercise the three keyword forms."""
from __future__ import annotations

import numpy as np

from parity_utils import ci_config, make_problem  # noqa: F401  (also puts the package on sys.path)

from cgx_hip import emi_models, fem
from cgx_hip.fem import Constant
from cgx_hip.ionic_models import HodgkinHuxley, IonicModel


def hh_rates(V, exp=fem.exp):
    """{gate: (alpha, beta)} in 1/s of V in mV above rest, operation by operation as ``k_hh_update`` writes them"""
    return {"n": (0.01e3 * (10.0 - V) / (exp((10.0 - V) / 10.0) - 1.0), 0.125e3 * exp(-V / 80.0)),
            "m": (0.1e3 * (25.0 - V) / (exp((25.0 - V) / 10.0) - 1.0), 4.0e3 * exp(-V / 18.0)),
            "h": (0.07e3 * exp(-V / 20.0), 1.0e3 / (exp((30.0 - V) / 10.0) + 1.0))}


def hh_closed_form(phi_m, n, m, h, dt, phi_rest, rush_larsen, substeps):
    """``k_hh_update`` restated in NumPy, in the precision of its inputs"""
    T = np.asarray(phi_m).dtype.type
    V = T(1000.0) * (phi_m - T(phi_rest))
    r = hh_rates(V, exp=np.exp)
    out = []
    for y, g in ((n, "n"), (m, "m"), (h, "h")):
        a, b = r[g]
        y = np.array(y, dtype=T)
        if rush_larsen:
            t = a + b
            y_inf = a / t
            y = y_inf + (y - y_inf) * np.exp(-T(dt) * t)
        else:
            dto = T(dt) / T(substeps)
            for _ in range(substeps):
                y = y + dto * a * (1 - y) - dto * b * y
        out.append(y)
    return out


def away_from_singularities(rng, size, phi_rest, lo=-0.1, hi=0.1):
    """phi_m in [lo, hi] V with V = 1000 (phi_m - phi_rest) more than 0.5 mV away from 10 and 25 mV, where alpha_n and alpha_m are 0 / 0"""
    phi = rng.uniform(lo, hi, size)
    for _ in range(100):
        V = 1000.0 * (phi - phi_rest)
        bad = (np.abs(V - 10.0) <= 0.5) | (np.abs(V - 25.0) <= 0.5)
        if not bad.any():
            return phi
        phi[bad] = rng.uniform(lo, hi, int(bad.sum()))
    raise AssertionError("no admissible phi_m drawn")


class HHFromStates(HodgkinHuxley):
    """The currents and the stimulus of ``HodgkinHuxley`` (inherited); n, m, h declared with ``add_state`` instead of advanced by
    ``knp_hh_update``"""

    def __str__(self):
        return "Hodgkin-Huxley from declared states"

    def _init(self):
        p = self.problem
        r = hh_rates(1000.0 * (p.phi_m_prev - p.phi_rest))
        for g in ("n", "m", "h"):
            setattr(p, g, self.add_state(g, getattr(p, g + "_init").value, alpha=r[g][0], beta=r[g][1]))
        self.t_mod = Constant(p.mesh, 0.0)

    def update_gating_variables(self):      # the solver advances the declared states
        pass


def hh_from_states_models(use_Rush_Larsen=True, time_steps_ODE=25):
    """the CI mechanism set and order of ``make_problem(cfg, "ci")`` with ``HHFromStates`` in the place of ``HodgkinHuxley``"""
    from cgx_hip.ionic_models import ATPPump, NeuronalCotransporters
    return lambda p: [NeuronalCotransporters(p), HHFromStates(p, use_Rush_Larsen=use_Rush_Larsen, time_steps_ODE=time_steps_ODE), ATPPump(p)]


class HHStatesEMI(emi_models.IonicModel):
    """``emi_models.HH_model`` with its gates declared through ``add_state`` (same constants, same current, same stimulus)"""
    H = emi_models.HH_model

    def __init__(self, EMIx_problem, tags=None, stim_fun=emi_models.g_syn_none):
        super().__init__(EMIx_problem, tags)
        self.g_Na_stim = stim_fun
        self.use_Rush_Larsen, self.time_steps_ODE = bool(self.H.use_Rush_Lar), int(self.H.time_steps_ODE)

    def __str__(self):
        return "Hodgkin-Huxley from declared states"

    def _init(self):
        p, H = self.problem, self.H
        r = hh_rates(1000.0 * (p.phi_M - H.V_rest))
        self.n = self.add_state("n", H.n_init_val, alpha=r["n"][0], beta=r["n"][1])
        self.m = self.add_state("m", H.m_init_val, alpha=r["m"][0], beta=r["m"][1])
        self.h = self.add_state("h", H.h_init_val, alpha=r["h"][0], beta=r["h"][1])
        self.g_stim = Constant(p.mesh, self.g_Na_stim(float(p.t.value)))

    def _eval(self):
        p, H = self.problem, self.H
        g_Na = H.g_Na_leak + H.g_Na_bar * self.m ** 3 * self.h
        g_K = H.g_K_leak + H.g_K_bar * self.n ** 4
        g_Na = g_Na + self.g_stim
        return g_Na * (p.phi_M - H.E_Na) + g_K * (p.phi_M - H.E_K) + H.g_Cl_leak * (p.phi_M - H.E_Cl)

    def refresh(self, t):
        self.g_stim.value = float(self.g_Na_stim(float(t)))


class Mixed(IonicModel):
    """A passive current and states of every form: a gate whose rates read K_e and another state, an inf / tau gate, a general
    state dy/dt = -a g (phi_m - E) - y / tau, two general states that read each other, and a time-dependent Constant"""
    A, E, TAU, W = 40.0, -0.08, 4e-3, 300.0

    def __str__(self):
        return "states of every form"

    def _init(self):
        p = self.problem
        ph, K_e = p.phi_m_prev, p.wh[1][1]
        x = fem.SpatialCoordinate(p.mesh)
        self.drive = Constant(p.mesh, 1.0)
        self.q = self.add_state("q", 0.3, inf=1.0 / (1.0 + fem.exp(-(ph + 0.05) / 0.01)), tau=2e-3 + 1e-3 * fem.exp(-(ph / 0.05) ** 2))
        self.g = self.add_state("g", np.linspace(0.1, 0.9, p.mesh.num_vertices),
                                alpha=50.0 * K_e * (1.0 + self.q), beta=lambda g: 120.0 * fem.exp(ph / 0.04) + 10.0 * g * x[0] * 1e6)
        self.y = self.add_state("y", 0.05, rhs=lambda y: -self.A * self.g * (ph - self.E) - y / self.TAU)
        self.u = self.add_state("u", 1.0, rhs=lambda u: self.W * self.v * self.drive)      # v is declared next
        self.v = self.add_state("v", 0.0, rhs=-self.W * self.u)

    def _eval(self, ion_idx):
        return self.problem.phi_m_prev * (1.0 + 0.1 * self.q)


class MaskedGate(IonicModel):
    """a gate whose rates are both zero on half of the mesh (x below the middle of the micrometre-scaled unit box)"""

    def __str__(self):
        return "masked gate"

    def _init(self):
        p = self.problem
        on = fem.conditional(fem.gt(fem.SpatialCoordinate(p.mesh)[0], 0.5e-6), 1.0, 0.0)
        self.calls = 0
        self.w = self.add_state("w", 0.4, alpha=on * 80.0, beta=on * 20.0)
        self.z = self.add_state("z", 0.2, inf=self._inf, tau=5e-3)

    def _inf(self, z):
        self.calls += 1
        return 1.0 / (1.0 + fem.exp(-(self.problem.phi_m_prev + 0.05) / 0.01))

    def _eval(self, ion_idx):
        return self.problem.phi_m_prev * (1.0 + 0.1 * self.w)
