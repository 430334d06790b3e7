"""0-D membrane ODE systems that give steady-state initial conditions (reference src/CGx/utils/membrane_ODE_systems.py).

A config without ``initial_conditions`` starts from the rest state of the membrane mechanisms: every compartment is one
well-mixed volume, the membrane one lumped area, and the ODE system of membrane potential(s), concentrations and
Hodgkin-Huxley gates is integrated until its right-hand side vanishes.  Restated from the equations of the reference:

  two compartments (neuron + ECS), state (phi_m, Na_i, Na_e, K_i, K_e, Cl_i, Cl_e, n, m, h);
  three compartments (neuron + glia + ECS), state (phi_m_n, Na_i_n, Na_e, K_i_n, K_e, Cl_i_n, Cl_e, phi_m_g, Na_i_g,
  K_i_g, Cl_i_g, n, m, h).

  d phi_m / dt = -(I_Na + I_K + I_Cl) / C_M                           [V/s]
  d k_i / dt   = -I_k / (z_k F) * area / vol_i,  d k_e / dt = +sum over membranes of I_k / (z_k F) * area / vol_e   [mM/s]
  d g / dt     = alpha_g (1 - g) - beta_g g,  g in {n, m, h}, rates at V = 1e3 (phi_m - phi_rest)

Neuronal currents: HH + leak, the Na/K-ATPase (3 Na out, 2 K in), KCC2 and NKCC1; glial currents: Kir4.1 on the K leak,
the glial pump, KCC1 and glial NKCC1.  Conductances are the problem's constants (``stimulus.conductance`` overrides,
otherwise the defaults of mixed_dim_problem.py:311-330); the initial guesses are the problem's default ``*_init``
constants and the gates start at alpha / (alpha + beta) of the guessed potential.

One deliberate quirk of the reference is kept: ``K_e_0`` (the upper end of the NKCC1 band and the Kir normalisation)
and ``E_K_0`` (Kir, from the *neuronal* K_i guess) are the guesses, while the PDE mechanisms later use the found K_e.
With the default guess K_e_0 = 3 mM the NKCC1 band [3, K_e_0] is empty, so NKCC1 is silent here as in the PDE.

Runs once on the host before the first step; there is no device code here.
"""
from __future__ import annotations

import math
from abc import ABC, abstractmethod

import numpy as np

# pump and cotransporter constants (reference :219-225, :280, :289-294)
_I_HAT = 0.25            # neuronal pump strength [A/m^2]
_P_NA_I = 10.0           # [Na+]_i threshold of the pumps [mM]
_P_K_E = 1.5             # [K+]_e threshold of the pumps [mM]
_S_KCC2 = 0.0068         # [A/m^2]
_S_NKCC1 = 0.00023       # [A/m^2]
_RHO_PUMP_G = 1.1 * 1.12e-6   # glial pump rate [mol/(m^2 s)]
_G_KCC1 = 7e-2           # [S/m^2]
_G_NKCC1_G = 2e-2        # [S/m^2]


def hh_rates(V):
    """Hodgkin-Huxley rates [1/s] at V = 1e3 (phi_m - phi_rest) [mV]: (alpha_n, beta_n, alpha_m, beta_m, alpha_h, beta_h)."""
    return (10.0 * (10.0 - V) / (np.exp((10.0 - V) / 10.0) - 1.0), 125.0 * np.exp(-V / 80.0),
            100.0 * (25.0 - V) / (np.exp((25.0 - V) / 10.0) - 1.0), 4000.0 * np.exp(-V / 18.0),
            70.0 * np.exp(-V / 20.0), 1000.0 / (np.exp((30.0 - V) / 10.0) + 1.0))


def f_NKCC1(K_e, K_e_0, K_min=3.0, eps=1e-6, cap=1.0):
    """NKCC1 silencing factor: zero outside the open band (K_min, K_e_0), a steep switch inside it (reference :104-115)."""
    K_e = np.asarray(K_e, dtype=np.float64)
    val = 1.0 / (1.0 + (0.03 / np.maximum(K_e - K_e_0, eps)) ** 10)
    return np.where((K_e <= K_min) | (K_e >= K_e_0), 0.0, np.clip(val, 0.0, cap))


def _have_matplotlib():
    try:
        import matplotlib  # noqa: F401
    except Exception:          # noqa: BLE001
        return False
    return True


class MembraneODESystem(ABC):
    """Steady state of a 0-D membrane ODE system, found by integrating it in time (reference :9-115)."""

    state_names: tuple = ()

    def __init__(self, problem, plot_show: bool = False, plot_save: bool = False, stimulus_flag: bool = False,
                 timestep: float = 1e-3, max_time: float = 500.0, verbose: bool = False):
        if stimulus_flag:
            raise NotImplementedError("stimulus_flag=True: the stimulus-driven membrane ODE is not implemented; "
                                      "steady-state initial conditions use stimulus_flag=False")
        self.problem = problem
        self.plot_show, self.plot_save = bool(plot_show), bool(plot_save)
        self.plot = (self.plot_show or self.plot_save) and _have_matplotlib()
        self.stimulus = False
        self.timestep = float(timestep)
        self.max_time = float(max_time)
        self.verbose = bool(verbose)
        self.initialize_constants()

    def initialize_constants(self):
        p = self.problem
        self.R, self.F, self.T, self.C_M = p.R.value, p.F.value, p.T.value, p.C_M.value
        self.psi = self.R * self.T / self.F
        self.g_Na_bar, self.g_K_bar = p.g_Na_bar.value, p.g_K_bar.value
        self.g_Na_leak, self.g_K_leak, self.g_Cl_leak = p.g_Na_leak.value, p.g_K_leak.value, p.g_Cl_leak.value
        self.phi_rest = p.phi_rest.value
        # guesses: the problem's default constants
        self.phi_m_init, self.Na_i_init, self.Na_e_init = p.phi_m_init.value, p.Na_i_init.value, p.Na_e_init.value
        self.K_i_init, self.K_e_init = p.K_i_init.value, p.K_e_init.value
        self.Cl_i_init, self.Cl_e_init = p.Cl_i_init.value, p.Cl_e_init.value
        # the guesses the mechanisms of the ODE keep (the quirk of the module docstring)
        self.K_e_0 = self.K_e_init

    def E(self, z, c_i, c_e):
        """Nernst potential [V]."""
        return self.psi / z * np.log(c_e / c_i)

    def gating_guess(self, phi_m):
        a_n, b_n, a_m, b_m, a_h, b_h = hh_rates((phi_m - self.phi_rest) * 1e3)
        return a_n / (a_n + b_n), a_m / (a_m + b_m), a_h / (a_h + b_h)

    def neuron_currents(self, phi, Na_i, Na_e, K_i, K_e, Cl_i, Cl_e, n, m, h):
        """(I_Na, I_K, I_Cl) through the neuronal membrane [A/m^2], outward positive."""
        I_ATP = _I_HAT / ((1.0 + _P_K_E / K_e) ** 2 * (1.0 + _P_NA_I / Na_i) ** 3)
        I_KCC2 = _S_KCC2 * np.log((K_i * Cl_i) / (K_e * Cl_e))
        I_NKCC1 = _S_NKCC1 * f_NKCC1(K_e, self.K_e_0) * np.log((Na_e * K_e * Cl_e ** 2) / (Na_i * K_i * Cl_i ** 2))
        I_Na = (self.g_Na_leak + self.g_Na_bar * m ** 3 * h) * (phi - self.E(1.0, Na_i, Na_e)) + 3.0 * I_ATP - I_NKCC1
        I_K = (self.g_K_leak + self.g_K_bar * n ** 4) * (phi - self.E(1.0, K_i, K_e)) - 2.0 * I_ATP - I_NKCC1 + I_KCC2
        I_Cl = self.g_Cl_leak * (phi - self.E(-1.0, Cl_i, Cl_e)) + 2.0 * I_NKCC1 - I_KCC2
        return I_Na, I_K, I_Cl

    def gating_rhs(self, phi, n, m, h):
        a_n, b_n, a_m, b_m, a_h, b_h = hh_rates((phi - self.phi_rest) * 1e3)
        return a_n * (1.0 - n) - b_n * n, a_m * (1.0 - m) - b_m * m, a_h * (1.0 - h) - b_h * h

    @abstractmethod
    def initial_guess(self) -> np.ndarray: ...

    @abstractmethod
    def rhs(self, t, x) -> np.ndarray:
        """Right-hand side; ``x`` is one state (n,) or a set of states (n, k)."""

    def initialize_initial_conditions(self, init_cond_array):
        for name, v in zip(self.state_names, init_cond_array):
            setattr(self, name + "_init", float(v))

    def solve_ode_system(self) -> list:
        """Integrate from the guesses until ``allclose(rhs, 0, rtol=1e-8, atol=1e-10)`` holds at a point of the
        ``timestep`` grid; returns that state (reference order and units).  ``solve_ivp(Radau, rtol=1e-6, atol=1e-8)``
        runs over windows of up to 1000 grid intervals (the reference restarts it every interval) and the stopping rule is
        checked at every grid point of a window.  Raises ``RuntimeError`` on a non-finite state or without a steady state
        by ``max_time``."""
        from scipy.integrate import solve_ivp
        x = np.asarray(self.initial_guess(), dtype=np.float64)
        dt, n_grid = self.timestep, int(round(self.max_time / self.timestep))
        traj = [(0.0, x.copy())] if self.plot else None
        k, width = 0, 1
        f = self.rhs(0.0, x)
        while k < n_grid:
            k1 = min(k + width, n_grid)
            grid = np.arange(k + 1, k1 + 1) * dt
            sol = solve_ivp(self.rhs, (k * dt, k1 * dt), x, method="Radau", rtol=1e-6, atol=1e-8, t_eval=grid)
            if sol.status < 0 or sol.y.shape[1] != grid.size:
                raise RuntimeError(f"membrane ODE: the integrator stopped at t = {sol.t[-1] if sol.t.size else k * dt:.6g} s: {sol.message}")
            Y = sol.y
            bad = ~np.isfinite(Y).all(axis=0)
            F = self.rhs(grid, Y)
            done = np.all(np.abs(F) <= 1e-10, axis=0) & ~bad          # allclose(F, 0, rtol=1e-8, atol=1e-10)
            stop = int(np.argmax(done | bad)) if (done | bad).any() else -1
            if traj is not None:
                traj += [(grid[j], Y[:, j].copy()) for j in range(grid.size if stop < 0 else stop + 1)]
            if stop >= 0 and bad[stop]:
                raise RuntimeError(f"membrane ODE: non-finite state at t = {grid[stop]:.6g} s (last finite largest |dx/dt| "
                                   f"{self._largest(f)})")
            if stop >= 0:
                x, self.t_steady = Y[:, stop].copy(), float(grid[stop])
                if self.verbose:
                    self.problem.print(f"Steady state reached at t = {self.t_steady:.3f} s: " +
                                       ", ".join(f"{nm} = {v:.12g}" for nm, v in zip(self.state_names, x)))
                if self.plot:
                    self.plot_results(traj)
                return [float(v) for v in x]
            x, f = Y[:, -1].copy(), F[:, -1]
            if self.verbose:
                self.problem.print(f"t = {k1 * dt:.3f} s: largest |dx/dt| {self._largest(f)}")
            k, width = k1, min(2 * width, 1000)
        if self.plot:
            self.plot_results(traj)
        raise RuntimeError(f"membrane ODE: no steady state within max_time = {self.max_time:g} s (t reached {n_grid * dt:.6g} s, "
                           f"largest |dx/dt| {self._largest(f)})")

    def _largest(self, f):
        j = int(np.argmax(np.abs(f)))
        return f"{abs(float(f[j])):.3e} in d{self.state_names[j]}/dt"

    def plot_results(self, traj):
        """One figure of the trajectory (potentials, concentrations, gates); shown and/or saved as membrane_ode.png."""
        import matplotlib
        if not self.plot_show:
            matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
        t = np.array([a for a, _ in traj])
        Y = np.array([b for _, b in traj])
        fig, axes = plt.subplots(1, 3, figsize=(15, 4))
        for j, nm in enumerate(self.state_names):
            ax = axes[0] if nm.startswith("phi") else axes[2] if nm in ("n", "m", "h") else axes[1]
            ax.plot(t, Y[:, j], label=nm)
        for ax, yl in zip(axes, ("potential [V]", "concentration [mM]", "gate")):
            ax.set_xlabel("t [s]")
            ax.set_ylabel(yl)
            ax.legend(fontsize="small")
        fig.tight_layout()
        if self.plot_save:
            fig.savefig("membrane_ode.png")
        if self.plot_show:
            plt.show()
        plt.close(fig)


class TwoCompartmentMembraneODESystem(MembraneODESystem):
    """Neurons and extracellular space (reference :585-827)."""

    state_names = ("phi_m", "Na_i", "Na_e", "K_i", "K_e", "Cl_i", "Cl_e", "n", "m", "h")

    def initial_guess(self):
        n0, m0, h0 = self.gating_guess(self.phi_m_init)
        return np.array([self.phi_m_init, self.Na_i_init, self.Na_e_init, self.K_i_init, self.K_e_init, self.Cl_i_init,
                         self.Cl_e_init, n0, m0, h0])

    def rhs(self, t, x):
        p = self.problem
        phi, Na_i, Na_e, K_i, K_e, Cl_i, Cl_e, n, m, h = x
        I_Na, I_K, I_Cl = self.neuron_currents(phi, Na_i, Na_e, K_i, K_e, Cl_i, Cl_e, n, m, h)
        si, se = p.area_g_n / (self.F * p.vol_i_n), p.area_g_n / (self.F * p.vol_e)
        dn, dm, dh = self.gating_rhs(phi, n, m, h)
        return np.array([-(I_Na + I_K + I_Cl) / self.C_M,
                         -I_Na * si, I_Na * se, -I_K * si, I_K * se, I_Cl * si, -I_Cl * se,
                         dn, dm, dh])


class ThreeCompartmentMembraneODESystem(MembraneODESystem):
    """Neurons, glia and extracellular space (reference :118-476)."""

    state_names = ("phi_m_n", "Na_i_n", "Na_e", "K_i_n", "K_e", "Cl_i_n", "Cl_e", "phi_m_g", "Na_i_g", "K_i_g", "Cl_i_g",
                   "n", "m", "h")

    def initialize_constants(self):
        super().initialize_constants()
        p = self.problem
        self.g_Na_leak_g, self.g_K_leak_g, self.g_Cl_leak_g = p.g_Na_leak_g.value, p.g_K_leak_g.value, p.g_Cl_leak_g.value
        self.phi_m_g_init, self.Na_i_g_init = p.phi_m_g_init.value, p.Na_i_g_init.value
        self.K_i_g_init, self.Cl_i_g_init = p.K_i_g_init.value, p.Cl_i_g_init.value
        # Kir4.1 constants: E_K_0 from the NEURONAL K_i guess and the K_e guess (reference :274-278)
        self.E_K_0 = float(self.E(1.0, self.K_i_init, self.K_e_0))
        self.kir_AB = (1.0 + math.exp(0.433)) * (1.0 + math.exp(-(0.1186 + self.E_K_0) / 0.0441))

    def initial_guess(self):
        n0, m0, h0 = self.gating_guess(self.phi_m_init)
        return np.array([self.phi_m_init, self.Na_i_init, self.Na_e_init, self.K_i_init, self.K_e_init, self.Cl_i_init,
                         self.Cl_e_init, self.phi_m_g_init, self.Na_i_g_init, self.K_i_g_init, self.Cl_i_g_init, n0, m0, h0])

    def f_Kir(self, K_e, phi_g, E_K_g):
        C = 1.0 + np.exp((phi_g - E_K_g + 0.0185) / 0.0425)
        D = 1.0 + np.exp(-(0.1186 + phi_g) / 0.0441)
        return self.kir_AB / (C * D) * np.sqrt(K_e / self.K_e_0)

    def glia_currents(self, phi, Na_i, Na_e, K_i, K_e, Cl_i, Cl_e):
        """(I_Na, I_K, I_Cl) through the glial membrane [A/m^2], outward positive."""
        I_pump = _RHO_PUMP_G * self.F / (1.0 + (_P_NA_I / Na_i) ** 1.5) / (1.0 + _P_K_E / K_e)
        I_KCC1 = _G_KCC1 * self.psi * np.log((K_i * Cl_i) / (K_e * Cl_e))
        I_NKCC1 = _G_NKCC1_G * self.psi * f_NKCC1(K_e, self.K_e_0) * np.log((Na_e * K_e * Cl_e ** 2) / (Na_i * K_i * Cl_i ** 2))
        E_K = self.E(1.0, K_i, K_e)
        I_Na = self.g_Na_leak_g * (phi - self.E(1.0, Na_i, Na_e)) + 3.0 * I_pump - I_NKCC1
        I_K = self.g_K_leak_g * self.f_Kir(K_e, phi, E_K) * (phi - E_K) - 2.0 * I_pump - I_NKCC1 + I_KCC1
        I_Cl = self.g_Cl_leak_g * (phi - self.E(-1.0, Cl_i, Cl_e)) + 2.0 * I_NKCC1 - I_KCC1
        return I_Na, I_K, I_Cl

    def rhs(self, t, x):
        p = self.problem
        phi_n, Na_i_n, Na_e, K_i_n, K_e, Cl_i_n, Cl_e, phi_g, Na_i_g, K_i_g, Cl_i_g, n, m, h = x
        In = self.neuron_currents(phi_n, Na_i_n, Na_e, K_i_n, K_e, Cl_i_n, Cl_e, n, m, h)
        Ig = self.glia_currents(phi_g, Na_i_g, Na_e, K_i_g, K_e, Cl_i_g, Cl_e)
        sn, sg = p.area_g_n / (self.F * p.vol_i_n), p.area_g_g / (self.F * p.vol_i_g)
        en, eg = p.area_g_n / (self.F * p.vol_e), p.area_g_g / (self.F * p.vol_e)
        z = (1.0, 1.0, -1.0)
        dn, dm, dh = self.gating_rhs(phi_n, n, m, h)
        return np.array([-(In[0] + In[1] + In[2]) / self.C_M,
                         -In[0] * sn, (In[0] * en + Ig[0] * eg),
                         -In[1] * sn, (In[1] * en + Ig[1] * eg),
                         In[2] * sn, -(In[2] * en + Ig[2] * eg),
                         -(Ig[0] + Ig[1] + Ig[2]) / self.C_M,
                         -Ig[0] * sg / z[0], -Ig[1] * sg / z[1], -Ig[2] * sg / z[2],
                         dn, dm, dh])
