"""Trans-membrane molar ion fluxes with the call surface of the reference's utils/calc_fluxes.py: ``create_flux_forms(problem)``
and ``compute_fluxes(flux_forms, comm)``.

A flux "form" here is a handle: (evaluator, position).  The evaluator is bound to ``problem.membrane_data_tag`` and to the
stimulus-region mask; the ``2 N_ions`` handles of one ``create_flux_forms`` call share it, so ``compute_fluxes`` gets all of
them from one pass over the membrane on the device (knp_diag_membrane_fluxes, csrc/knp_diagnostics.inc) and one read-back.

    flux[s][k] = int_Gamma(tag) mask (-D_k (grad c_k^s + (z_k / psi) c_k^s grad phi^s)) . n_s dS      [mol/s]

s = 0: intracellular fields and the normal out of the intracellular cell; s = 1: extracellular fields and the opposite normal.
A positive value means ions leave that side's domain through the membrane.
"""
from __future__ import annotations

import numpy as np

from .diagnostics import stimulus_box


class FluxEvaluator:
    """The fluxes through one set of membrane tags (one group), optionally masked with the stimulus region"""

    def __init__(self, problem, tags, mask=True):
        self.problem = problem
        self.groups = (tuple(int(t) for t in tags),)
        self.box = stimulus_box(problem) if mask else None

    def enqueue(self, out=None):
        """this rank's part, [2 N_ions] on the device (side-major): launched, not waited for"""
        be = self.problem.create_backend()
        be.set_flux_groups(self.groups, self.box)
        return be.membrane_fluxes(out)

    def values(self):
        """[2 N_ions] on the host, this rank's part: one launch pair, one read-back"""
        return self.enqueue().reshape(-1).cpu().numpy()


class FluxForm:
    """One of the ``2 N_ions`` scalars of an evaluator: ``index = side * N_ions + ion``"""

    def __init__(self, evaluator, index, name):
        self.evaluator = evaluator
        self.index = index
        self.name = name

    def __repr__(self):
        return f"FluxForm({self.name}, tags={self.evaluator.groups[0]}, masked={self.evaluator.box is not None})"


def create_flux_forms(problem):
    """Handles of the molar fluxes [mol/s] across the membrane ``problem.membrane_data_tag`` inside the stimulus region (when the
    problem has one): intracellular Na, K, Cl, then extracellular Na, K, Cl."""
    ev = FluxEvaluator(problem, [problem.membrane_data_tag], mask=True)
    n = problem.N_ions
    return [FluxForm(ev, s * n + k, f"{ion['name']}_{'ie'[s]}") for s in range(2) for k, ion in enumerate(problem.ion_list)]


def compute_fluxes(flux_forms, comm=None):
    """The values of the handles, summed over the ranks of ``comm`` (default: the problem's communicator), as an array in the order
    of ``flux_forms``.  Handles of one evaluator are computed together, once per call."""
    cache = {}
    out = np.zeros(len(flux_forms))
    for i, f in enumerate(flux_forms):
        ev = f.evaluator
        if id(ev) not in cache:
            cache[id(ev)] = ev.values()
        out[i] = cache[id(ev)][f.index]
    for i, f in enumerate(flux_forms):
        c = comm if comm is not None and hasattr(comm, "allreduce_sum") else f.evaluator.problem.comm
        out[i] = c.allreduce_sum(float(out[i]))
    return out
