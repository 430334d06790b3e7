"""Flexible GMRES without a GPU: which ksp_type / norm_type combinations the solver accepts (PETSc's table, as the reference would get
it), and the NumPy restatement of the method (tests/fgmres_ref.py) against dense solves, including a preconditioner that changes from
one application to the next."""
from __future__ import annotations

import numpy as np
import pytest

from fgmres_ref import CONVERGED_RTOL, DIVERGED_ITS, fgmres
from parity_utils import ci_config, make_problem


def _solver(ksp_type=None, norm_type=None, direct=False, pc="hypre"):
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    cfg = ci_config(N=8, steps=1, pc=pc, direct=direct)
    ks = cfg["solver"]["ksp_settings"]
    ks.pop("norm_type", None)
    if ksp_type is not None:
        ks["ksp_type"] = ksp_type
    if norm_type is not None:
        ks["norm_type"] = norm_type
    p = make_problem(cfg)
    return SolverKNPEMI(p, solver_config=p.solver_config)


@pytest.mark.parametrize("ksp_type,norm_type,flexible", [
    ("gmres", None, False), ("gmres", "preconditioned", False), ("gmres", "unpreconditioned", True), ("fgmres", "unpreconditioned", True)])
def test_accepted_settings(ksp_type, norm_type, flexible):
    s = _solver(ksp_type, norm_type)
    assert s._flexible is flexible


def test_direct_keeps_left_gmres():
    assert _solver("fgmres", "unpreconditioned", direct=True)._flexible is False


@pytest.mark.parametrize("norm_type", [None, "preconditioned"])
def test_fgmres_needs_unpreconditioned_norm(norm_type):
    """PETSc: FGMRES supports only right preconditioning, so only the unpreconditioned norm (the reference always sets it)."""
    with pytest.raises(ValueError, match="unpreconditioned"):
        _solver("fgmres", norm_type)


@pytest.mark.parametrize("ksp_type,norm_type", [("cg", None), ("bcgs", "unpreconditioned"), ("preonly", None), ("gmres", "natural"),
                                                ("gmres", "none")])
def test_other_settings_still_refused(ksp_type, norm_type):
    with pytest.raises(NotImplementedError):
        _solver(ksp_type, norm_type)


def _system(n, seed, singular=False):
    rng = np.random.default_rng(seed)
    A = np.eye(n) * 4 + rng.standard_normal((n, n)) / np.sqrt(n) + np.diag(rng.uniform(0, 3, n))   # nonsymmetric, well conditioned
    ns = None
    if singular:   # A ns = 0 with ns the normalised indicator of every fourth entry (the potentials), b consistent
        ns = np.zeros(n)
        ns[3::4] = 1.0
        ns /= np.linalg.norm(ns)
        A = A - np.outer(A @ ns, ns)
        ell = np.linalg.svd(A)[0][:, -1]   # left null vector
        b = rng.standard_normal(n)
        b -= ell * (ell @ b)
        return A, b, ns
    return A, rng.standard_normal(n), ns


@pytest.mark.parametrize("restart", [30, 5, 2])
def test_matches_dense_solve(restart):
    A, b, _ = _system(80, 1)
    x0 = np.random.default_rng(2).standard_normal(80)
    M = np.diag(1.0 / np.diag(A))
    x, its, res, reason = fgmres(A, b, x0, M, rtol=1e-12, restart=restart)
    assert reason == CONVERGED_RTOL
    true = np.linalg.norm(b - A @ x)
    assert true <= 1e-12 * np.linalg.norm(b) * 1.05 and abs(true - res) <= 1e-3 * res + 1e-15 * np.linalg.norm(b)
    xs = np.linalg.solve(A, b)
    assert np.abs(x - xs).max() <= 1e-10 * np.abs(xs).max()
    if restart == 2:
        assert its > 2   # the restarted path ran


def test_flexible_preconditioner():
    """A preconditioner that is a different operator at every application (alternating Jacobi / a few steps of an inner iteration):
    left GMRES has no Krylov space for it, FGMRES still converges to the dense solution on the true residual."""
    A, b, _ = _system(60, 3)
    D = np.diag(1.0 / np.diag(A))
    calls = {"k": 0}

    def M(v):
        calls["k"] += 1
        k = calls["k"]
        if k % 3 == 0:
            return D @ v
        z = np.zeros_like(v)
        for _ in range(1 + k % 4):   # inexact inner Richardson-Jacobi solve, a different number of sweeps each time
            z = z + D @ (v - A @ z)
        return z
    x, its, res, reason = fgmres(A, b, np.zeros(60), M, rtol=1e-11, restart=10)
    assert reason == CONVERGED_RTOL and calls["k"] == its
    xs = np.linalg.solve(A, b)
    assert np.linalg.norm(b - A @ x) <= 1.05e-11 * np.linalg.norm(b)
    assert np.abs(x - xs).max() <= 1e-9 * np.abs(xs).max()


def test_no_preconditioner_and_iteration_limit():
    A, b, _ = _system(50, 4)
    x, its, res, reason = fgmres(A, b, np.zeros(50), None, rtol=1e-10)
    assert reason == CONVERGED_RTOL and np.linalg.norm(b - A @ x) <= 1.05e-10 * np.linalg.norm(b)
    x, its, res, reason = fgmres(A, b, np.zeros(50), None, rtol=1e-14, max_it=3)
    assert reason == DIVERGED_ITS and its == 3


def test_gauge_step_keeps_the_null_space_component():
    """Singular A (A ns = 0, consistent b): the correction of every cycle is added without its ns component, so ns.x stays that of the
    initial guess while the true residual still meets the bound; the solution is the dense one in that gauge."""
    A, b, ns = _system(64, 5, singular=True)
    x0 = np.random.default_rng(6).standard_normal(64)
    M = np.diag(1.0 / np.diag(A + np.outer(ns, ns)))
    x, its, res, reason = fgmres(A, b, x0, M, ns=ns, rtol=1e-11, restart=4)
    assert reason == CONVERGED_RTOL
    assert abs(ns @ x - ns @ x0) <= 1e-12 * np.linalg.norm(x0)
    assert np.linalg.norm(b - A @ x) <= 1.05e-11 * np.linalg.norm(b)
    xs = np.linalg.lstsq(A, b, rcond=None)[0]
    xs += ns * (ns @ x0 - ns @ xs)
    assert np.abs(x - xs).max() <= 1e-8 * np.abs(xs).max()
