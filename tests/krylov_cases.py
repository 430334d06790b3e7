"""What the host and the GPU tests of the Krylov drivers share (tests/test_krylov_ref_host.py, tests/test_gpu_krylov_long.py): the cycle
lengths, the three comparisons of one cycle with the long-double optimum, the permutation spread that says how far summation order alone
moves a converged solve, and the inputs of an exact breakdown.  Host side, plain NumPy."""
from __future__ import annotations

import numpy as np

from fgmres_ref import fgmres
from gmres_ref import gmres

# edges of the fused short-cycle update (jd <= 8), of the SpMV-folded first stage (BU_MAX_M = 8), of every 8-wide k_multi_dot launch and
# of the slot layout (GM_MAX_RESTART = 55)
MS = (1, 2, 7, 8, 9, 16, 17, 24, 25, 32, 33, 48, 49, 55)
FLOOR = 1e-12
DRIVERS = {"left": gmres, "flex": fgmres}


def nullspace(n):
    ns = np.zeros(n)
    ns[3::4] = 1.0
    return ns / np.linalg.norm(ns)


def consistent_rhs(A, seed=7, zero=None):
    """b = A x* with a seeded random x* (zero on the unknowns ``zero``)"""
    xs = np.random.default_rng(seed).standard_normal(A.shape[1])
    if zero is not None:
        xs[zero] = 0.0
    return A @ xs


def driver_norm(r, ns, left):
    """the norm the driver stops on, without a preconditioner: ||P r|| for the left driver with a null space, else ||r||"""
    if left and ns is not None:
        r = r - ns * (ns @ r)
    return float(np.linalg.norm(r))


def deviations(A, b, ns, left, x, est, x_opt, rho):
    """The three comparisons of section 3a: the estimate against the optimum, the true residual (fp64, in the driver's norm) against the
    estimate, and the iterate against the optimal one."""
    true = driver_norm(b - A @ x, ns, left)
    return {"est": abs(est / rho - 1.0), "true": abs(true / est - 1.0), "x": float(np.linalg.norm(x - x_opt) / np.linalg.norm(x_opt))}


def tolerances(ref_dev):
    """100 times what the restatement itself shows against the same optimum, floor 1e-12: (tol for the two residual checks, tol_x)"""
    return max(100.0 * max(ref_dev["est"], ref_dev["true"]), FLOOR), max(100.0 * ref_dev["x"], FLOOR)


def field_diff(x, y):
    """largest difference per field, relative to the field's largest entry"""
    return max(float(np.abs(x[f::4] - y[f::4]).max() / np.abs(y[f::4]).max()) for f in range(4))


def permutation_runs(driver, A, Bd, b, ns, rtol, max_it, restart, seed=5, trials=3):
    """The restatement on the original ordering and on ``trials`` seeded symmetric permutations of the unknowns (same mathematics, other
    summation order): [(x in the original ordering, its, estimate, reason)]; ``Bd``: the preconditioner as a dense matrix, or None."""
    n = b.size
    rng = np.random.default_rng(seed)
    out = []
    for t in range(trials + 1):
        p = np.arange(n) if t == 0 else rng.permutation(n)
        Ap = A[p][:, p].tocsr()
        Bp = None if Bd is None else Bd[np.ix_(p, p)]
        x, it, res, reason = DRIVERS[driver](Ap, b[p], np.zeros(n), Bp, ns=None if ns is None else ns[p], rtol=rtol, max_it=max_it, restart=restart)
        xx = np.empty(n)
        xx[p] = x
        out.append((xx, it, res, reason))
    return out


def spread(runs):
    """(same iteration count in every run, largest per-field difference of x from the first run, largest relative difference of the estimate)"""
    x0, it0, res0, _ = runs[0]
    return (all(r[1] == it0 for r in runs), max(field_diff(r[0], x0) for r in runs[1:]), max(abs(r[2] / res0 - 1.0) for r in runs[1:]))


def dense_operator(B, n):
    return np.column_stack([B(e) for e in np.eye(n)])


def real_eigenpairs(A):
    """(lambda, u) of the real eigenvalues of the dense matrix, largest modulus first, u real with unit norm; near-null ones left out"""
    w, U = np.linalg.eig(A.toarray())
    big = np.abs(w).max()
    idx = np.nonzero((np.abs(w.imag) < 1e-14 * big) & (np.abs(w) > 1e-6 * big))[0]
    idx = idx[np.argsort(-np.abs(w[idx]))]
    return [(float(w[k].real), U[:, k].real / np.linalg.norm(U[:, k].real)) for k in idx]


def breakdown_rhs(A):
    """Right-hand sides in invariant subspaces of dimension 1 and 2: (lambda_1, u_1, u_1 + u_5), the eigenvectors of the largest and the
    fifth-largest real eigenvalue.  From x0 = 0 a Krylov solve ends after 1 and 2 iterations, through an exact breakdown."""
    ep = real_eigenpairs(A)
    (l1, u1), (_, u5) = ep[0], ep[4]
    return l1, u1, u1 + u5
