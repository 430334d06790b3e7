"""The exact minimal-residual iterate of one GMRES cycle from x0 = 0, in ``np.longdouble`` and matrix-free: what both Krylov drivers
approximate after m iterations without a preconditioner, whatever their bookkeeping.

One Arnoldi process (modified Gram-Schmidt applied twice) builds V_1..V_mmax of K(P A, P b); W = P A V is orthogonalised once more
(again twice) into Q R, and every m <= mmax is read off the prefixes: y_m = R_m^-1 Q_m^T r0, x_m = V_m y_m, rho_m = ||r0 - W_m y_m||
= min ||P (b - A x)|| over the Krylov space.  The matrix entries are fp64 values, so the long-double CSR product is exact up to its
summation.  ``left`` with a null-space vector ns: P = I - ns ns^T (the left driver's norm); otherwise P = I, and with ns given x_m is
returned without its component along ns (the flexible driver's gauge step)."""
from __future__ import annotations

import numpy as np

LD = np.longdouble


def ld_matvec(A):
    """v -> A v in long double on the CSR arrays of ``A`` (every row must hold at least one entry, as every row of these matrices does)"""
    d, ci, rp = A.data.astype(LD), A.indices, A.indptr
    assert np.all(np.diff(rp) > 0)
    return lambda v: np.add.reduceat(d * v[ci], rp[:-1])


def _mgs2(w, basis, coef=None):
    for _ in range(2):
        for i, q in enumerate(basis):
            c = q @ w
            w = w - q * c
            if coef is not None:
                coef[i] += c
    return w


def optimum(A, b, ns=None, left=True, ms=(55,)):
    """Returns ({m: x_m}, {m: rho_m}, beta) for the m in ``ms``, as float64 arrays and floats: one process of max(ms) vectors serves all."""
    mmax = max(ms)
    mv = ld_matvec(A)
    nsl = None if ns is None else ns.astype(LD)
    P = (lambda z: z - nsl * (nsl @ z)) if (left and ns is not None) else (lambda z: z)
    r0 = P(b.astype(LD))
    beta = np.sqrt(r0 @ r0)
    V, W = [r0 / beta], []
    for j in range(mmax):
        w = P(mv(V[j]))
        W.append(w)
        w = _mgs2(w.copy(), V)
        V.append(w / np.sqrt(w @ w))
    Q, R = [], np.zeros((mmax, mmax), LD)
    for j in range(mmax):
        col = np.zeros(j, LD)
        q = _mgs2(W[j].copy(), Q, col)
        R[:j, j] = col
        R[j, j] = np.sqrt(q @ q)
        Q.append(q / R[j, j])
    c = np.array([q @ r0 for q in Q])
    xs, rhos = {}, {}
    for m in sorted(set(ms)):
        y = np.zeros(m, LD)
        for i in range(m - 1, -1, -1):
            y[i] = (c[i] - R[i, i + 1:m] @ y[i + 1:]) / R[i, i]
        x = sum(yi * v for yi, v in zip(y, V[:m]))
        if not left and ns is not None:
            x = x - nsl * (nsl @ x)
        res = r0 - sum(yi * w for yi, w in zip(y, W[:m]))
        xs[m] = np.asarray(x, np.float64)
        rhos[m] = float(np.sqrt(res @ res))
    return xs, rhos, float(beta)
