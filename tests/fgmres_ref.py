"""NumPy restatement of the library's flexible GMRES (knp_fgmres_solve): the checker of the GPU tests and the subject of the CPU ones.

FGMRES(restart) with classical Gram-Schmidt (one reduction: the norm of the orthogonalised vector by Pythagoras, an explicit norm only
when that cancels), right preconditioning with a preconditioner that may change from one application to the next (z_j = M(v_j) is
kept), Givens rotations, and PETSc's KSPConvergedDefault on the TRUE residual: stop when |g_{j+1}| <= max(rtol ||b||, atol), divergence
when it exceeds 1e5 ||b||.  Gauge step: with a null-space vector ``ns`` (unit norm, A ns = 0) each cycle's correction Z y is added without
its component along ns, so x keeps the null-space component of the initial guess."""
from __future__ import annotations

import numpy as np

CONVERGED_RTOL, CONVERGED_ATOL, DIVERGED_ITS, DIVERGED_DTOL, DIVERGED_NANORINF = 2, 3, -3, -4, -9
GM_CANCEL = 1e-8


def fgmres(A, b, x0, M=None, ns=None, rtol=1e-9, atol=1e-50, max_it=5000, restart=30):
    """A, M: callables (vector -> vector) or matrices; M None = no preconditioner.  Returns (x, iterations, residual estimate, reason)."""
    Aop = A if callable(A) else (lambda v: A @ v)
    Mop = (lambda v: v.copy()) if M is None else (M if callable(M) else (lambda v: M @ v))
    x = np.array(x0, dtype=np.float64, copy=True)
    n = b.size
    bnorm = float(np.linalg.norm(b))
    ttol = max(rtol * bnorm, atol)
    dtol = 1e5 * (bnorm if bnorm > 0 else 1.0)
    V = np.zeros((restart + 1, n))
    Z = np.zeros((restart, n))
    it = 0
    while True:
        r = b - Aop(x)
        beta = float(np.linalg.norm(r))
        if not np.isfinite(beta):
            return x, it, beta, DIVERGED_NANORINF
        if beta <= ttol:
            return x, it, beta, CONVERGED_ATOL if beta <= atol else CONVERGED_RTOL
        if it >= max_it:
            return x, it, beta, DIVERGED_ITS
        V[0] = r / beta
        H = np.zeros((restart + 1, restart))
        cs, sn = np.zeros(restart), np.zeros(restart)
        g = np.zeros(restart + 1)
        g[0] = beta
        jd, reason, res = 0, 0, beta
        for j in range(restart):
            Z[j] = Mop(V[j])
            w = Aop(Z[j])
            h = V[:j + 1] @ w                        # classical Gram-Schmidt: all coefficients from the same w
            ww = float(w @ w)
            vn = w - h @ V[:j + 1]
            nrm2 = ww - float(h @ h)
            if not (nrm2 > GM_CANCEL * ww) and ww > 0:
                nrm2 = float(vn @ vn)                # cancellation: explicit norm
            hn = np.sqrt(max(nrm2, 0.0))
            col = np.concatenate([h, [hn]])
            for i in range(j):
                t = cs[i] * col[i] + sn[i] * col[i + 1]
                col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1]
                col[i] = t
            den = np.hypot(col[j], col[j + 1])
            if not (den > 0) or not np.isfinite(den):
                reason = DIVERGED_NANORINF
                break
            cs[j], sn[j] = col[j] / den, col[j + 1] / den
            col[j], col[j + 1] = den, 0.0
            H[:j + 2, j] = col
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            res = abs(g[j + 1])
            V[j + 1] = vn / (hn if hn > 0 else 1.0)
            it += 1
            jd = j + 1
            if res <= ttol:
                reason = CONVERGED_ATOL if res <= atol else CONVERGED_RTOL
                break
            if it >= max_it:
                reason = DIVERGED_ITS
                break
            if res > dtol:
                reason = DIVERGED_DTOL
                break
        if jd > 0:
            y = np.linalg.solve(np.triu(H[:jd, :jd]), g[:jd])
            c = y @ Z[:jd]
            if ns is not None:
                c = c - ns * float(ns @ c)
            x += c
        if reason != 0:
            return x, it, res, reason
