"""NumPy restatement of the library's left-preconditioned GMRES (knp_gmres_solve): the checker of the GPU tests and the subject of the CPU
ones, in the style of tests/fgmres_ref.py and with the same reason codes.

GMRES(restart) on B A x = B b with classical Gram-Schmidt and ONE reduction per iteration: the coefficients V_i.w, the coefficient of w
along the null-space vector ``ns`` (unit norm, A ns = 0), which takes part in the pass as one more vector, and w.w; the norm of the
orthogonalised vector follows by Pythagoras, an explicit norm only when that cancels (below GM_CANCEL of w.w).  The norm of a
preconditioned residual is taken the same way, z.z - (ns.z)^2 with the explicit projection as its fallback.  Stop on
|g_{j+1}| <= max(rtol ||P B b||, atol) (P = I - ns ns^T); divergence is judged against the first preconditioned residual of the solve.
``oracle/knpemi_oracle.py:gmres_left`` is the same method without reasons and without the fallback."""
from __future__ import annotations

import numpy as np

from fgmres_ref import CONVERGED_ATOL, CONVERGED_RTOL, DIVERGED_DTOL, DIVERGED_ITS, DIVERGED_NANORINF, GM_CANCEL

GM_DTOL = 1e5


def _projected(z, ns):
    """(P z, ||P z||): Pythagoras, the explicit norm when it cancels"""
    zz = float(z @ z)
    if ns is None:
        return z, np.sqrt(zz)
    s = float(ns @ z)
    pz = z - ns * s
    nrm2 = zz - s * s
    if not (nrm2 > GM_CANCEL * zz) and zz > 0:
        nrm2 = float(pz @ pz)
    return pz, np.sqrt(max(nrm2, 0.0)) if np.isfinite(nrm2) else float("nan")


def gmres(A, b, x0, M=None, ns=None, rtol=1e-9, atol=1e-50, max_it=5000, restart=30):
    """A, M: callables (vector -> vector) or matrices; M None = no preconditioner.  Returns (x, iterations, residual estimate, reason)."""
    Aop = A if callable(A) else (lambda v: A @ v)
    Mop = (lambda v: v.copy()) if M is None else (M if callable(M) else (lambda v: M @ v))
    x = np.array(x0, dtype=np.float64, copy=True)
    n = b.size
    bnorm = _projected(Mop(b), ns)[1]
    if not np.isfinite(bnorm):
        return x, 0, bnorm, DIVERGED_NANORINF
    ttol = max(rtol * bnorm, atol)
    nv = 0 if ns is None else 1
    V = np.zeros((restart + 1 + nv, n))          # the last row: ns, the extra vector of the Gram-Schmidt pass
    if nv:
        V[restart + 1] = ns
    it, res0 = 0, None
    while True:
        r, beta = _projected(Mop(b - Aop(x)), ns)
        if res0 is None:
            res0 = beta
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
            w = Mop(Aop(V[j]))
            rows = np.r_[0:j + 1, restart + 1:restart + 1 + nv]
            hx = V[rows] @ w                         # classical Gram-Schmidt: every coefficient from the same w, ns included
            ww = float(w @ w)
            vn = w - hx @ V[rows]
            nrm2 = ww - float(hx @ hx)
            if not (nrm2 > GM_CANCEL * ww) and ww > 0:
                nrm2 = float(vn @ vn)                # cancellation: explicit norm
            hn = np.sqrt(max(nrm2, 0.0))
            col = np.concatenate([hx[:j + 1], [hn]])
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
            if res > GM_DTOL * res0:
                reason = DIVERGED_DTOL
                break
        if jd > 0:
            y = np.linalg.solve(np.triu(H[:jd, :jd]), g[:jd])
            x += y @ V[:jd]
        if reason != 0:
            return x, it, res, reason
