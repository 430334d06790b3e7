"""Preconditions of tests/test_gpu_krylov_long.py, on the CPU with the oracle's matrices (no GPU):

  a. the two NumPy restatements (tests/gmres_ref.py, tests/fgmres_ref.py) against the long-double optimum of one cycle
     (tests/krylov_hp_ref.py) at every cycle length the GPU tests use: the "reference alone" that the GPU tolerances are 100 times of;
  b. the power of that comparison: a copy of the restatement with ONE wrong Gram-Schmidt coefficient, and one with ONE entry of y left
     out of the update, miss the checks by more than 100 times their tolerance;
  c. which converged solves may be compared by iteration count: the same count on four orderings of the unknowns, estimates well away
     from the threshold;
  d. right-hand sides in invariant subspaces of dimension 1 and 2 end both restatements after 1 and 2 iterations.

Measured (oracle matrices in the perturbed state, b as assembled, no preconditioner), restatement against the optimum, left / flexible:
  square 8   (388 unknowns):  est/rho - 1 <= 1.5e-12 / 2.8e-13 up to m = 17, 8.6e-7 / 1.6e-7 at m = 55;  ||x - x_m|| / ||x_m|| <= 2.7e-7
  cube 3     (288 unknowns):  est/rho - 1 = 5.6e-7 / 5.9e-7 at m = 55;                                   ||x - x_m|| / ||x_m|| <= 3.5e-8
  square 64  (17 412 unknowns), m = 55: est/rho - 1 = 9.5e-13 / 1.2e-12;                                 ||x - x_m|| / ||x_m|| <= 1.8e-10
(|true/est - 1| equals the first figure in every case: the iterate is optimal to the third figure, the estimate is what classical
Gram-Schmidt's loss of orthogonality moves.)  Mutants at m = 33 / 55, b = A x*: one zeroed coefficient moves the estimate by 0.76 / 0.50,
the true residual against it by 3.5 / 5.5 and x by 1.8e-3 / 0.57; one y_i left out moves the true residual by 1.5e2 / 6.9e3 and x by
2.0e-2 / 0.21, against tolerances of at most 4.4e-5 (residuals) and 7.2e-8 (x)."""
from __future__ import annotations

import numpy as np
import pytest

import irregular_meshes as IM
import krylov_cases as KC
import krylov_hp_ref as HP
from fgmres_ref import CONVERGED_RTOL, DIVERGED_ITS, GM_CANCEL, fgmres
from gmres_ref import gmres
from parity_utils import make_oracle

# 100 times this is the most a GPU tolerance may be: the 1e-3 at which the least visible effect of a wrong coefficient shows (b).  The
# deviation itself is the loss of orthogonality of classical Gram-Schmidt, which the summation order of the BLAS at hand moves by a
# factor of up to ten (1.5e-7 to 1.3e-6 seen for the same case on two machines)
REF_ALONE_MAX = 1e-5
CASES_A = [("square", 8, KC.MS), ("square", 64, (9, 55)), ("cube", 3, (55,))]


@pytest.fixture(scope="module")
def systems():
    """(A, b, ns, layout) of the oracle in the perturbed state of test_gpu_parity._setup, one per mesh"""
    cache = {}

    def get(kind, N):
        if (kind, N) not in cache:
            o = make_oracle(N, kind)
            IM.perturb(o)
            A = o.assemble_A().tocsr()
            A.sort_indices()
            cache[kind, N] = (A, o.assemble_b(), o.nullspace(), o.lay)
        return cache[kind, N]
    return get


@pytest.fixture(scope="module")
def optima(systems):
    """one long-double Arnoldi process per (mesh, driver, right-hand side) serves every m"""
    cache = {}

    def get(kind, N, left, ms, rhs="assembled"):
        key = (kind, N, left, rhs)
        if key not in cache:
            A, b, ns, _ = systems(kind, N)
            if rhs != "assembled":
                b = KC.consistent_rhs(A)
            cache[key] = (b, HP.optimum(A, b, ns, left, ms))
        assert set(ms) <= set(cache[key][1][0])
        return cache[key]
    return get


# ---- a. the restatements against the optimum ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("left", [True, False], ids=["left", "flex"])
@pytest.mark.parametrize("kind,N,ms", CASES_A, ids=[f"{k}{n}" for k, n, _ in CASES_A])
def test_restatements_reach_the_long_double_optimum(systems, optima, kind, N, ms, left):
    A, _, ns, _ = systems(kind, N)
    b, (xs, rhos, beta) = optima(kind, N, left, ms)
    drv = gmres if left else fgmres
    for m in ms:
        x, it, est, reason = drv(A, b, np.zeros(b.size), None, ns=ns, rtol=1e-30, atol=1e-300, max_it=m, restart=m)
        d = KC.deviations(A, b, ns, left, x, est, xs[m], rhos[m])
        print(f"{kind}{N} {'left' if left else 'flex'} m={m:2d} rho/beta={rhos[m] / beta:.3e} est/rho-1={d['est']:.2e} "
              f"true/est-1={d['true']:.2e} |x-x_m|/|x_m|={d['x']:.2e}")
        assert it == m and reason == DIVERGED_ITS
        assert rhos[m] > 1e-3 * beta                 # far from the rounding floor: the residual falls by 1-70 % per cycle
        assert max(d.values()) <= REF_ALONE_MAX, (m, d)


# ---- b. the power of the comparison ------------------------------------------------------------------------------------------------
def _one_cycle(A, b, ns, left, m, zero_h=None, drop_y=None):
    """A copy of one cycle of the restatements from x0 = 0 without a preconditioner (both drivers: ``left`` puts ns into the Gram-Schmidt
    pass, the flexible form projects the correction), with two places to break it: ``zero_h = (j, i)`` zeroes coefficient i of iteration
    j as it comes out of the reduction, ``drop_y = i`` leaves y_i V_i out of the update.  Returns (x, estimate)."""
    n = b.size
    ext = ns is not None and left
    r = b - ns * (ns @ b) if ext else b.copy()
    beta = float(np.linalg.norm(r))
    V = np.zeros((m + 2, n))
    V[0] = r / beta
    if ext:
        V[m + 1] = ns
    H = np.zeros((m + 1, m))
    cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
    g[0] = beta
    for j in range(m):
        w = A @ V[j]
        rows = np.r_[0:j + 1, m + 1:m + 1 + int(ext)]
        hx = V[rows] @ w
        if zero_h is not None and zero_h[0] == j:
            hx[zero_h[1]] = 0.0
        ww = float(w @ w)
        vn = w - hx @ V[rows]
        nrm2 = ww - float(hx @ hx)
        if not (nrm2 > GM_CANCEL * ww) and ww > 0:
            nrm2 = float(vn @ vn)
        hn = np.sqrt(max(nrm2, 0.0))
        col = np.concatenate([hx[:j + 1], [hn]])
        for i in range(j):
            t = cs[i] * col[i] + sn[i] * col[i + 1]
            col[i + 1] = -sn[i] * col[i] + cs[i] * col[i + 1]
            col[i] = t
        den = np.hypot(col[j], col[j + 1])
        cs[j], sn[j] = col[j] / den, col[j + 1] / den
        col[j], col[j + 1] = den, 0.0
        H[:j + 2, j] = col
        g[j + 1] = -sn[j] * g[j]
        g[j] = cs[j] * g[j]
        V[j + 1] = vn / hn
    y = np.linalg.solve(np.triu(H[:m, :m]), g[:m])
    if drop_y is not None:
        y[drop_y] = 0.0
    c = y @ V[:m]
    if ns is not None and not left:
        c = c - ns * float(ns @ c)
    return c, abs(g[m])


@pytest.mark.parametrize("left", [True, False], ids=["left", "flex"])
@pytest.mark.parametrize("m", [33, 55])
def test_one_wrong_coefficient_misses_every_check(systems, optima, m, left):
    """b = A x* with a seeded random x*: every Hessenberg entry and every y_i carries weight, so one wrong value moves all three
    quantities.  (The residual estimate is fixed before y is formed: leaving y_i out cannot move est/rho, and is asserted not to; it
    shows in the other two.)"""
    A, _, ns, _ = systems("square", 8)
    b, (xs, rhos, _) = optima("square", 8, left, (33, 55), rhs="consistent")
    drv = gmres if left else fgmres
    x, it, est, _ = drv(A, b, np.zeros(b.size), None, ns=ns, rtol=1e-30, atol=1e-300, max_it=m, restart=m)
    xc, estc = _one_cycle(A, b, ns, left, m)
    assert np.array_equal(x, xc) and est == estc          # the copy IS the restatement
    ref = KC.deviations(A, b, ns, left, x, est, xs[m], rhos[m])
    tol, tol_x = KC.tolerances(ref)
    print(f"m={m} restatement {ref} tol {tol:.2e} tol_x {tol_x:.2e}")
    assert max(ref.values()) <= REF_ALONE_MAX
    xh, esth = _one_cycle(A, b, ns, left, m, zero_h=(20, 16))
    dh = KC.deviations(A, b, ns, left, xh, esth, xs[m], rhos[m])
    xy, esty = _one_cycle(A, b, ns, left, m, drop_y=m // 2)
    dy = KC.deviations(A, b, ns, left, xy, esty, xs[m], rhos[m])
    print(f"  h[16] of iteration 20 zeroed: {dh}\n  y[{m // 2}] left out: {dy}")
    assert dh["est"] > 100 * tol and dh["true"] > 100 * tol and dh["x"] > 100 * tol_x, dh
    assert dy["true"] > 100 * tol and dy["x"] > 100 * tol_x, dy
    assert esty == est


# ---- c. which converged solves may be compared by iteration count ------------------------------------------------------------------
RTOL_C = 1e-8
ELIGIBLE = [("left", 3, 54), ("left", 4, None), ("left", 8, 39), ("left", 9, 39), ("left", 10, 38), ("flex", 55, 112)]


@pytest.fixture(scope="module")
def jacobi8(systems):
    import knpemi_oracle as K
    A, b, ns, lay = systems("square", 8)
    return KC.dense_operator(K.pc_vertex_block_jacobi(lay)(A), b.size)


@pytest.mark.parametrize("driver,restart,its", ELIGIBLE, ids=[f"{d}{r}" for d, r, _ in ELIGIBLE])
def test_converged_cases_are_eligible(systems, jacobi8, driver, restart, its):
    A, b, ns, _ = systems("square", 8)
    runs = KC.permutation_runs(driver, A, jacobi8, b, ns, RTOL_C, 400, restart)
    same, sx, _ = KC.spread(runs)
    x, it, res, reason = runs[0]
    left = driver == "left"
    rhs = jacobi8 @ b if left else b
    ttol = RTOL_C * KC.driver_norm(rhs, ns, left)
    r = b - A @ x
    true = KC.driver_norm(jacobi8 @ r if left else r, ns, left)
    # the estimate one iteration earlier: the same solve stopped by its budget
    prev = KC.DRIVERS[driver](A, b, np.zeros(b.size), jacobi8, ns=ns, rtol=RTOL_C, max_it=it - 1, restart=restart)
    print(f"{driver} restart {restart}: its {[r_[1] for r_ in runs]} spread {sx:.2e} est/ttol {res / ttol:.4f} before {prev[2] / ttol:.4f} "
          f"true/ttol {true / ttol:.4f}")
    assert reason == CONVERGED_RTOL and same and it == (its or it)
    assert prev[1] == it - 1 and prev[3] == DIVERGED_ITS
    assert res <= (1 - 1e-3) * ttol and prev[2] >= (1 + 1e-3) * ttol
    assert true <= 1.05 * ttol
    assert sx <= 1e-8          # 100 times the spread stays far below the 1e-3 of a wrong coefficient


def test_cases_that_are_not_eligible(systems, jacobi8):
    """Why the GPU file compares no iteration count there.  The flexible driver at short restarts stagnates on the unpreconditioned norm
    and runs into the budget; on cube 3 summation order alone moves the flexible count; and the LEFT driver at restart 55 stops on an
    estimate that Pythagoras (w.w - h.h) overstates once classical Gram-Schmidt has lost orthogonality: it stalls above the threshold
    while the true residual is below it, and which iteration it crosses at depends on the ordering (gmres_left, with an explicit norm
    of v_{j+1}, takes 32 iterations in all four)."""
    import knpemi_oracle as K
    A, b, ns, _ = systems("square", 8)
    for restart in (3, 10):
        assert fgmres(A, b, np.zeros(b.size), jacobi8, ns=ns, rtol=RTOL_C, max_it=400, restart=restart)[3] == DIVERGED_ITS
    runs = KC.permutation_runs("left", A, jacobi8, b, ns, RTOL_C, 400, 55)
    same, sx, _ = KC.spread(runs)
    ttol = RTOL_C * KC.driver_norm(jacobi8 @ b, ns, True)
    x40, _, est40, _ = gmres(A, b, np.zeros(b.size), jacobi8, ns=ns, rtol=1e-30, max_it=40, restart=55)
    true40 = KC.driver_norm(jacobi8 @ (b - A @ x40), ns, True)
    xo, ito, _ = K.gmres_left(A, b, np.zeros(b.size), lambda r: jacobi8 @ r, ns=ns, rtol=RTOL_C, max_it=400, restart=55)
    print("left restart 55: its", [r[1] for r in runs], "spread", sx, "iteration 40: est/ttol", est40 / ttol, "true/ttol", true40 / ttol,
          "gmres_left", ito)
    assert not same or sx > 1e-8
    assert est40 > 2.0 * ttol and true40 < ttol
    assert all(r[3] == CONVERGED_RTOL and r[1] <= 55 for r in runs)      # ... and a restart, which recomputes the residual, ends it
    A, b, ns, lay = systems("cube", 3)
    Bd = KC.dense_operator(K.pc_vertex_block_jacobi(lay)(A), b.size)
    same, sx, _ = KC.spread(KC.permutation_runs("flex", A, Bd, b, ns, RTOL_C, 400, 55))
    print("cube 3 flexible restart 55: same count", same, "spread", sx)
    assert not same or sx > 1e-8


# ---- d. the breakdown inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("left", [True, False], ids=["left", "flex"])
def test_invariant_subspaces_end_in_one_and_two_iterations(systems, left):
    A, _, ns, _ = systems("square", 8)
    ep = KC.real_eigenpairs(A)
    lam, u1, u12 = KC.breakdown_rhs(A)
    print("real eigenvalues", len(ep), "of", A.shape[0], "ns.u", ns @ u1)
    assert len(ep) >= 300 and abs(ns @ u1) <= 1e-12
    drv = gmres if left else fgmres
    for b, its in ((u1, 1), (u12, 2)):
        x, it, res, reason = drv(A, b, np.zeros(b.size), None, ns=ns, rtol=1e-10, max_it=50, restart=30)
        true = KC.driver_norm(b - A @ x, ns, left)
        print("its", it, "reason", reason, "est", res, "true", true)
        assert it == its and reason == CONVERGED_RTOL
        assert true <= 1.05 * 1e-10 * np.linalg.norm(b)
    x = drv(A, u1, np.zeros(u1.size), None, ns=ns, rtol=1e-10, max_it=50, restart=30)[0]
    assert np.linalg.norm(lam * x - u1) <= 1e-10
