"""Both Krylov drivers (knp_gmres_solve, knp_fgmres_solve; csrc/knp_krylov.inc) on cycles of up to GM_MAX_RESTART = 55 iterations and on
every way a solve can end, each case on a raw backend (no solver object, no AMG) and against a statement that does not come from the
library.  Preconditions, and the power of the comparisons, in tests/test_krylov_ref_host.py.

  a. ONE cycle of exactly m iterations from x0 = 0 without a preconditioner, m at every edge of the bookkeeping kernels, against the
     minimal-residual iterate computed in long double (tests/krylov_hp_ref.py): the estimate against the optimal residual, the true
     residual (fp64 on the host, from the exported CSR) against the estimate, x against the optimal iterate.  Tolerance: 100 times the
     deviation the NumPy restatement (gmres_ref / fgmres_ref) shows from the same optimum on the same matrix, floor 1e-12 -- another
     summation order loses orthogonality at the same rate, a wrong coefficient or a dropped vector shows at 1e-3 or more.  The same with
     vertex-block Jacobi at m = 9, 17 against the restatement driven by knp_spmv / knp_pc_apply, tolerance 100 times the spread of the
     restatement over four orderings of the unknowns.
  b. converged solves over restarts, only where the host test finds the iteration count independent of the summation order.
  c. a later solve with a larger restart (the regrowth of d_gm, d_V, d_Z), and a prepare followed by a solve with another restart.
  d. endings: atol at the start and inside a cycle, a zero budget, a budget ending on and one past a cycle boundary, b = 0, NaN / Inf in
     b, NaN in x0, exact breakdown (the cancellation fallback of arnoldi_step_read), and KNP_DIVERGED_DTOL of the flexible driver; after
     each, an ordinary solve on the same context gives the bits it gave before.

Not reachable, so not tested:
  * KNP_DIVERGED_DTOL of the LEFT driver: the estimates inside a cycle never exceed the cycle's beta, the reference is the first beta of the
    solve, and beta at a restart is not tested against GM_DTOL.  (The flexible driver judges against ||b||, not the first residual: an
    initial guess far off makes the first estimate exceed 1e5 ||b|| -- that case is in d.)
  * flag 2 of givens_body (den == 0): no finite input produces it deterministically.
Not compared by count: the left driver with Jacobi at restart 55.  The estimate takes the norm of v_{j+1} from Pythagoras (w.w - h.h),
which overstates it once classical Gram-Schmidt has lost orthogonality.  Past a reduction of about 1e-7 inside one cycle the
restatement's estimate stalls at 3.4 times the threshold while the true residual is 0.4 of it, and its count is 55, 55, 33, 55 over four
orderings; the library, which loses orthogonality about five times more slowly (section a below: fused multiply-adds), crosses at 32,
where oracle/knpemi_oracle.py:gmres_left with its explicit norm does.  In c that solve is checked by its true residual and against the
bits of a context that never had a smaller workspace.

Measured on MI355X, section a, the largest over m: GPU |est/rho - 1| (= |true/est - 1| to two figures), GPU x, and the restatement's
own figures, which the tolerances are 100 times of:
  square 8   left      2.2e-7   6.6e-8    restatement 1.2e-6   3.5e-7        flexible  6.7e-8   2.1e-8    restatement 1.3e-6   3.9e-7
  square 64  left      2.0e-13  2.9e-11   restatement 8.3e-13  9.3e-11       flexible  1.0e-14  7.9e-12   restatement 9.4e-13  1.2e-10
  cube 3     left      4.1e-7   2.5e-8    restatement 3.1e-7   1.5e-8        flexible  9.6e-8   7.3e-9    restatement 6.7e-7   3.9e-8
  square 8, null space off    2.8e-8   3.1e-10   restatement 1.3e-7  1.7e-9;   Dirichlet rows  1.3e-6  2.7e-9   restatement 5.1e-7  4.0e-9
The largest deviation / tolerance over all of a: 0.033.  Jacobi, m = 9 / 17: x 3.6e-13 of a field (tolerance 2.5e-11), estimate 4.6e-7
(4.0e-4).  b: the restatement's counts (54, 39, 39, 38; flexible 112), true residual 0.87 to 0.95 of the threshold, x 1.7e-10 (7.1e-8).
The module runs in 5 s."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import irregular_meshes as IM
import krylov_cases as KC
import krylov_hp_ref as HP
from fgmres_ref import CONVERGED_ATOL, CONVERGED_RTOL, DIVERGED_DTOL, DIVERGED_ITS, DIVERGED_NANORINF
from parity_utils import ci_config, make_problem

pytestmark = pytest.mark.gpu
PC_NONE, PC_VBJACOBI = 0, 1
MARGIN = 1.05          # the true residual against the threshold: test_gpu_fgmres.MARGIN
RTOL_B = 1e-8
MAX_IT = 400           # every call: a stagnating solve ends by itself


class Ctx:
    """one raw backend with its matrix and right-hand side assembled in the perturbed state of test_gpu_parity._setup"""

    def __init__(self, kind, N, mode):
        import knpemi_oracle as K
        cfg = ci_config(N=N, steps=1, kind=kind)
        params = None
        if mode == "dirichlet":      # the configuration of test_gpu_irregular._context(dirichlet=True): every field pinned on the boundary
            cfg["dirichlet_bcs"] = True
            cfg["initial_conditions"].update({"Na_i": 10, "Na_e": 145, "K_i": 130, "K_e": 3, "Cl_i": 5, "Cl_e": 134})
            params = K.Params(ki_init=K.OracleKNPEMI.REF_DEFAULT_KI, ke_init=K.OracleKNPEMI.REF_DEFAULT_KE)
        self.p = p = make_problem(cfg)
        self.be = be = p.create_backend()
        o = (K.make_square if kind == "square" else K.make_cube)(N, models=K.CI_MODELS(), params=params)
        IM.perturb(o, p)
        p.t.value = o.p.dt
        for m in p.ionic_models:
            if hasattr(m, "update_t_mod"):
                m.update_t_mod()
        be.assemble_matrix()
        be.assemble_rhs()
        be.apply_dirichlet_rhs()
        assert (be.bc_dofs is not None) == (mode == "dirichlet")
        be.set_nullspace(mode == "ns")
        self.n = be.n_dof_owned
        assert be.n_dof_local == self.n
        self.A = be.csr()
        self.b0 = be.b.cpu().numpy().copy()
        self.ns = KC.nullspace(self.n) if mode != "dirichlet" else None      # the null vector of A; ``mode`` says whether the library uses it
        self.ns_lib = self.ns if mode == "ns" else None
        self.pc = None
        self.set_pc(PC_NONE)
        v = np.random.default_rng(11).standard_normal(self.n)
        assert np.abs(self.A_lib(v) - self.A @ v).max() <= 1e-12 * np.abs(self.A @ v).max()      # the exported CSR is what knp_spmv applies
        if self.ns is not None:
            assert np.abs(self.A @ self.ns).max() <= 1e-12 * np.abs(self.A.data).max()

    def set_pc(self, kind):
        if kind != self.pc:
            self.be.pc_setup(kind)
            self.pc = kind
            self._Bd = None

    def _dev(self, v):
        return torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device=self.be.device)

    def A_lib(self, v):
        y = torch.empty(self.n, dtype=torch.float64, device=self.be.device)
        self.be.spmv(self._dev(v), y)
        return y.cpu().numpy()

    def B_lib(self, v):
        """knp_pc_apply (with the null space on it also removes that component of its output)"""
        if self.pc == PC_NONE:
            return np.array(v, dtype=np.float64, copy=True)
        z = torch.empty(self.n, dtype=torch.float64, device=self.be.device)
        self.be.pc_apply(self._dev(v), z)
        return z.cpu().numpy()

    def Bd(self):
        """the preconditioner as a dense matrix, from n applications of knp_pc_apply (None without one)"""
        if self.pc != PC_NONE and self._Bd is None:
            self._Bd = KC.dense_operator(self.B_lib, self.n)
        return self._Bd

    def solve(self, driver, b, x0, rtol, atol=1e-50, max_it=MAX_IT, restart=30):
        """(x, its, rnorm, reason) of one call of the library's driver"""
        assert max_it <= MAX_IT
        be = self.be
        be.b.copy_(self._dev(b))
        be.x.copy_(self._dev(x0))
        its, rn, reason = (be.gmres if driver == "left" else be.fgmres)(rtol, atol, max_it, restart)
        torch.cuda.synchronize()
        return be.x.cpu().numpy().copy(), its, rn, reason

    def ref(self, driver, b, x0, rtol, atol=1e-50, max_it=MAX_IT, restart=30, lib=True):
        """the NumPy restatement, driven by the library's own operators (``lib``) or by the exported matrix (no preconditioner only)"""
        if lib:
            return KC.DRIVERS[driver](self.A_lib, b, x0, None if self.pc == PC_NONE else self.B_lib, ns=self.ns_lib, rtol=rtol, atol=atol,
                                      max_it=max_it, restart=restart)
        assert self.pc == PC_NONE
        return KC.DRIVERS[driver](self.A, b, x0, None, ns=self.ns_lib, rtol=rtol, atol=atol, max_it=max_it, restart=restart)

    def norm(self, driver, r):
        """the driver's norm of a residual r, on the host: ||P B r|| for the left driver, ||r|| for the flexible one"""
        left = driver == "left"
        return KC.driver_norm(self.B_lib(r) if left else r, self.ns_lib, left)

    def true_residual(self, driver, b, x):
        return self.norm(driver, b - self.A @ x)

    def ordinary(self, driver):
        """a plain solve with the assembled right-hand side from x0 = 0, as raw bits: what a bad ending before it must not change"""
        x, its, rn, reason = self.solve(driver, self.b0, np.zeros(self.n), 1e-8, max_it=60, restart=9)
        return its, reason, np.float64(rn).view(np.uint64), x.view(np.uint64).copy()


def _same_bits(a, b):
    return a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def contexts():
    """one context per (mesh, null-space setting): each case costs its solve and its host reference"""
    cache = {}

    def get(kind="square", N=8, mode="ns"):
        if (kind, N, mode) not in cache:
            cache[kind, N, mode] = Ctx(kind, N, mode)
        return cache[kind, N, mode]
    yield get
    cache.clear()


@pytest.fixture(scope="module")
def optima(contexts):
    """one long-double Arnoldi process per (context, driver) serves every m"""
    cache = {}

    def get(kind, N, mode, driver, ms):
        key = (kind, N, mode, driver)
        if key not in cache:
            c = contexts(kind, N, mode)
            # K.ns == false: b = A x*, consistent where the matrix is singular.  On the Dirichlet configuration the assembled right-hand
            # side is that of a steady state, and any right-hand side that is not zero on the pinned rows is dominated by them (identity
            # rows next to entries of 1e-10): nine iterations then reach rho / beta = 3e-11, the rounding floor.  x* = 0 there.
            b = c.b0 if mode == "ns" else KC.consistent_rhs(c.A, zero=c.be.bc_dofs_host)
            cache[key] = (b, HP.optimum(c.A, b, c.ns_lib, driver == "left", ms))
        return cache[key]
    return get


# ---- a. one cycle of exactly m iterations against the long-double optimum ----------------------------------------------------------
ONE_CYCLE = ([("square", 8, "ns", d, KC.MS) for d in ("left", "flex")] +
             [("square", 64, "ns", d, (9, 55)) for d in ("left", "flex")] +      # 69 reduction blocks: a second partial per lane
             [("cube", 3, "ns", d, (55,)) for d in ("left", "flex")] +
             [("square", 8, "ns_off", "left", (9, 17, 55)), ("square", 8, "dirichlet", "left", (9, 17, 55))])      # K.ns == false
ONE_CYCLE = [(k, N, mode, d, m, ms) for k, N, mode, d, ms in ONE_CYCLE for m in ms]


@pytest.mark.parametrize("kind,N,mode,driver,m,ms", ONE_CYCLE, ids=[f"{k}{N}-{mode}-{d}-m{m}" for k, N, mode, d, m, _ in ONE_CYCLE])
def test_one_cycle_reaches_the_long_double_optimum(contexts, optima, kind, N, mode, driver, m, ms):
    c = contexts(kind, N, mode)
    c.set_pc(PC_NONE)
    b, (xs, rhos, beta) = optima(kind, N, mode, driver, ms)
    left = driver == "left"
    x0 = np.zeros(c.n)
    xr, itr, estr, reasonr = c.ref(driver, b, x0, 1e-30, 1e-300, m, m, lib=False)
    ref = KC.deviations(c.A, b, c.ns_lib, left, xr, estr, xs[m], rhos[m])
    tol, tol_x = KC.tolerances(ref)
    x, its, rn, reason = c.solve(driver, b, x0, 1e-30, 1e-300, m, m)
    gpu = KC.deviations(c.A, b, c.ns_lib, left, x, rn, xs[m], rhos[m])
    print(f"{kind}{N} {mode} {driver} m={m:2d} rho/beta={rhos[m] / beta:.3e}  GPU est {gpu['est']:.2e} true {gpu['true']:.2e} (tol {tol:.2e}) "
          f"x {gpu['x']:.2e} (tol_x {tol_x:.2e})  restatement est {ref['est']:.2e} true {ref['true']:.2e} x {ref['x']:.2e}")
    assert (itr, reasonr) == (m, DIVERGED_ITS)
    assert tol <= 1e-3 and tol_x <= 1e-3      # the input keeps the cycle off the rounding floor (a wrong coefficient shows at 1e-3 or more)
    assert its == m and reason == DIVERGED_ITS
    assert gpu["est"] <= tol, gpu
    assert gpu["true"] <= tol, gpu
    assert gpu["x"] <= tol_x, gpu


def _spread_tol(c, driver, b, rtol, max_it, restart):
    """(iteration count independent of the ordering, 100 x spread of x, 100 x spread of the estimate), floors 1e-12"""
    same, sx, se = KC.spread(KC.permutation_runs(driver, c.A, c.Bd(), b, c.ns_lib, rtol, max_it, restart))
    return same, max(100.0 * sx, KC.FLOOR), max(100.0 * se, KC.FLOOR)


@pytest.mark.parametrize("driver", ["left", "flex"])
@pytest.mark.parametrize("m", [9, 17])
def test_one_cycle_with_jacobi_matches_the_restatement(contexts, m, driver):
    """The faster regime (the flexible driver keeps a separate Z with jd > 8): against the fp64 restatement on knp_spmv / knp_pc_apply."""
    c = contexts()
    c.set_pc(PC_VBJACOBI)
    b, x0 = c.b0, np.zeros(c.n)
    _, tol_x, tol_e = _spread_tol(c, driver, b, 1e-30, m, m)
    xr, itr, estr, reasonr = c.ref(driver, b, x0, 1e-30, 1e-300, m, m)
    x, its, rn, reason = c.solve(driver, b, x0, 1e-30, 1e-300, m, m)
    true, true_r = c.true_residual(driver, b, x), c.true_residual(driver, b, xr)
    tol_t = max(tol_e, 100.0 * abs(true_r / estr - 1.0))
    dx, de, dt = KC.field_diff(x, xr), abs(rn / estr - 1.0), abs(true / rn - 1.0)
    print(f"jacobi {driver} m={m}: x {dx:.2e} (tol {tol_x:.2e}) est {de:.2e} (tol {tol_e:.2e}) true/est-1 {dt:.2e} (tol {tol_t:.2e}); "
          f"est/beta {rn / c.norm(driver, b):.2e}")
    assert (itr, reasonr) == (m, DIVERGED_ITS) and its == m and reason == DIVERGED_ITS
    assert de <= tol_e and dt <= tol_t and dx <= tol_x


# ---- b. converged solves over restarts ---------------------------------------------------------------------------------------------
def _converged(c, driver, restart, label):
    """One converged solve as section b checks it; returns (x, its, rnorm) of the library."""
    b, x0 = c.b0, np.zeros(c.n)
    same, tol_x, _ = _spread_tol(c, driver, b, RTOL_B, MAX_IT, restart)
    xr, itr, estr, reasonr = c.ref(driver, b, x0, RTOL_B, 1e-50, MAX_IT, restart)
    x, its, rn, reason = c.solve(driver, b, x0, RTOL_B, 1e-50, MAX_IT, restart)
    ttol = max(RTOL_B * c.norm(driver, b), 1e-50)
    true = c.true_residual(driver, b, x)
    dx = KC.field_diff(x, xr)
    print(f"{label} {driver} restart {restart}: its {its} (restatement {itr}) reason {reason} true/ttol {true / ttol:.4f} x {dx:.2e} (tol {tol_x:.2e})")
    assert same, "the iteration count of this case depends on the summation order: not a case for this test"
    assert reasonr == CONVERGED_RTOL and reason == CONVERGED_RTOL
    assert its == itr
    assert true <= MARGIN * ttol
    assert dx <= tol_x
    return x, its, rn


@pytest.mark.parametrize("driver,restart", [("left", 3), ("left", 8), ("left", 9), ("left", 10), ("flex", 55)])
def test_converged_solves_over_restarts(contexts, driver, restart):
    c = contexts()
    c.set_pc(PC_VBJACOBI)
    _, its, _ = _converged(c, driver, restart, "converged")
    assert its > 3 * restart or restart == 55      # several cycles (restart 55: two full ones and a short one)


# ---- c. workspace growth -----------------------------------------------------------------------------------------------------------
def test_left_workspace_growth():
    """Restart 4, 55, 4 on one fresh context (d_V and d_gm regrown by the second solve): the first and third as in b and equal in their
    bits, the second against a context that starts at restart 55 (module docstring: its count is not comparable)."""
    c = Ctx("square", 8, "ns")
    c.set_pc(PC_VBJACOBI)
    x1, its1, rn1 = _converged(c, "left", 4, "growth 1")
    x2, its2, rn2, reason2 = c.solve("left", c.b0, np.zeros(c.n), RTOL_B, 1e-50, MAX_IT, 55)
    x3, its3, rn3 = _converged(c, "left", 4, "growth 3")
    assert its3 == its1 and rn3 == rn1 and np.array_equal(_bits(x3), _bits(x1))
    ttol = RTOL_B * c.norm("left", c.b0)
    true2 = c.true_residual("left", c.b0, x2)
    f = Ctx("square", 8, "ns")
    f.set_pc(PC_VBJACOBI)
    xf, itsf, rnf, reasonf = f.solve("left", f.b0, np.zeros(f.n), RTOL_B, 1e-50, MAX_IT, 55)
    itr = c.ref("left", c.b0, np.zeros(c.n), RTOL_B, 1e-50, MAX_IT, 55)[1]
    print(f"growth 2 left restart 55: its {its2} reason {reason2} true/ttol {true2 / ttol:.4f}; fresh context its {itsf}; restatement its {itr}")
    # (the true residual first meets the threshold at iteration 32, host test c; the residual recomputed at the restart ends it at 55)
    assert reason2 == CONVERGED_RTOL and true2 <= MARGIN * ttol and 32 <= its2 <= 55
    assert (its2, reason2, rn2) == (itsf, reasonf, rnf) and np.array_equal(_bits(x2), _bits(xf))


def test_flexible_workspace_growth():
    """The same for d_Z: restart 4, 55, 4 with a budget of 60 iterations per call."""
    c = Ctx("square", 8, "ns")
    c.set_pc(PC_VBJACOBI)
    b, x0 = c.b0, np.zeros(c.n)
    got = []
    for restart in (4, 55, 4):
        _, _, tol_e = _spread_tol(c, "flex", b, RTOL_B, 60, restart)
        xr, itr, estr, reasonr = c.ref("flex", b, x0, RTOL_B, 1e-50, 60, restart)
        x, its, rn, reason = c.solve("flex", b, x0, RTOL_B, 1e-50, 60, restart)
        true = c.true_residual("flex", b, x)
        print(f"flexible growth restart {restart}: its {its} reason {reason} est {abs(rn / estr - 1.0):.2e} (tol {tol_e:.2e}) true/est {true / rn:.4f}")
        assert (itr, reasonr) == (60, DIVERGED_ITS) and (its, reason) == (60, DIVERGED_ITS)
        assert abs(rn / estr - 1.0) <= tol_e
        assert abs(true / rn - 1.0) <= 0.05
        got.append((its, rn, _bits(x).copy()))
    assert got[2][0] == got[0][0] and got[2][1] == got[0][1] and np.array_equal(got[2][2], got[0][2])


def test_prepare_for_another_restart_changes_nothing(contexts):
    """knp_gmres_prepare starts ||B b|| on the side stream for the workspace's restart; a solve with another restart must discard it."""
    c = contexts()
    c.set_pc(PC_NONE)
    x0 = np.zeros(c.n)
    c.solve("left", c.b0, x0, 1e-30, 1e-300, 55, 55)                      # the workspace now holds restart 55
    plain = c.solve("left", c.b0, x0, 1e-8, 1e-50, 40, 9)
    c.be.b.copy_(c._dev(c.b0))
    c.be.gmres_prepare()
    be = c.be
    be.x.copy_(c._dev(x0))
    its, rn, reason = be.gmres(1e-8, 1e-50, 40, 9)
    torch.cuda.synchronize()
    x = be.x.cpu().numpy()
    print("prepare then restart 9:", its, rn, reason, "plain:", plain[1:])
    assert (its, rn, reason) == plain[1:] and np.array_equal(_bits(x), _bits(plain[0]))
    assert its == 40 and reason == DIVERGED_ITS


# ---- d. endings --------------------------------------------------------------------------------------------------------------------
DRIVER_PC = [(d, pc) for d in ("left", "flex") for pc in (PC_NONE, PC_VBJACOBI)]
IDS = [f"{d}-{'none' if pc == PC_NONE else 'jacobi'}" for d, pc in DRIVER_PC]


class _Unchanged:
    """``with _Unchanged(c, driver):`` -- the ordinary solve gives the same bits after the block as before it"""

    def __init__(self, c, driver):
        self.c, self.driver = c, driver

    def __enter__(self):
        self.before = self.c.ordinary(self.driver)

    def __exit__(self, et, ev, tb):
        if et is None:
            assert _same_bits(self.before, self.c.ordinary(self.driver)), "the ending left something behind in the context"
        return False


def _guess(c):
    return 0.01 * np.random.default_rng(3).standard_normal(c.n)


@pytest.mark.parametrize("driver,pc", DRIVER_PC, ids=IDS)
def test_atol_above_the_initial_residual(contexts, driver, pc):
    c = contexts()
    c.set_pc(pc)
    x0 = _guess(c)
    beta = c.true_residual(driver, c.b0, x0)
    with _Unchanged(c, driver):
        x, its, rn, reason = c.solve(driver, c.b0, x0, 1e-30, 10.0 * beta, MAX_IT, 30)
        print(driver, pc, "beta", beta, "rnorm", rn)
        assert (its, reason) == (0, CONVERGED_ATOL)
        assert np.array_equal(_bits(x), _bits(x0))
        assert abs(rn / beta - 1.0) <= 1e-12


@pytest.mark.parametrize("driver,pc", DRIVER_PC, ids=IDS)
def test_atol_inside_a_cycle(contexts, driver, pc):
    """atol between the third and the fourth estimate: CONVERGED_ATOL at iteration 4; the same threshold through rtol: CONVERGED_RTOL"""
    c = contexts()
    c.set_pc(pc)
    b, x0 = c.b0, np.zeros(c.n)
    e3, e4 = (c.ref(driver, b, x0, 1e-30, 1e-300, k, 30)[2] for k in (3, 4))
    assert e4 < (1 - 1e-6) * e3      # a gap that no summation order closes
    mid = np.sqrt(e3 * e4)
    ra = c.ref(driver, b, x0, 1e-30, mid, MAX_IT, 30)
    bnorm = c.norm(driver, b)
    with _Unchanged(c, driver):
        x, its, rn, reason = c.solve(driver, b, x0, 1e-30, mid, MAX_IT, 30)
        x2, its2, rn2, reason2 = c.solve(driver, b, x0, mid / bnorm, 1e-300, MAX_IT, 30)
        print(driver, pc, "e3", e3, "e4", e4, "atol", mid, "->", its, rn, reason, "| rtol ->", its2, rn2, reason2)
        assert ra[1] == 4 and ra[3] == CONVERGED_ATOL
        assert (its, reason) == (4, CONVERGED_ATOL) and rn <= mid
        assert (its2, reason2) == (4, CONVERGED_RTOL)
        assert np.array_equal(_bits(x), _bits(x2))


@pytest.mark.parametrize("driver,pc", DRIVER_PC, ids=IDS)
def test_zero_budget(contexts, driver, pc):
    c = contexts()
    c.set_pc(pc)
    x0 = _guess(c)
    beta = c.true_residual(driver, c.b0, x0)
    with _Unchanged(c, driver):
        x, its, rn, reason = c.solve(driver, c.b0, x0, 1e-10, 1e-50, 0, 30)
        assert (its, reason) == (0, DIVERGED_ITS)
        assert np.array_equal(_bits(x), _bits(x0))
        assert abs(rn / beta - 1.0) <= 1e-12


@pytest.mark.parametrize("driver,pc", DRIVER_PC, ids=IDS)
@pytest.mark.parametrize("restart,extra", [(8, 0), (8, 1), (9, 0), (9, 1)])
def test_budget_on_and_past_a_cycle_boundary(contexts, driver, pc, restart, extra):
    """max_it = restart ends with the cycle's update, restart + 1 in a one-column update after a full cycle"""
    c = contexts()
    c.set_pc(pc)
    b, x0, max_it = c.b0, np.zeros(c.n), restart + extra
    _, tol_x, _ = _spread_tol(c, driver, b, 1e-30, max_it, restart)
    xr, itr, _, reasonr = c.ref(driver, b, x0, 1e-30, 1e-300, max_it, restart)
    with _Unchanged(c, driver):
        x, its, rn, reason = c.solve(driver, b, x0, 1e-30, 1e-300, max_it, restart)
        dx = KC.field_diff(x, xr)
        print(driver, pc, restart, max_it, "x", dx, "tol", tol_x)
        assert (itr, reasonr) == (max_it, DIVERGED_ITS) and (its, reason) == (max_it, DIVERGED_ITS)
        assert dx <= tol_x


@pytest.mark.parametrize("driver,pc", DRIVER_PC, ids=IDS)
def test_zero_right_hand_side(contexts, driver, pc):
    c = contexts()
    c.set_pc(pc)
    with _Unchanged(c, driver):
        x, its, rn, reason = c.solve(driver, np.zeros(c.n), np.zeros(c.n), 1e-10, 1e-50, MAX_IT, 30)
        assert (its, reason) == (0, CONVERGED_ATOL) and rn == 0.0
        assert not x.any()


@pytest.mark.parametrize("driver,pc", DRIVER_PC, ids=IDS)
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_right_hand_side(contexts, driver, pc, bad):
    c = contexts()
    c.set_pc(pc)
    b, x0 = c.b0.copy(), _guess(c)
    b[c.n // 2 + 1] = bad
    with _Unchanged(c, driver):
        x, its, rn, reason = c.solve(driver, b, x0, 1e-10, 1e-50, MAX_IT, 30)
        assert (its, reason) == (0, DIVERGED_NANORINF)
        assert np.array_equal(_bits(x), _bits(x0))


@pytest.mark.parametrize("driver,pc", DRIVER_PC, ids=IDS)
def test_nan_in_the_initial_guess(contexts, driver, pc):
    c = contexts()
    c.set_pc(pc)
    x0 = _guess(c)
    x0[c.n // 2 + 2] = np.nan
    with _Unchanged(c, driver):
        x, its, rn, reason = c.solve(driver, c.b0, x0, 1e-10, 1e-50, MAX_IT, 30)
        assert (its, reason) == (0, DIVERGED_NANORINF)
        assert np.array_equal(_bits(x), _bits(x0))      # the NaN included


@pytest.mark.parametrize("driver", ["left", "flex"])
def test_exact_breakdown(contexts, driver):
    """b in an invariant subspace of dimension 1 and 2 (eigenvectors of the exported matrix): w is a combination of the basis, Pythagoras
    cancels, the explicit norm of arnoldi_step_read takes over and the solve ends converged after 1 and 2 iterations."""
    c = contexts()
    c.set_pc(PC_NONE)
    lam, u1, u12 = KC.breakdown_rhs(c.A)
    assert abs(c.ns @ u1) <= 1e-12
    x0 = np.zeros(c.n)
    for b, n_it in ((u1, 1), (u12, 2)):
        xr, itr, _, reasonr = c.ref(driver, b, x0, 1e-10, 1e-50, 50, 30, lib=False)
        with _Unchanged(c, driver):
            before = c.be.stats()["norm_fallbacks"]
            x, its, rn, reason = c.solve(driver, b, x0, 1e-10, 1e-50, 50, 30)
            after = c.be.stats()["norm_fallbacks"]
            true = c.true_residual(driver, b, x)
            print(driver, "subspace of dimension", n_it, "its", its, "reason", reason, "rnorm", rn, "true", true, "fallbacks", after - before)
            assert (itr, reasonr) == (n_it, CONVERGED_RTOL)
            assert reason > 0 and its == n_it
            assert true <= MARGIN * 1e-10 * np.linalg.norm(b)
            assert after > before
            if n_it == 1:
                assert np.linalg.norm(lam * x - u1) <= 1e-10 * np.linalg.norm(u1)


def test_flexible_divergence_tolerance(contexts):
    """The flexible driver judges divergence against ||b||: from a guess with ||b - A x0|| > 1e5 ||b|| the first estimate, which a step
    without a preconditioner lowers by a few per cent only, is past the tolerance.  One iteration, two reductions of 388 terms."""
    c = contexts()
    c.set_pc(PC_NONE)
    g = np.random.default_rng(9).standard_normal(c.n)
    g -= c.ns * (c.ns @ g)
    x0 = g * (1e7 * np.linalg.norm(c.b0) / np.linalg.norm(c.A @ g))
    xr, itr, estr, reasonr = c.ref("flex", c.b0, x0, 1e-10, 1e-50, MAX_IT, 30, lib=False)
    with _Unchanged(c, "flex"):
        x, its, rn, reason = c.solve("flex", c.b0, x0, 1e-10, 1e-50, MAX_IT, 30)
        print("dtol: its", its, "reason", reason, "rnorm/||b||", rn / np.linalg.norm(c.b0), "restatement", itr, reasonr, estr / np.linalg.norm(c.b0))
        assert (itr, reasonr) == (1, DIVERGED_DTOL)
        assert (its, reason) == (1, DIVERGED_DTOL)
        assert abs(rn / estr - 1.0) <= 1e-10
        assert KC.field_diff(x, xr) <= 1e-10
