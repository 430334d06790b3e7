"""The stages of ``pc_apply_proj`` (csrc/knp_kernels.hip) behind the preconditioner B -- the Dirichlet copy (k_bc_copy), the deflation
correction z += Z Einv Z^T r (k_defl_sums<8> -> k_reduce_partials -> k_defl_add) and the gauge projection (k_phi_sum ->
k_reduce_partials -> k_phi_sub) -- against the long-double reference of tests/pc_tail_ref.py, whose inputs
tests/test_pc_tail_host.py shows to be well-posed and sensitive to six ways a kernel could be subtly wrong.  Deflation is set through
the C ABI (``knp_set_deflation``) on one GPU: the Python layer sets it on several ranks only.

  a. the bare tail behind KNP_PC_NONE (z_plain = r): m = 1, 7, 8, 9, 32 modes x six node_mode patterns x null space off / on, on the
     672 nodes of delaunay2d_24 and the 608 of delaunay3d_7 (three blocks of 256, the last partial);
  b. behind vbjacobi, hypre, btcc (fp64 and fp32 storage): z_plain from the library with deflation and null space off, the path
     tests/test_gpu_irregular.py checks against the NumPy cycle -- the sums are taken from r before a cycle may overwrite it;
  c. with Dirichlet rows, pinned potential rows out of the modes (what cgx_hip.backend passes) and inside one (include/knpemi_hip.h:
     such a row receives the correction);
  d. the ABI: what knp_set_deflation rejects, that a rejected call changes nothing, switching off, replacing;
  e. the in-order branches of both Krylov drivers that deflation forces on one GPU (plain norm sequence, no enqueue-ahead, no
     reduction folded into the cycle, no fused tail), against the NumPy drivers on the library's own operators.

Tolerance of a-c: 1e-13 bound[n], bound[n] = sum_c |Einv[mode(n), c]| sum_{mode c} |r_phi| + |z_plain_phi[n]| (+ mean |z_phi| with the
null space on).  Per entry: one rounding per level of the 64-lane tree (6), of the wave tree of a block (2) and of the tree over the
block partial sums (<= 8 + 2), a few per-thread terms, the 32-term dot of k_defl_add, the addition, and the same again for the mean and
its subtraction: about 50 roundings of 2^-53, 6e-15.  1e-13 is the project's tolerance for sums of this length (the sampling and gather
tests) and leaves a factor of 15.  Ion entries, and without the null space the potential entries outside every mode, are copies: bit
for bit.  Nothing here iterates except e, which ends on its budget of 12 iterations.

The grid-stride trip of these kernels starts beyond 1024 x 256 nodes; it is left to tests/test_gpu_fullsize.py and is out of scope.

Measured on MI355X (largest |z - ref| / bound per part; iterations and residuals of e):
  a. 3.6e-16 (delaunay3d_7, m = 8, single_node, null space on); null space off at most 1.2e-16;
  b. 1.6e-16 (delaunay3d_7, vbjacobi, null space on); null space off at most 4.1e-17;  c. 1.9e-16;  d. 1.2e-16;
  e. every solve: 12 iterations, KNP_DIVERGED_ITS, 16 read-backs with and without deflation, no norm fallback, fused_dots = fused_tails = 0.
     Residual estimate over the reference norm after 12 iterations (the same 4 digits from the NumPy driver), and the largest
     |x - x_numpy| / max |x_numpy| over the four fields:
       square32-hypre  fgmres 3.637e-08 (without deflation 1.185e-09), 2.1e-12;   gmres 4.179e-10 (5.143e-11), 1.0e-12
       cube8-btcc      fgmres 4.432e-06 (8.085e-09), 1.3e-10;                     gmres 2.177e-07 (6.546e-10), 1.4e-12
     B multiplies the potential entries of a random r by 3.9e13 (square32-hypre) and 2.1e18 (cube8-btcc).
With the two indices of einv swapped in k_defl_add all of b and c and the 40 cases of a with m >= 2 and more than one populated mode
fail (the 12 cases with m = 1 and the 8 with every node in one mode cannot see it, tests/test_pc_tail_host.py); with
knp_set_deflation clearing the modes before it scans the mode ids, d fails at "mode id = n_modes".
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import pytest
import torch

import irregular_meshes as IM
import pc_tail_ref as T
from parity_utils import ci_config, make_problem

pytestmark = pytest.mark.gpu

E_ARG, DIVERGED_ITS = -1, -3
KINDS = {"none": 0, "vbjacobi": 1}
WORST = {}


def _i32(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _f64(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _set_deflation(be, md, E):
    """straight through the ABI; returns the status"""
    if md is None:
        return be.lib.knp_set_deflation(be.ctx, 0, None, None)
    md, E = np.ascontiguousarray(md, dtype=np.int32), np.ascontiguousarray(E, dtype=np.float64)
    return be.lib.knp_set_deflation(be.ctx, E.shape[0], _i32(md), _f64(E))


def _apply(be, rt):
    z = torch.full_like(rt, float("nan"))        # an entry the library does not write shows
    be.pc_apply(rt, z)
    return z.cpu().numpy()


def _gain(zp, r):
    """The size of B on this r, largest potential entry over largest potential entry.  In these units B multiplies a potential
    residual by up to 4e13, and a correction from an Einv of order one would vanish in the rounding of z_plain: behind a
    preconditioner the generator's Einv (dense, not symmetric, uniform in [-1, 1]) is multiplied by this number, so that the
    correction and B r are of one size and ``bound`` is sensitive to both."""
    return float(np.abs(zp[3::4]).max() / np.abs(r[3::4]).max())


def _note(part, what, ratio):
    WORST[part] = max(WORST.get(part, 0.0), ratio)
    print(f"{part} {what}: max |z - ref| / bound = {ratio:.3e} (largest of part {part} so far {WORST[part]:.3e})")


def _check(part, what, z, zp, r, md, E, ns_on, bc_dofs=None, pattern=None):
    """the assertions shared by a, b and c; returns the reference"""
    ref, bound = T.tail_ref(zp, r, md, E, ns_on, bc_dofs=bc_dofs)
    for f in range(3):
        assert np.array_equal(z[f::4], zp[f::4]), (what, "ion entries", f)
    if not ns_on:
        off = np.asarray(md) < 0
        assert np.array_equal(z[3::4][off], zp[3::4][off]), (what, "potential entries outside every mode")
    ratio = float((np.abs(z[3::4] - ref[3::4]) / bound).max())
    _note(part, what, ratio)
    assert ratio <= T.GPU_TOL, (what, ratio)
    if pattern is not None and E.shape[0] >= 2 and T.indistinguishable("einv_transposed", pattern, E.shape[0], ns_on) is None:
        # these very inputs (z_plain as the library gave it) tell a transposed Einv from the right one
        seen = float((np.abs(T.tail_wrong("einv_transposed", zp, r, md, E, ns_on)[3::4] - ref[3::4]) / bound).max())
        assert seen >= 1e3 * T.GPU_TOL, (what, seen)
    return ref, bound


@pytest.fixture(scope="module")
def contexts(tmp_path_factory):
    """One context per (mesh, preconditioner, storage, Dirichlet rows), shared by the tests of this module.  Every test leaves
    deflation and the null space switched off."""
    from test_gpu_irregular import COARSE, _context, _pc_solver, _set_time
    cache = {}
    tmp = tmp_path_factory.mktemp("pc_tail")

    def amg_dirichlet(name, pc):
        """_pc_solver of test_gpu_irregular with the Dirichlet configuration of its _context"""
        import knpemi_oracle as K
        from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
        cfg = IM.config(tmp, name, pc=pc)
        cfg["dirichlet_bcs"] = True
        cfg["initial_conditions"].update({"Na_i": 10, "Na_e": 145, "K_i": 130, "K_e": 3, "Cl_i": 5, "Cl_e": 134})
        ks = cfg["solver"]["ksp_settings"]
        ks["amg_coarse_size"], ks["amg_fp32"], ks["amg_setup"] = COARSE[name], False, "host"
        p = make_problem(cfg)
        s = SolverKNPEMI(p, solver_config=p.solver_config)
        s.setup_solver()
        be = s.backend
        o = IM.oracle(name, params=K.Params(ki_init=K.OracleKNPEMI.REF_DEFAULT_KI, ke_init=K.OracleKNPEMI.REF_DEFAULT_KE))
        IM.perturb(o, p)
        p.setup_preconditioner(s.use_block_Jacobi)
        s.assemble_preconditioner()
        _set_time(p, o)
        be.assemble_rhs()
        be.assemble_matrix()
        be.pc_setup(s._pc_kind)
        return s, be

    def get(name, kind, fp32=False, dirichlet=False):
        key = (name, kind, fp32, dirichlet)
        if key not in cache:
            if kind in KINDS:
                p, be, _ = _context(tmp, name, dirichlet=dirichlet)
                be.assemble_matrix()
                be.pc_setup(KINDS[kind])
                keep = p
            elif dirichlet:
                keep, be = amg_dirichlet(name, kind)
            else:
                keep, be, _ = _pc_solver(tmp, name, kind, fp32)
            assert be.n_nodes_owned == be.n_nodes and be.n_dof_owned == 4 * be.n_nodes_owned
            assert (be.bc_dofs is not None) == dirichlet
            cache[key] = (keep, be)
        return cache[key][1]
    yield get
    cache.clear()


class _restored:
    """deflation and null space off again, whatever happens in between"""

    def __init__(self, be):
        self.be = be

    def __enter__(self):
        return self.be

    def __exit__(self, *exc):
        self.be.check(_set_deflation(self.be, None, None))
        self.be.set_nullspace(False)


# ---- a. the bare tail --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", T.PATTERNS)
@pytest.mark.parametrize("m", T.M_VALUES)
@pytest.mark.parametrize("name", T.MESHES)
def test_bare_tail_against_the_long_double_reference(name, m, pattern, contexts):
    with _restored(contexts(name, "none")) as be:
        n = be.n_nodes_owned
        r = T.residual(n)
        rt = torch.as_tensor(r, device=be.device)
        md, E = T.node_mode(pattern, m, n), T.einv(m)
        for ns_on in (False, True):
            be.set_nullspace(ns_on)
            be.check(_set_deflation(be, md, E))
            z = _apply(be, rt)
            _check("a", f"{name} m={m} {pattern} ns={int(ns_on)}", z, r, r, md, E, ns_on, pattern=pattern)
            assert np.array_equal(_apply(be, rt), z), "two applications, two results"


# ---- b. behind every preconditioner kind ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,fp32", [("vbjacobi", False), ("hypre", False), ("btcc", False), ("btcc", True)])
@pytest.mark.parametrize("name", T.MESHES)
def test_tail_behind_every_preconditioner_kind(name, kind, fp32, contexts):
    with _restored(contexts(name, kind, fp32)) as be:
        n = be.n_nodes_owned
        r = T.residual(n)
        rt = torch.as_tensor(r, device=be.device)
        zp = _apply(be, rt)                                  # deflation off, null space off
        assert np.all(np.isfinite(zp)) and not np.array_equal(zp, r)
        md, E = T.node_mode("random", 9, n), _gain(zp, r) * T.einv(9)
        for ns_on in (False, True):
            be.set_nullspace(ns_on)
            be.check(_set_deflation(be, md, E))
            z = _apply(be, rt)
            _check("b", f"{name} {kind} fp32={int(fp32)} ns={int(ns_on)}", z, zp, r, md, E, ns_on, pattern="random")
        be.set_nullspace(False)
        be.check(_set_deflation(be, None, None))
        assert np.array_equal(_apply(be, rt), zp), "n_modes = 0 does not return to the plain preconditioner"


# ---- c. with Dirichlet rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["none", "vbjacobi", "hypre"])
def test_tail_with_dirichlet_rows(kind, contexts):
    """The configuration of test_gpu_parity.test_dirichlet_bcs_without_mms on delaunay2d_24: every extracellular unknown of the
    exterior boundary is pinned.  With -1 on the pinned potential rows the preconditioner stays the identity on all pinned rows;
    a pinned potential row inside a mode receives the correction (include/knpemi_hip.h, knp_set_deflation) and nothing else does."""
    name = "delaunay2d_24"
    with _restored(contexts(name, kind, dirichlet=True)) as be:
        n = be.n_nodes_owned
        bc = be.bc_dofs_host.astype(np.int64)
        pinned = bc[(bc & 3) == 3] >> 2
        assert 40 <= pinned.size < n // 4 and bc.size == 4 * pinned.size
        r = T.residual(n)
        rt = torch.as_tensor(r, device=be.device)
        zp = _apply(be, rt)
        assert np.array_equal(zp[bc], r[bc])                 # B is the identity on Dirichlet rows
        E = _gain(zp, r) * T.einv(9)
        free = T.node_mode("random", 9, n)
        assert (free[pinned] >= 0).sum() >= 10               # the generator did put pinned rows into modes
        inside = free.copy()
        free[pinned] = -1
        inside[pinned[1::2]] = -1                            # every second pinned row stays in its mode
        hit = pinned[inside[pinned] >= 0]
        assert hit.size >= 5
        for ns_on in (False, True):
            be.set_nullspace(ns_on)
            be.check(_set_deflation(be, free, E))
            z = _apply(be, rt)
            _check("c", f"{name} {kind} Dirichlet, pinned rows out, ns={int(ns_on)}", z, zp, r, free, E, ns_on, bc_dofs=bc, pattern="random")
            ions = bc[(bc & 3) != 3]
            assert np.array_equal(z[ions], r[ions])
            if not ns_on:
                assert np.array_equal(z[bc], r[bc])
            be.check(_set_deflation(be, inside, E))
            z = _apply(be, rt)
            ref, bound = _check("c", f"{name} {kind} Dirichlet, pinned rows inside, ns={int(ns_on)}", z, zp, r, inside, E, ns_on, bc_dofs=bc, pattern="random")
            assert np.array_equal(z[ions], r[ions])
            if not ns_on:
                out = np.setdiff1d(pinned, hit)
                assert np.array_equal(z[4 * out + 3], r[4 * out + 3])
                moved = np.abs(z[4 * hit + 3] - r[4 * hit + 3]) / bound[hit]
                assert moved.min() >= 1e3 * T.GPU_TOL, moved.min()     # the correction did arrive on every pinned row of a mode


# ---- d. the ABI --------------------------------------------------------------------------------------------------------------------
def test_set_deflation_rejects_without_changing_anything(contexts):
    with _restored(contexts("delaunay3d_7", "none")) as be:
        n = be.n_nodes_owned
        r = T.residual(n)
        rt = torch.as_tensor(r, device=be.device)
        md, E = T.node_mode("random", 9, n), T.einv(9)
        be.set_nullspace(True)
        be.check(_set_deflation(be, md, E))
        before = _apply(be, rt)
        _check("d", "accepted, m=9", before, r, r, md, E, True)
        lib, ctx = be.lib, be.ctx
        big = np.ascontiguousarray(np.random.default_rng(0).uniform(-1, 1, (33, 33)))
        top, low = md.copy(), md.copy()
        top[n // 2] = 9
        low[n - 1] = -2
        rejected = [
            ("n_modes = 33", lambda: lib.knp_set_deflation(ctx, 33, _i32(md), _f64(big)), b"n_modes"),
            ("n_modes = -1", lambda: lib.knp_set_deflation(ctx, -1, _i32(md), _f64(E)), b"n_modes"),
            ("null node_mode", lambda: lib.knp_set_deflation(ctx, 9, None, _f64(E)), b"null"),
            ("null einv", lambda: lib.knp_set_deflation(ctx, 9, _i32(md), None), b"null"),
            ("mode id = n_modes", lambda: lib.knp_set_deflation(ctx, 9, _i32(top), _f64(E)), b"mode id"),
            ("mode id = -2", lambda: lib.knp_set_deflation(ctx, 9, _i32(low), _f64(E)), b"mode id"),
        ]
        for what, call, word in rejected:
            assert call() == E_ARG, what
            msg = lib.knp_last_error(ctx)
            assert b"deflation" in msg and word in msg, (what, msg)
            assert np.array_equal(_apply(be, rt), before), f"{what}: a rejected call changed the preconditioner"
        # a second accepted call with fewer modes and another map replaces the first
        md2, E2 = T.node_mode("descending", 7, n), T.einv(7)
        be.check(_set_deflation(be, md2, E2))
        z2 = _apply(be, rt)
        _check("d", "replaced, m=7", z2, r, r, md2, E2, True)
        assert not np.array_equal(z2, before)
        # n_modes = 0 with null arrays is accepted and switches deflation off
        assert lib.knp_set_deflation(ctx, 0, None, None) == 0
        z0 = _apply(be, rt)
        ref0, _ = T.tail_ref(r, r, np.full(n, -1, dtype=np.int32), np.zeros((0, 0)), True)
        be.set_nullspace(False)
        assert np.array_equal(_apply(be, rt), r)
        assert np.abs(z0 - ref0).max() <= T.GPU_TOL * (np.abs(r[3::4]).max() + np.abs(r[3::4]).mean())


# ---- e. the in-order branches of the Krylov drivers ------------------------------------------------------------------------------------
KRYLOV = {"square32-hypre": (32, "square", "hypre"), "cube8-btcc": (8, "cube", "btcc")}
BUDGET, RESTART, RTOL = 12, 5, 1e-12      # two full cycles and two iterations of a third; 1e-12 is out of reach in 12 iterations


def _krylov_case(N, kind, pc):
    """Deflation for these solves: m = 3, the random pattern, and the non-symmetric Einv of the generator scaled so that the
    correction Z Einv Z^T r of a random r is 1e-2 of B r (largest potential entry of each over the largest of r): B stays a usable
    preconditioner.  (Einv itself at 1e-2 of that ratio would make the correction, whose sums run over some 230 nodes, larger than B.)
    Einv is also made to give a correction of zero mean (node counts times Einv = 0; it stays dense and non-symmetric): left GMRES
    folds the gauge projection into Gram-Schmidt and takes the norm of the new vector by Pythagoras, so a correction with a large
    constant part makes that norm cancel, and the explicit norm the library then takes is one more read-back (``norm_fallbacks``,
    measured with the unmodified Einv: 1 on square32-hypre, read-backs 17 against 16) -- a case these tests are not to aim at.
    One step of the reference's loop with the first solve intercepted (the pattern of test_gpu_fgmres._wrap): b, the initial
    guess, the null space and the preconditioner are those of the run.  Both drivers are then run from that initial guess
    (a) without deflation and with KNP_GMRES_AHEAD=0, (b) with deflation through the library and (c) through the NumPy drivers."""
    import knpemi_oracle as K
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    from fgmres_ref import fgmres
    p = make_problem(ci_config(N=N, steps=1, rtol=1e-9, kind=kind, pc=pc))
    p.solver_config["view_ksp"] = False
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    s.setup_solver()
    s.setup_solver = lambda: None
    be = s.backend
    real = {"gmres": be.gmres, "fgmres": be.fgmres}
    out = {}

    def experiment(rtol, atol=1e-50, max_it=5000, restart=30):
        dev, n = be.b.device, be.n_nodes_owned
        b, x0 = be.b.clone(), be.x.clone()
        bh, x0h = b.cpu().numpy(), x0.cpu().numpy()
        ns = np.zeros(bh.size)
        ns[3::4] = 1.0
        ns /= np.linalg.norm(ns)

        def A(v):
            t = torch.as_tensor(np.ascontiguousarray(v), device=dev)
            y = torch.empty_like(t)
            be.spmv(t, y)
            return y.cpu().numpy()

        def B(v):
            t = torch.as_tensor(np.ascontiguousarray(v), device=dev)
            z = torch.empty_like(t)
            be.pc_apply(t, z)
            return z.cpu().numpy()

        class Op:
            def __matmul__(self, v):
                return A(v)

        def run(driver):
            be.x.copy_(x0)
            be.profile_reset()
            its, rn, reason = real[driver](RTOL, 1e-50, BUDGET, RESTART)
            return {"its": its, "rn": rn, "reason": reason, "x": be.x.cpu().numpy().copy(), "stats": be.stats()}
        # the size of B on a random vector (null space off for the measurement), and Einv at 1e-2 of it
        r = T.residual(n)
        be.set_nullspace(False)
        zr = B(r)
        be.set_nullspace(True)
        gain = _gain(zr, r)
        md, E = T.node_mode("random", 3, n), T.einv(3)
        cnt = np.bincount(md[md >= 0], minlength=3).astype(np.float64)
        E = E - np.outer(np.ones(3), cnt @ E) / cnt.sum()        # cnt^T E = 0: the correction has zero mean for every r
        assert np.abs(cnt @ E).max() <= 1e-12 * cnt.sum() and np.abs(E - E.T).max() > 0.1
        corr = T.tail_ref(np.zeros_like(r), r, md, E, False)[0]
        E = E * (1e-2 * gain * np.abs(r[3::4]).max() / np.abs(corr[3::4]).max())
        old = os.environ.get("KNP_GMRES_AHEAD")
        try:
            os.environ["KNP_GMRES_AHEAD"] = "0"          # read at knp_pc_setup
            be.pc_setup(s._pc_kind)
            for d in real:
                out[d, "plain"] = run(d)
        finally:
            if old is None:
                os.environ.pop("KNP_GMRES_AHEAD", None)
            else:
                os.environ["KNP_GMRES_AHEAD"] = old
            be.pc_setup(s._pc_kind)
        try:
            be.check(_set_deflation(be, md, E))
            for d in real:
                out[d, "deflated"] = run(d)
            xr, itr, rr, reasonr = fgmres(A, bh, x0h, B, ns=ns, rtol=RTOL, max_it=BUDGET, restart=RESTART)
            out["fgmres", "ref"] = {"its": itr, "rn": rr, "reason": reasonr, "x": xr}
            xr, itr, rr = K.gmres_left(Op(), bh, x0h, B, ns=ns, rtol=RTOL, max_it=BUDGET, restart=RESTART)
            out["gmres", "ref"] = {"its": itr, "rn": rr, "reason": DIVERGED_ITS if itr >= BUDGET else 2, "x": xr}
            out["gain"] = gain
        finally:
            be.check(_set_deflation(be, None, None))
        be.x.copy_(x0)
        be.b.copy_(b)
        be.profile_reset()
        return real["fgmres" if s._flexible else "gmres"](rtol, atol, max_it, restart)
    be.gmres = be.fgmres = experiment
    s.solve()
    assert all(r > 0 for r in s.reasons), s.reasons
    return out


@pytest.fixture(scope="module")
def krylov():
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = _krylov_case(*KRYLOV[case])
        return cache[case]
    yield get
    cache.clear()


@pytest.mark.parametrize("driver", ["fgmres", "gmres"])
@pytest.mark.parametrize("case", list(KRYLOV))
def test_krylov_drivers_in_order_with_deflation(case, driver, krylov):
    """With ``defl_m > 0`` neither driver may use k_proj_norm's one-reduction norm, start a cycle ahead of the host, fold a reduction
    into the cycle's last leg or fuse the tail.  Same algorithm as the NumPy drivers on the library's A and B (deflation and gauge
    step included): same count, same end, x per field within the 1e-9 of test_gpu_fgmres.test_same_algorithm_as_numpy; and the
    host reads back exactly as often as in the in-order solve without deflation (KNP_GMRES_AHEAD=0)."""
    res = krylov(case)
    lib, ref, plain = res[driver, "deflated"], res[driver, "ref"], res[driver, "plain"]
    err = [float(np.abs(lib["x"][f::4] - ref["x"][f::4]).max() / np.abs(ref["x"][f::4]).max()) for f in range(4)]
    bn = lib["stats"]["bnorm"]
    print(f"e {case} {driver}: gain {res['gain']:.3e}, norm fallbacks {lib['stats']['norm_fallbacks']} (plain {plain['stats']['norm_fallbacks']}), its {lib['its']} (ref {ref['its']}, plain {plain['its']}), reason {lib['reason']}, "
          f"residual / reference norm {lib['rn'] / bn:.3e} (ref {ref['rn'] / bn:.3e}, plain {plain['rn'] / plain['stats']['bnorm']:.3e}), "
          f"x err per field {err}, readbacks {lib['stats']['readbacks']} (plain {plain['stats']['readbacks']}), "
          f"stats {lib['stats']}, plain stats {plain['stats']}")
    assert lib["its"] == ref["its"] == BUDGET
    assert lib["reason"] == ref["reason"] == DIVERGED_ITS
    assert max(err) <= 1e-9, err
    assert lib["stats"]["fused_dots"] == 0 and lib["stats"]["fused_tails"] == 0, lib["stats"]
    assert plain["its"] == BUDGET and plain["reason"] == DIVERGED_ITS
    assert lib["stats"]["readbacks"] == plain["stats"]["readbacks"], (lib["stats"], plain["stats"])
    assert not np.array_equal(lib["x"], plain["x"])          # deflation did change the preconditioner
