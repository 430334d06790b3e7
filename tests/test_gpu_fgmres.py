"""Flexible GMRES on the GPU (knp_fgmres_solve: ksp_type fgmres, or gmres with norm_type unpreconditioned).

  * same algorithm: the NumPy restatement (tests/fgmres_ref.py) driven by the library's own knp_spmv and knp_pc_apply as A and B takes
    the same iterations and reaches the same iterate, step by step;
  * true residual: after every step ||b - A x|| <= rtol ||b||, recomputed in fp64 through knp_spmv, and the oracle's independent
    single-step check of the solution;
  * the first reduction stage folded into the SpMV (KNP_SPMV_DOTS) changes only summation order;
  * gauge: the null-space component of x is what the left-preconditioned solve leaves;
  * two ranks on one GPU."""
from __future__ import annotations

import os
import socket
import sys

import numpy as np
import pytest
import torch

from fgmres_ref import fgmres
from parity_utils import ci_config, make_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLEX = {"ksp_type": "fgmres", "norm_type": "unpreconditioned"}
# the true residual recomputed in fp64 through knp_spmv against the solver's own estimate |g_{j+1}|: rounding of the recurrence, 5 %
MARGIN = 1.05
# 512^2, rtol 1e-9 on the true residual, against the oracle's sparse direct solve of the same step (measured on MI355X):
# ||phi_e|| 7.7e-6 relative (the left solve at the same rtol: 6.7e-5), fields 1.1e-8 of their max norm, ||phi_i|| and phi_m 8e-9
PHI_E_REL, FIELD_REL = 3e-5, 1e-7


def _cfg(N, kind, pc, rtol, steps, ksp=FLEX, **extra):
    c = ci_config(N=N, steps=steps, rtol=rtol, kind=kind, pc=pc)
    c["solver"]["ksp_settings"].update(ksp)
    c["solver"]["ksp_settings"].update(extra)
    return c


def _solver(cfg):
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    p = make_problem(cfg)
    p.solver_config["view_ksp"] = False
    return SolverKNPEMI(p, solver_config=p.solver_config)


def _wrap(s, check):
    """Run the reference's loop unchanged; around every flexible solve record (b, x0) and append ``check(...)`` to the returned list."""
    s.setup_solver()
    be = s.backend
    real = be.fgmres
    out = []

    def wrapped(rtol, atol=1e-50, max_it=5000, restart=30):
        b = be.b.clone()
        x0 = be.x.clone()
        its, rn, reason = real(rtol, atol, max_it, restart)
        out.append(check(be, b, x0, be.x.clone(), its, rn, rtol, max_it, restart, reason))
        return its, rn, reason
    be.fgmres = wrapped
    s.setup_solver = lambda: None
    return out


def _same_algorithm(be, b, x0, x, its, rn, rtol, max_it, restart, reason):
    """NumPy FGMRES with the library's A and B (knp_pc_apply also removes the null-space component of its output: A ns = 0, so the
    iterates do not change), from the same initial guess and with the same gauge step."""
    dev = b.device
    ns = np.zeros(b.numel())
    ns[3::4] = 1.0
    ns /= np.linalg.norm(ns)

    def A(v):
        t = torch.as_tensor(v, device=dev).contiguous()
        y = torch.empty_like(t)
        be.spmv(t, y)
        return y.cpu().numpy()

    def B(v):
        t = torch.as_tensor(v, device=dev).contiguous()
        z = torch.empty_like(t)
        be.pc_apply(t, z)
        return z.cpu().numpy()
    xr, itr, rr, reasonr = fgmres(A, b.cpu().numpy(), x0.cpu().numpy(), B, ns=ns, rtol=rtol, max_it=max_it, restart=restart)
    xg = x.cpu().numpy()
    err = [float(np.abs(xg[f::4] - xr[f::4]).max() / np.abs(xr[f::4]).max()) for f in range(4)]
    return {"its": its, "its_ref": itr, "err": err, "reason": reason, "reason_ref": reasonr, "rn": rn, "rn_ref": rr}


@pytest.mark.parametrize("N,kind,pc,rtol,extra,ksp", [
    (32, "square", "hypre", 1e-9, {}, FLEX),                                      # 10-11 iterations: cycles longer than 8 vectors
    (8, "cube", "btcc", 1e-9, {}, FLEX),
    (32, "square", "hypre", 1e-9, {"gmres_restart": 4}, FLEX),                    # restarts, cycles shorter than 8 vectors
    (32, "square", "hypre", 1e-10, {}, FLEX),
    (32, "square", "hypre", 1e-9, {}, {"ksp_type": "gmres", "norm_type": "unpreconditioned"}),
])
def test_same_algorithm_as_numpy(N, kind, pc, rtol, extra, ksp):
    s = _solver(_cfg(N, kind, pc, rtol, 3, ksp, **extra))
    rec = _wrap(s, _same_algorithm)
    s.solve()
    print(rec)
    assert s._flexible and len(rec) == 3
    for r in rec:
        assert r["reason"] == 2 and r["its"] == r["its_ref"], r
        assert max(r["err"]) <= 1e-9, r
    if "gmres_restart" in extra:
        assert min(r["its"] for r in rec) > extra["gmres_restart"], rec
    if not extra:
        assert max(r["its"] for r in rec) > 8, rec   # iterations past the folded first stage (k_multi_dot) in the same cycle


def _true_res(be, b, x0, x, its, rn, rtol, max_it, restart, reason):
    y = torch.empty_like(b)
    be.spmv(x, y)
    n = be.n_dof_owned
    bn = float(torch.linalg.norm(b[:n]))
    return {"its": its, "reason": reason, "true": float(torch.linalg.norm(b[:n] - y[:n])) / bn, "est": rn / bn}


@pytest.mark.parametrize("N,kind,pc", [(512, "square", "hypre"), (64, "cube", "btcc")])
def test_true_residual_at_benchmarked_sizes(N, kind, pc):
    import knpemi_oracle as K
    from parity_utils import make_oracle, run_with_snapshots
    rtol = 1e-9
    s = _solver(_cfg(N, kind, pc, rtol, 3))
    rec = _wrap(s, _true_res)
    snaps = run_with_snapshots(s, (2, 3))
    print("flexible", N, kind, pc, rec)
    assert len(rec) == 3
    for r in rec:
        assert r["reason"] == 2 and r["true"] <= MARGIN * rtol, r
    # the oracle's own A and b of step 3 applied to the GPU's x, and at 512^2 its sparse direct solve of that step (the 64^3
    # factorisation takes an hour on one core: residual only)
    chk = K.single_step_check(make_oracle(N, kind), snaps[2]["state"], snaps[3]["x"], lu=(kind == "square"))
    print("single-step check:", {k: v for k, v in chk.items() if k != "blocks"})
    # (independently assembled A and b: 9.3e-10 at 512^2, 7.6e-10 at 64^3)
    assert chk["rel_residual"] <= 2 * rtol and chk["gauge_drift"] <= 1e-10, chk
    if kind == "square":
        assert max(chk["lu_field_diff"]) <= FIELD_REL, chk
        assert chk["rel_err_phi_i_L2"] <= FIELD_REL and chk["rel_err_phi_m_max"] <= FIELD_REL, chk
        assert chk["rel_err_phi_e_L2"] <= PHI_E_REL, chk


def _fields(cfg, env):
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)   # read at knp_pc_setup
        s = _solver(cfg)
        s.solve()
        return list(s.iterations), s.backend.x.cpu().numpy(), s.backend.stats()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# rtol stays well above the floor of the true residual: b is consistent only to ~2e-13 of its norm on the square (the left null vector's
# component), and at rtol 1e-12 the solve creeps along that floor for hundreds of iterations, where summation order
# alone moves the iteration count.
@pytest.mark.parametrize("N,kind,pc,rtol", [(32, "square", "hypre", 1e-10), (8, "cube", "btcc", 1e-10), (32, "square", "hypre", 1e-9)])
def test_fold_equivalence(N, kind, pc, rtol):
    cfg = _cfg(N, kind, pc, rtol, 4)
    its1, x1, st1 = _fields(cfg, {"KNP_SPMV_DOTS": "1"})
    its0, x0, st0 = _fields(cfg, {"KNP_SPMV_DOTS": "0"})
    print(its1, st1, its0, st0)
    assert st0["spmv_dots"] == 0
    # every iteration of a cycle of up to 8 vectors and every residual (at least one per solve) ran folded
    assert st1["spmv_dots"] >= sum(min(i, 8) for i in its1) + len(its1), (its1, st1)
    assert its1 == its0
    assert kind != "square" or max(its1) > 8, its1   # cycles past the fold's 8 vectors: the same cycle then runs k_multi_dot
    for f in range(4):
        scale = np.max(np.abs(x0[f::4]))
        assert np.max(np.abs(x1[f::4] - x0[f::4])) <= 1e-10 * scale, (f, np.max(np.abs(x1[f::4] - x0[f::4])) / scale)


@pytest.mark.parametrize("N,kind,pc", [(32, "square", "hypre"), (8, "cube", "btcc")])
def test_gauge_matches_left_gmres(N, kind, pc):
    """Both solves leave the sum of the potential unknowns where the initial guess had it (the initial data: phi_i = -0.07 on every
    intra node, phi_e = 0); the flexible one by projecting each cycle's correction, the left one through its projected basis."""
    sums = []
    for ksp in (FLEX, {"ksp_type": "gmres", "norm_type": "preconditioned"}):
        s = _solver(_cfg(N, kind, pc, 1e-10, 3, ksp))
        s.solve()
        x = s.backend.x.cpu().numpy()
        sums.append((float(x[3::4].sum()), int((s.backend.node_i >= 0).sum())))
    (fs, n_intra), (ls, _) = sums
    assert abs(fs - ls) <= 1e-10 * 0.07 * n_intra, sums
    assert abs(fs - (-0.07 * n_intra)) <= 1e-10 * 0.07 * n_intra, sums


def _free_port():
    so = socket.socket()
    so.bind(("127.0.0.1", 0))
    p = so.getsockname()[1]
    so.close()
    return p


def _worker(rank, size, port, q, N, kind, pc, rtol):
    try:
        os.environ["KNP_COMM"] = "p2p"
        os.environ.setdefault("KNP_P2P_TIMEOUT", "10")
        for p in (os.path.join(ROOT, "knp-emi-cgx_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
            sys.path.insert(0, p)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch as th
        import torch.distributed as dist
        th.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=size)
        s = _solver(_cfg(N, kind, pc, rtol, 2))

        def check(be, b, x0, x, its, rn, rt, max_it, restart, reason):   # true residual over the owned rows of both ranks
            y = th.empty_like(b)
            be.spmv(x, y)
            n = be.n_dof_owned
            sq = th.tensor([float(th.sum((b[:n] - y[:n]) ** 2)), float(th.sum(b[:n] ** 2))], dtype=th.float64)
            dist.all_reduce(sq)
            return (its, reason, float(np.sqrt(sq[0] / sq[1])))
        rec = _wrap(s, check)
        s.solve()
        ni, ne = s.potential_norms()
        q.put((rank, "ok", ni, ne, rec, bool(getattr(s.backend, "p2p_on", False))))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:      # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("N,kind,pc", [(32, "square", "hypre"), (8, "cube", "btcc")])
def test_two_ranks_on_one_gpu(N, kind, pc):
    """Two ranks (gloo rendezvous, native peer-to-peer exchange): k_multi_dot over the owned rows, one all-reduce per iteration; the
    true residual over both ranks meets the bound and the potentials match the oracle."""
    import torch.multiprocessing as mp
    from parity_utils import run_oracle
    rtol = 1e-9
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, N, kind, pc, rtol)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
    print(res)
    for r in res:
        assert r[1] == "ok", f"rank {r[0]}:\n{r[1]}"
    o = run_oracle(N=N, steps=2, kind=kind)
    oi, oe = o.potential_norms()
    for r in res:
        assert r[5], "the native exchange did not run"
        assert len(r[4]) == 2
        for its, reason, true in r[4]:
            assert reason == 2 and true <= MARGIN * rtol, r[4]
        assert abs(r[2] - oi) <= 2e-6 * oi
