"""Per-tag ion budgets and the stimulus-current trace on the device (csrc/knp_diagnostics.inc, cgx_hip/diagnostics.py):
``print_conservation`` / ``ion_budget`` against host P1 integrals of the device fields, per-cell charge conservation, the
stimulus trace of ``CGx.KNPEMI.main`` against a host quadrature of the stimulus expression, determinism and two ranks."""
import copy
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp
import yaml

from parity_utils import ci_config, make_problem, tissue_config, two_cell_config, two_cell_mesh

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.array([1.0, 1.0, -1.0])


def _host_budget(p):
    """P1 integrals of the device fields, copied to the host: per cell tag, [Na, K, Cl] (owned cells, cell volume times the
    mean of the vertex values on the cell's side)"""
    lm = p.local_mesh
    nco = lm.n_cells_owned
    cells = lm.cells[:nco]
    X = lm.coords[cells]
    d = X.shape[2]
    vol = np.abs(np.linalg.det(X[:, 1:, :] - X[:, :1, :])) / (2.0 if d == 2 else 6.0)
    tags = list(p.intra_tags) + list(np.ravel(p.extra_tag))
    out = np.zeros((len(tags), 3))
    for j in range(3):
        ki, ke = p.wh[0][j].numpy(), p.wh[1][j].numpy()
        k = np.where((p.cell_side[:nco] == 0)[:, None], ki[cells], ke[cells])
        per = vol * k.mean(axis=1)
        for t, tag in enumerate(tags):
            out[t, j] = per[lm.cell_tags[:nco] == tag].sum()
    return np.array(tags), out


def _solver(cfg, models="ci"):
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    p = make_problem(cfg, models)
    p.solver_config["view_ksp"] = False
    return SolverKNPEMI(p, solver_config=p.solver_config)


def _two_cell_cfg(tmp_path, steps=2):
    coords, cells, tags, fverts, ftags = two_cell_mesh(16)
    path = str(tmp_path / "twocells.npz")
    np.savez(path, coords=coords, cells=cells, cell_tags=tags, facets=fverts, facet_tags=ftags)
    return two_cell_config(path, steps=steps)


@pytest.mark.parametrize("case", ["square16", "cube8", "tissue2d", "tissue3d", "two_cell"])
def test_print_conservation_matches_host_integrals(case, tmp_path, capsys):
    models = "ci"
    if case == "square16":
        cfg = ci_config(N=16, steps=2, rtol=1e-11)
    elif case == "cube8":
        cfg = ci_config(N=8, steps=2, rtol=1e-11, kind="cube")
    elif case == "tissue2d":
        cfg = tissue_config(2, 18, 3, steps=2, rtol=1e-11)
    elif case == "tissue3d":
        cfg = tissue_config(3, 12, 2, steps=2, rtol=1e-11, pc="btcc")
    else:
        from cgx_hip.configs import default_ionic_models
        cfg, models = _two_cell_cfg(tmp_path), default_ionic_models
    s = _solver(cfg, models)
    s.solve()
    p = s.problem
    capsys.readouterr()
    p.print_conservation()
    out = capsys.readouterr().out.splitlines()
    b = p.ion_budget()
    tags, host = _host_budget(p)
    assert np.array_equal(b["tag"], tags)
    if case.startswith("tissue"):
        assert (b["side"] == 0).sum() >= 8
    for j, nm in enumerate(("Na", "K", "Cl")):
        assert np.allclose(b[nm], host[:, j], rtol=1e-12, atol=0), nm
        assert b[nm].sum() == pytest.approx(host[:, j].sum(), rel=1e-12)
    assert np.allclose(b["charge"], float(p.F.value) * (host @ Z), rtol=1e-12, atol=1e-12 * float(p.F.value) * np.abs(host).sum(axis=1).max())
    # the reference's lines (KNPEMIx_problem.py:825-843)
    intra = np.nonzero(b["side"] == 0)[0]
    want = [f"Time {p.t.value*1e3:.2f} ms", f"Total Na+ concentration: {b['Na'].sum():.2e} mol",
            f"Total K+  concentration: {b['K'].sum():.2e} mol", f"Total Cl- concentration: {b['Cl'].sum():.2e} mol"]
    want += [f"  Intra tag {b['tag'][k]}: Volume = {b['volume'][k]:.2e} m^3, Area = {b['area'][k]:.2e} m^2, Charge = {b['charge'][k]:.2e} C"
             for k in intra]
    assert out == want
    tot = s.backend.total_ion_amounts()
    assert np.allclose(tot, host.sum(axis=0), rtol=1e-12, atol=0)
    if case in ("tissue2d", "tissue3d", "two_cell"):
        assert np.all(b["area"][intra] > 0)


def test_per_cell_charge_is_conserved():
    """Test function 1 on one cell's intracellular nodes: the stiffness and drift terms vanish, the cell's phi_i rows give
    C_M int_G dphi_m = -dt int_G I_ch and the ion rows, weighted by z_k F and summed (sum_k alpha_k = 1), give
    F sum_k z_k dN_k = -(C_M int_G dphi_m + dt int_G I_ch) = 0 (KNPEMIx_problem.py:594-610, 637-642).  No volume sources.

    Bound from the solver tolerance: flexible GMRES stops on the true residual, ||b - A x||_2 <= rtol ||b||_2 per step.  The
    rows of a cell (3 ion rows and the phi_i row per intracellular node, in mol) enter the step's charge change with weights
    F z_k and F, so |dQ_step| <= F ||r_cell||_1 <= F sqrt(4 n_cell) ||r||_2 <= F sqrt(4 n_cell) rtol ||b_step||_2.  Summed over
    the steps, plus the rounding of the budget sums (1e-13 of F sum_k |z_k| N_k, ~100 ulp)."""
    steps, rtol = 20, 1e-11
    cfg = tissue_config(2, 25, 6, steps=steps, rtol=rtol, pc="hypre", stimulus=True, width=1)
    cfg["solver"]["ksp_settings"]["ksp_type"] = "fgmres"
    cfg["solver"]["ksp_settings"]["norm_type"] = "unpreconditioned"
    s = _solver(cfg)
    p = s.problem
    s.prepare()
    be = s.backend
    b0 = p.ion_budget()
    bnorm = []
    solve = be.fgmres

    def fgmres(*a, **k):
        import torch
        bnorm.append(float(torch.linalg.norm(be.b[:be.n_dof_owned])))
        return solve(*a, **k)
    be.fgmres = fgmres
    for i in range(1, steps + 1):
        s.step(i)
    s.finish()
    assert len(bnorm) == steps and all(r > 0 for r in s.reasons)
    b1 = p.ion_budget()
    F = float(p.F.value)
    amounts = lambda b: np.stack([b["Na"], b["K"], b["Cl"]], axis=1)
    A0, A1 = amounts(b0), amounts(b1)
    lm = p.local_mesh
    intra = np.nonzero(b0["side"] == 0)[0]
    assert len(intra) == 36
    moved = 0
    for t in intra:
        tag = b0["tag"][t]
        verts = np.unique(lm.cells[lm.cell_tags == tag])
        n_cell = len(verts)
        dQ = F * Z @ (A1[t] - A0[t])
        scale = F * np.abs(Z) @ A0[t]
        bound = F * np.sqrt(4.0 * n_cell) * rtol * sum(bnorm) + 1e-13 * scale
        assert abs(dQ) <= bound, (tag, dQ, bound, scale)
        assert abs(b1["charge"][t] - b0["charge"][t]) <= bound
        moved += np.abs(A1[t] - A0[t]).max() > 1e-9 * np.abs(A0[t]).max()
    assert moved > 0, "no cell's ion amounts changed: the check would be vacuous"


def _host_stimulus(p):
    """int stim_ufl_expr dS(stimulus_tags) on the host: this rank's facets (owner of the first vertex), the problem's
    quadrature, the fields interpolated at the points, the expression's constants as they are now"""
    from cgx_hip import fem
    lm = p.local_mesh
    sel = np.isin(p.gamma_facet_tags, p.stimulus_tags) & (p._fv[:, 0] < lm.n_vertices_owned)
    fv, fm = p._fv[sel], p._fmeas[sel]
    lam = p.q_pts                                             # (q, d) barycentric
    xq = np.einsum("qa,nak->nqk", lam, lm.coords[fv])
    fields = {}
    for f in [*p.wh[0], *p.wh[1], p.phi_m_prev] + list(p.aux_functions):
        fields[id(f)] = np.einsum("qa,na->nq", lam, f.numpy()[fv])
    env = {"x": [xq[:, :, k] for k in range(xq.shape[2])], "fields": fields}
    vals = np.broadcast_to(fem.evaluate_numpy(p.stim_ufl_expr, env), xq.shape[:2])
    return float((fm[:, None] * vals * p.q_w[None, :]).sum())


@pytest.fixture(scope="module")
def long_tags():
    """tissue_config(3, 30, 5) with random fields and no time step: tags of more chunks than the 64 lanes of the combine's wave"""
    import torch
    p = make_problem(tissue_config(3, 30, 5, steps=1), "ci")
    be = p.create_backend()
    rng = np.random.default_rng(29)
    n = p.local_mesh.coords.shape[0]
    write = lambda fn, v: fn.x.array.copy_(torch.from_numpy(v).to(fn.x.array.device))
    for s in range(2):
        for j in range(p.N_ions):
            write(p.wh[s][j], rng.uniform(1.0, 150.0, n))
        write(p.wh[s][p.N_ions], rng.uniform(-0.1, 0.1, n))
    write(p.phi_m_prev, p.wh[0][p.N_ions].numpy() - p.wh[1][p.N_ions].numpy())
    return p, be


def test_ion_amounts_of_a_tag_longer_than_a_wave_match_host_integrals(long_tags):
    p, be = long_tags
    lay = be.budget_layout()
    tags, host = _host_budget(p)
    assert np.array_equal(lay.tags, tags)
    e = len(tags) - 1                                         # the extracellular tag
    assert lay.side[e] == 1
    chunks = (lay.seg_ptr[e + 1] - 1) // 256 - lay.seg_ptr[e] // 256 + 1
    print("extracellular tag:", lay.seg_ptr[e + 1] - lay.seg_ptr[e], "cells in", chunks, "chunks")
    assert chunks > 64
    got = be.ion_amounts().cpu().numpy()
    print("max rel. difference", np.abs(got / host - 1.0).max())
    assert np.allclose(got, host, rtol=1e-12, atol=0)
    assert be.ion_amounts().cpu().numpy().tobytes() == got.tobytes()


def test_membrane_integral_of_a_group_longer_than_a_wave_matches_host_quadrature(long_tags):
    import torch
    from cgx_hip.diagnostics import facet_group_map, membrane_program
    p, be = long_tags
    seg_ptr, facets = facet_group_map(p, [p.stimulus_tags])
    assert len(facets) == 24000 and (seg_ptr[1] - 1) // 128 + 1 == 188      # one group, 188 chunks of 128
    be.set_diag_program(membrane_program(p, p.stim_ufl_expr))
    be.set_facet_groups([p.stimulus_tags])
    got = be.membrane_integral(torch.zeros(1, dtype=torch.float64, device=be.device)).cpu().numpy()
    host = np.array([_host_stimulus(p)])
    print("device", got[0], "host", host[0], "rel. difference", abs(got[0] / host[0] - 1.0))
    assert np.abs(host).max() > 0
    assert np.allclose(got, host, rtol=1e-12, atol=1e-12 * np.abs(host).max())


def _write_cfg(tmp_path, name, cfg, out_dir):
    cfg = copy.deepcopy(cfg)
    cfg["output_dir"] = str(out_dir) + "/"
    cfg["solver"]["output"].update({"save_pngs": True, "save_dat": True})
    path = tmp_path / name
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return str(path)


def _run_main_with_host_stimulus(path):
    """CGx.KNPEMI.main --config, recording at every record the host quadrature of the stimulus with that step's fields"""
    from cgx_hip import output as outmod
    from CGx.KNPEMI import main as mainmod
    host = []
    orig = outmod.RunOutput.record

    def record(self, i):
        orig(self, i)
        host.append(_host_stimulus(self.p))
    outmod.RunOutput.record = record
    try:
        s = mainmod.main(["--config", path])
    finally:
        outmod.RunOutput.record = orig
    return s, np.array(host)


@pytest.mark.parametrize("case", ["square", "tissue"])
def test_stimulus_trace_matches_host_quadrature(case, tmp_path):
    if case == "square":
        cfg = ci_config(N=16, steps=6, rtol=1e-11)
        assert cfg["stimulus"]["scale"] is True
        name = "square_config_stim.yml"
    else:
        cfg = tissue_config(2, 18, 3, steps=6, rtol=1e-11)
        assert "stimulus_region" in cfg
        name = "tissue_stim.yml"
    out = tmp_path / "out"
    s, host = _run_main_with_host_stimulus(_write_cfg(tmp_path, name, cfg, out))
    stim = np.load(out / "stimulus.npy")
    assert stim.shape == (cfg["time_steps"] + 1,)
    assert len(host) == len(stim)
    assert np.allclose(stim, host, rtol=1e-12, atol=1e-12 * np.abs(host).max())
    assert np.abs(stim).max() > 0
    # the budget trace is opt-in: no file without the key
    assert not (out / "ion_budget.npy").exists() and not (out / "ion_budget_tags.npy").exists()


def _budget_run(tmp_path, tag):
    cfg = tissue_config(2, 18, 3, steps=4, rtol=1e-11)
    cfg["solver"]["output"]["save_ion_budget"] = True
    cfg["solver"]["output"]["save_interval"] = 1
    out = tmp_path / tag
    from CGx.KNPEMI import main as mainmod
    s = mainmod.main(["--config", _write_cfg(tmp_path, f"tissue_{tag}.yml", cfg, out)])
    return s, np.load(out / "ion_budget.npy"), np.load(out / "ion_budget_tags.npy"), np.load(out / "stimulus.npy")


def test_budget_and_stimulus_traces_are_deterministic(tmp_path):
    s1, b1, t1, st1 = _budget_run(tmp_path, "a")
    s2, b2, t2, st2 = _budget_run(tmp_path, "b")
    assert b1.shape == (5, 10, 3) and t1.shape == (10, 4)
    assert b1.tobytes() == b2.tobytes() and st1.tobytes() == st2.tobytes() and t1.tobytes() == t2.tobytes()
    # last record = the final state
    _, host = _host_budget(s1.problem)
    assert np.allclose(b1[-1], host, rtol=1e-12, atol=0)
    bud = s1.problem.ion_budget()
    assert np.array_equal(t1[:, 0], bud["tag"]) and np.allclose(t1[:, 2], bud["volume"], rtol=1e-14)


def _free_port():
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def _worker(rank, size, port, out_dir, q):
    try:
        for path in (os.path.join(ROOT, "knp-emi-cgx_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
            sys.path.insert(0, path)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        if size > 1:
            dist.init_process_group("gloo", rank=rank, world_size=size)
        from parity_utils import run_native, tissue_config
        from cgx_hip import output as outmod
        host = []
        orig = outmod.RunOutput.record

        def record(self, i):                # host quadrature of this rank layout's own fields, summed over the ranks
            orig(self, i)
            host.append(self.p.comm.allreduce_sum(_host_stimulus(self.p)))
        outmod.RunOutput.record = record
        cfg = tissue_config(2, 18, 3, steps=3, rtol=1e-13)
        cfg["output_dir"] = out_dir + "/"
        cfg["solver"]["output"].update({"save_dat": True, "save_ion_budget": True, "save_interval": 1})
        s = run_native(cfg)
        b = s.problem.ion_budget()
        tot = s.backend.total_ion_amounts()
        q.put((rank, "ok", {k: np.asarray(v) for k, v in b.items()}, tot, np.array(host)))
        if size > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:      # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc(), None, None, None))


def _spawn(size, out_dir):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, size, port, out_dir, q)) for r in range(size)]
    for pr in procs:
        pr.start()
    res = sorted([q.get(timeout=300) for _ in range(size)], key=lambda r: r[0])
    for pr in procs:
        pr.join(timeout=60)
    for r in res:
        assert r[1] == "ok", f"rank {r[0]}:\n{r[1]}"
    return res


def test_two_ranks_give_the_one_rank_budgets(tmp_path):
    one = _spawn(1, str(tmp_path / "one"))[0]
    two = _spawn(2, str(tmp_path / "two"))
    for r in two:                      # every rank returns the sums over ranks
        for k in ("tag", "side"):
            assert np.array_equal(r[2][k], one[2][k])
        for k in ("volume", "area", "Na", "K", "Cl", "charge"):
            assert np.allclose(r[2][k], one[2][k], rtol=1e-12, atol=0), k
        assert np.allclose(r[3], one[3], rtol=1e-12, atol=0)
    a, b = np.load(tmp_path / "one" / "ion_budget.npy"), np.load(tmp_path / "two" / "ion_budget.npy")
    assert a.shape == b.shape == (4, 10, 3)
    assert np.allclose(b, a, rtol=1e-12, atol=0)
    # the stimulus trace: on each layout it is the host quadrature of that layout's fields; the two layouts agree to 1e-12 where
    # the fields are the same (record 0).  Later records follow the two solves' trajectories, which drift apart (measured: 3e-11,
    # 8e-10, 2e-9 after steps 1-3); held to the 1e-6 the multi-rank solve tests ask of phi_m
    a, b = np.load(tmp_path / "one" / "stimulus.npy"), np.load(tmp_path / "two" / "stimulus.npy")
    assert a.shape == b.shape == (4,) and np.abs(a).min() > 0
    for trace, res in ((a, one[4]), (b, two[0][4])):
        assert np.allclose(trace, res, rtol=1e-12, atol=0)
    assert abs(b[0] - a[0]) <= 1e-12 * abs(a[0])
    rel = np.abs(b - a) / np.abs(a)
    assert rel.max() <= 1e-6, rel
    assert np.allclose(np.load(tmp_path / "two" / "ion_budget_tags.npy"), np.load(tmp_path / "one" / "ion_budget_tags.npy"), rtol=1e-12)
