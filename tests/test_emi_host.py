"""Host-side checks of the EMI model: the pins of the independent restatement tests/emi_ref.py (which the GPU tests then use as
their reference), the configuration surface of ``ProblemEMI`` / ``SolverEMI``, the reference's import paths, and the bytecode of
the membrane models against their closed forms.  Nothing here needs a GPU."""
import os

import numpy as np
import pytest

import emi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(**kw):
    cfg = {"problem_type": "EMI", "dt": 5e-5, "time_steps": 2, "cell_tag_file": "square8.xdmf", "facet_tag_file": "square8.xdmf",
           "ics_tags": [1], "ecs_tags": [2], "membrane_tags": [4], "quiet": True}
    cfg.update(kw)
    return cfg


# ------------------------------------------------------------------------------------------ emi_ref pins
@pytest.fixture(scope="module")
def mms():
    return {N: emi_ref.mms_run(N, dt=0.01, steps=2) for N in (16, 32)}


def test_reference_matrix_is_symmetric_and_annihilates_the_constant(mms):
    for N, (_, ref) in mms.items():
        A = ref.A
        assert abs(A - A.T).max() == 0.0
        assert np.abs(A @ np.ones(ref.n)).max() <= 1e-15 * abs(A).max()


def test_reference_node_layout_and_quadrature():
    _, ref = emi_ref.mms_run(8, steps=1)
    both = (ref.node_i >= 0) & (ref.node_e >= 0)
    assert both.sum() == 16 and np.all(ref.node_e[both] == ref.node_i[both] + 1)      # a membrane vertex: intra node, then extra node
    assert ref.n == ref.coords.shape[0] + both.sum()
    for dim in (2, 3):
        pts, w = emi_ref.facet_quadrature(dim, 10)
        assert abs(w.sum() - 1.0) < 1e-14 and np.allclose(pts.sum(axis=1), 1.0)
        # exact for lambda_0^a lambda_1^b of degree 10: a! b! (d-1)! / (a + b + d - 1)! on the unit facet with weights summing to 1
        from math import factorial as f
        for a, b in ((10, 0), (6, 4), (3, 7)):
            exact = f(a) * f(b) * f(dim - 1) / f(a + b + dim - 1)
            assert abs((w * pts[:, 0] ** a * pts[:, 1] ** b).sum() - exact) <= 1e-13 * exact


def test_reference_mms_errors_and_second_order(mms):
    """the figures of the issue: lumped-mass nodal L2 errors at dt = 0.01 after 2 steps"""
    (ei16, ee16), (ei32, ee32) = mms[16][0], mms[32][0]
    print(f"MMS errors N=16: {ei16:.4e} {ee16:.4e}; N=32: {ei32:.4e} {ee32:.4e}; ratios {ei16 / ei32:.3f} {ee16 / ee32:.3f}")
    assert ei16 == pytest.approx(2.42e-2, rel=5e-3) and ee16 == pytest.approx(2.02e-2, rel=5e-3)
    assert ei32 == pytest.approx(6.21e-3, rel=5e-3) and ee32 == pytest.approx(5.12e-3, rel=5e-3)
    assert ei16 / ei32 >= 3.0 and ee16 / ee32 >= 3.0


def test_reference_gating_forms_agree_for_small_steps():
    rng = np.random.default_rng(3)
    phi = rng.uniform(-0.08, 0.02, 50)
    y = [rng.uniform(0.05, 0.95, 50) for _ in range(3)]
    # 25 forward-Euler sub-steps against the exact exponential: at most (r dt)^2 / 50 apart, r = alpha + beta < 2e4 / s on this range
    rl = emi_ref.hh_gating_step(phi, *y, dt=1e-8, rush_larsen=True)
    fe = emi_ref.hh_gating_step(phi, *y, dt=1e-8, rush_larsen=False)
    for a, b in zip(rl, fe):
        assert np.allclose(a, b, rtol=0, atol=(2e4 * 1e-8) ** 2 / 50 + 1e-15)


# ------------------------------------------------------------------------------------------ configuration surface
def test_problem_emi_parses_a_config_without_a_solver_section():
    from cgx_hip.emi_problem import ProblemEMI
    p = ProblemEMI(_config(C_M=0.02, sigma_i=0.7, sigma_e=1.3, T=1.0))
    assert "solver" not in _config() and p.solver_config == {}
    assert (p.C_M, p.sigma_i, p.sigma_e, p.time_steps) == (0.02, 0.7, 1.3, 2) and float(p.dt.value) == 5e-5
    assert p.gamma_tags == (4,) and p.intra_tags == (1,) and p.extra_tag == (2,) and not p.dirichlet_bcs
    assert p.local_mesh.gamma.shape == (16, 4) and p.rhs_scale == 1.0
    assert [f.name for f in p.wh] == ["phi_i", "phi_e"] and [f.name for f in p.u_p] == ["phi_i", "phi_e"]
    cfg = _config(T=1e-3)
    del cfg["time_steps"]
    assert ProblemEMI(cfg).time_steps == 20                 # T / dt
    # class defaults of EMIx_problem.py:311-332
    d = ProblemEMI(_config())
    assert (d.C_M, d.sigma_i, d.sigma_e, d.phi_M_init, d.phi_e_init, d.fem_order) == (0.1, 1, 1, -0.06774, 0, 1)
    ProblemEMI.literal_reference_rhs = True
    try:
        assert ProblemEMI(_config()).rhs_scale == 5e-5
    finally:
        ProblemEMI.literal_reference_rhs = False


def test_solver_section_stays_mandatory_for_knpemi_and_for_other_problem_types():
    from cgx_hip.emi_problem import ProblemEMI
    from cgx_hip.problem import ProblemKNPEMI
    with pytest.raises(RuntimeError, match="solver configuration"):
        ProblemKNPEMI(_config())
    with pytest.raises(RuntimeError, match="problem_type"):
        ProblemEMI(_config(problem_type="KNP-EMI"))


def test_problem_emi_reads_the_reference_config_file(tmp_path):
    """the reference's EMI/config.yaml (tests/golden/emi_config.yaml: settings only), which has no solver section"""
    from cgx_hip.emi_problem import ProblemEMI
    text = open(os.path.join(ROOT, "tests", "golden", "emi_config.yaml")).read() + "\nquiet: true\n"
    path = tmp_path / "config.yaml"
    path.write_text(text)
    p = ProblemEMI(str(path))
    assert p.time_steps == 10 and p.C_M == 0.02 and p.mesh_description == "generated square32" and p.local_mesh.gamma.shape[0] == 64
    assert p.boundary_tag == 3


def test_dirichlet_and_multi_rank():
    from types import SimpleNamespace as NS
    from cgx_hip.emi_problem import ProblemEMI
    p = ProblemEMI(_config(dirichlet_bcs=True))
    x = p.mesh.geometry.x[p.bc_vertices]
    assert len(p.bc_vertices) == 32 and np.all(np.isclose(x, 0.0).any(axis=1) | np.isclose(x, 1.0).any(axis=1))
    assert np.all(p.bc_values == 0.0)
    with pytest.raises(NotImplementedError):
        ProblemEMI(_config(), comm=NS(size=2, rank=0))


def test_models_tags_and_solver_options():
    from cgx_hip.emi_models import HH_model, Passive_model, g_syn, g_syn_none
    from cgx_hip.emi_problem import ProblemEMI
    from cgx_hip.emi_solver import SolverEMI
    p = ProblemEMI(_config())
    hh = HH_model(p)
    p.add_ionic_model([hh], p.gamma_tags, stim_fun=g_syn)           # the call of the reference's EMI/main.py
    p.init_ionic_model([hh])
    assert len(p.ionic_models) == 1 and isinstance(p.ionic_models[0], HH_model) and p.ionic_models[0].g_Na_stim is g_syn
    assert float(p.n.x.array[0]) == HH_model.n_init_val and g_syn_none(0.3) == 0.0 and g_syn(0.003) == pytest.approx(40 * np.exp(-1.5))
    q = ProblemEMI(_config())
    q.add_ionic_model("Passive", tags=(7,))
    with pytest.raises(RuntimeError, match="membrane tags"):
        q.init_ionic_model()
    with pytest.raises(RuntimeError, match="not supported"):
        q.add_ionic_model("FitzHugh")
    assert str(Passive_model(q)) == "Passive"
    # class defaults of EMIx_solver.py:543-561 with the two stated deviations
    assert (SolverEMI.ksp_rtol, SolverEMI.ksp_max_it, SolverEMI.pc_type, SolverEMI.norm_type, SolverEMI.save_interval) == (1e-6, 1000, "hypre", "preconditioned", 1)
    assert SolverEMI.ksp_type == "cg" and SolverEMI.direct_rtol == 1e-12

    class G(SolverEMI):
        ksp_type = "gmres"
    with pytest.raises(NotImplementedError):
        G(p)

    class F(SolverEMI):
        pc_type = "fieldsplit"
    with pytest.raises(NotImplementedError):
        F(p)


def test_reference_import_paths():
    from CGx.EMI.EMIx_ionic_model import HH_model, Passive_model, g_syn, g_syn_none  # noqa: F401
    from CGx.EMI.EMIx_problem import ProblemEMI
    from CGx.EMI.EMIx_solver import SolverEMI
    from CGx.EMI.main import main, main_yaml  # noqa: F401
    from CGx.utils.mixed_dim_problem import MixedDimensionalProblem
    assert issubclass(ProblemEMI, MixedDimensionalProblem)
    for name in ("solve", "assemble_system", "assemble_rhs", "setup_solver", "create_and_set_nullspace", "print_info"):
        assert callable(getattr(SolverEMI, name))
    for name in ("add_ionic_model", "init_ionic_model", "setup_bilinear_form", "setup_linear_form", "setup_preconditioner", "print_errors"):
        assert callable(getattr(ProblemEMI, name))


# ------------------------------------------------------------------------------------------ membrane programs
def test_membrane_bytecode_against_the_closed_forms():
    import membrane_program_ref as mpr
    from cgx_hip._lib import OPS
    from cgx_hip.emi_models import g_syn
    from cgx_hip.emi_problem import ProblemEMI
    p = ProblemEMI(_config())
    p.add_ionic_model("HH", stim_fun=g_syn)
    p.add_ionic_model("Passive")
    p.init_ionic_model()
    rng = np.random.default_rng(5)
    ph = rng.uniform(-0.1, 0.1, (40, 6))
    n, m, h = (rng.uniform(0.0, 1.0, (40, 6)) for _ in range(3))
    inp = {"ki": [None] * 3, "ke": [None] * 3, "phim": ph, "aux": [n, m, h], "xq": [None] * 3}
    inv = {v: k for k, v in OPS.items()}
    for t in (0.0, 0.003, 0.0125):
        for model in p.ionic_models:
            model.refresh(t)
        hh, passive = p.compile_programs()
        for spec in (hh, passive):
            assert mpr.check_program(spec.code, len(spec.constants()), 2) is None
            used = {inv[op] for op, *_ in spec.code.tolist()}
            assert used <= {"CONST", "PHIM", "AUX", "ADD", "SUB", "MUL", "POWI", "OUT"}, used
            assert [r[2] for r in spec.code.tolist() if inv[r[0]] == "OUT"] == [0]
            assert {r[2] for r in spec.code.tolist() if inv[r[0]] == "AUX"} <= {0, 1, 2}
        got = np.asarray(mpr.run(("hh", hh.code, hh.constants()), inp)[0], dtype=np.float64)
        want = emi_ref.hh_current(ph, n, m, h, t)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
        got = np.asarray(mpr.run(("passive", passive.code, passive.constants()), inp)[0], dtype=np.float64)
        assert np.array_equal(got, ph)
    # the stimulus is ONE constant of the program: refreshing it changes nothing else
    p.ionic_models[0].refresh(0.0)
    c0 = hh.constants()
    p.ionic_models[0].refresh(0.004)
    c1 = hh.constants()
    assert (c0 != c1).sum() == 1 and c1[c0 != c1][0] == pytest.approx(float(g_syn(0.004)))
