"""Host-side checks of the state variables that membrane mechanisms declare with ``IonicModel.add_state``: the three keyword forms
against hand-written formulas, Hodgkin-Huxley's gates declared that way against the closed forms of ``k_hh_update``, the order of
evaluation within a sub-step, and the error paths.  The stepping is that of tests/state_program_ref.py (long double), which the GPU
tests then use as their reference.  Nothing here needs a GPU."""
import numpy as np
import pytest

import state_models as M
import state_program_ref as R
from parity_utils import ci_config, make_problem

from cgx_hip import fem
from cgx_hip._lib import KNP_MAX_AUX, KNP_MAX_PROG_REGS, OPS
from cgx_hip.ionic_models import HodgkinHuxley, IonicModel

LD = np.longdouble


def _problem(models, **kw):
    return make_problem(ci_config(N=8, steps=1, **kw), models)


def _fields(p, rng):
    """random nodal fields in the problem's ranges, as long doubles: (phi_m, ki, ke, x)"""
    n = p.mesh.num_vertices
    phim = M.away_from_singularities(rng, n, float(p.phi_rest.value)).astype(LD)
    ki = [rng.uniform(5.0, 150.0, n).astype(LD) for _ in range(3)]
    ke = [rng.uniform(3.0, 150.0, n).astype(LD) for _ in range(3)]
    x = [p.mesh.geometry.x[:, d].astype(LD) for d in range(p.mesh.geometry.x.shape[1])]
    return phim, ki, ke, x


@pytest.fixture(scope="module")
def mixed():
    p = _problem(lambda p: [M.Mixed(p)])
    return p, p.ionic_models[0]


def test_states_take_the_first_aux_slots_and_mark_the_problem(mixed):
    p, m = mixed
    assert [st.name for st in p.state_variables] == ["q", "g", "y", "u", "v"] == [st.function.name for st in p.state_variables]
    assert [st.kind for st in p.state_variables] == [0, 0, 1, 1, 1]
    assert [st.aux_index for st in p.state_variables] == [0, 1, 2, 3, 4]
    assert all(p.aux_functions[st.aux_index] is st.function for st in p.state_variables)
    assert p.gating_variables and (p.state_rush_larsen, p.state_substeps) == (True, 25)
    assert np.all(m.q.numpy() == 0.3) and np.array_equal(m.g.numpy(), np.linspace(0.1, 0.9, p.mesh.num_vertices))
    # the currents read the state under its slot
    aux_ops = {(a) for spec in p.programs.values() for op, d, a, b in spec.code.tolist() if op == OPS["AUX"]}
    assert aux_ops == {0}
    for st in p.state_variables:       # a gate writes OUT 0 and OUT 1, a general state OUT 0
        outs = [a for op, d, a, b in st.spec.code.tolist() if op == OPS["OUT"]]
        assert outs == ([0, 1] if st.kind == 0 else [0])


def test_keyword_forms_equal_hand_written_formulas(mixed):
    p, m = mixed
    rng = np.random.default_rng(11)
    phim, ki, ke, x = _fields(p, rng)
    n = phim.shape[0]
    val = {nm: rng.uniform(0.05, 0.95, n).astype(LD) for nm in ("q", "g", "y", "u", "v")}
    slots = [np.zeros(n, dtype=LD)] * KNP_MAX_AUX
    slots = list(slots)
    by = {st.name: st for st in p.state_variables}
    for nm, st in by.items():
        slots[st.aux_index] = val[nm]
    out = {nm: R.outputs(st, slots, phim, ki, ke, x) for nm, st in by.items()}
    close = lambda a, b: np.max(np.abs(a - b)) <= 1e-15 * np.max(np.abs(b))
    # inf / tau: alpha = inf / tau, beta = (1 - inf) / tau
    inf = 1 / (1 + np.exp(-(phim + LD(0.05)) / LD(0.01)))
    tau = LD(2e-3) + LD(1e-3) * np.exp(-(phim / LD(0.05)) ** 2)
    assert close(out["q"][0], inf / tau) and close(out["q"][1], (1 - inf) / tau)
    # alpha / beta reading K_e, another state, itself and a coordinate
    assert close(out["g"][0], 50 * ke[1] * (1 + val["q"]))
    assert close(out["g"][1], 120 * np.exp(phim / LD(0.04)) + 10 * val["g"] * x[0] * LD(1e6))
    # rhs
    assert close(out["y"][0], -LD(m.A) * val["g"] * (phim - LD(m.E)) - val["y"] / LD(m.TAU))
    assert close(out["u"][0], LD(m.W) * val["v"]) and close(out["v"][0], -LD(m.W) * val["u"])
    m.drive.value = 0.25                  # constants are read at every evaluation
    assert close(R.outputs(by["u"], slots, phim, ki, ke, x)[0], LD(m.W) * val["v"] * LD(0.25))
    m.drive.value = 1.0


@pytest.mark.parametrize("rush_larsen,substeps", [(True, 25), (False, 1), (False, 25)])
def test_hh_gates_from_add_state_reproduce_the_closed_forms(rush_larsen, substeps):
    """n, m, h declared through add_state, stepped by state_program_ref, against k_hh_update's formulas: 1e-14 in long double"""
    p = _problem(M.hh_from_states_models(rush_larsen, substeps))
    assert [st.name for st in p.state_variables] == ["n", "m", "h"] and p.aux_functions[:3] == [p.n, p.m, p.h]
    assert (p.state_rush_larsen, p.state_substeps) == (rush_larsen, substeps)
    rng = np.random.default_rng(5)
    rest = float(p.phi_rest.value)
    phim = M.away_from_singularities(rng, 400, rest).astype(LD)
    y = [rng.uniform(0.01, 0.99, 400).astype(LD) for _ in range(3)]
    dt = float(p.dt.value)
    got = R.state_step(p.state_variables, y, phim, dt, rush_larsen, substeps)
    want = M.hh_closed_form(phim, *y, dt, rest, rush_larsen, substeps)
    for g, w, nm in zip(got, want, "nmh"):
        err = float(np.max(np.abs(g - w)))
        print(f"{nm}: max |state program - closed form| = {err:.3e}")
        assert g.dtype == LD and err <= 1e-14


def test_built_in_hh_is_untouched_by_the_state_surface():
    p = _problem("ci")
    assert p.state_variables == [] and p.aux_functions == [p.m, p.h, p.n] and p.gating_variables
    assert isinstance(p.ionic_models[1], HodgkinHuxley) and not hasattr(p.ionic_models[1], "states")


def test_jacobi_order_of_two_states_that_read_each_other(mixed):
    """u' = W v, v' = -W u: both right-hand sides of a sub-step see the values of its beginning, so after one Euler sub-step
    (u, v) = (u0 + h W v0, v0 - h W u0); an update in place would give v0 - h W (u0 + h W v0)"""
    p, m = mixed
    n = p.mesh.num_vertices
    sts = [st for st in p.state_variables if st.name in ("u", "v")]
    u0, v0 = np.full(n, 1.0, dtype=LD), np.full(n, 0.5, dtype=LD)
    h = LD(1e-3)
    u1, v1 = R.state_step(sts, [u0, v0], np.zeros(n), float(h), True, 1)
    W = LD(m.W)
    assert np.max(np.abs(u1 - (u0 + h * W * v0))) <= 1e-18 and np.max(np.abs(v1 - (v0 - h * W * u0))) <= 1e-18
    assert np.min(np.abs(v1 - (v0 - h * W * (u0 + h * W * v0)))) > 1e-3
    # two sub-steps: the second starts from the first's results
    u2, v2 = R.state_step(sts, [u0, v0], np.zeros(n), float(2 * h), True, 2)
    assert np.max(np.abs(u2 - (u1 + h * W * v1))) <= 1e-17 and np.max(np.abs(v2 - (v1 - h * W * u1))) <= 1e-17


def test_rush_larsen_gates_keep_their_start_value_for_the_general_states(mixed):
    """y' = -A g (phi - E) - y / tau reads the gate g: with Rush-Larsen g advances at the end of the step, with forward Euler in every sub-step"""
    p, m = mixed
    rng = np.random.default_rng(2)
    phim, ki, ke, x = _fields(p, rng)
    sts = p.state_variables
    y0 = [st.function.numpy().astype(LD) for st in sts]
    dt = 1e-3
    rl = R.state_step(sts, y0, phim, dt, True, 4, ki, ke, None, x)
    fe = R.state_step(sts, y0, phim, dt, False, 4, ki, ke, None, x)
    g0, yy = y0[1], y0[2]
    for _ in range(4):
        yy = yy + LD(dt) / 4 * (-LD(m.A) * g0 * (phim - LD(m.E)) - yy / LD(m.TAU))
    assert np.max(np.abs(rl[2] - yy)) <= 1e-17 and np.max(np.abs(fe[2] - yy)) > 1e-8
    assert np.max(np.abs(rl[1] - g0)) > 1e-3            # ... and g itself did move


class _Bare(IonicModel):
    def __str__(self):
        return "bare"

    def _eval(self, ion_idx):
        return self.problem.phi_m_prev


def _with_init(init, **attrs):
    cls = type("Custom", (_Bare,), {"_init": init, **attrs})
    return lambda p: [cls(p)]


@pytest.mark.parametrize("kw", [dict(alpha=1.0, beta=2.0, rhs=3.0), dict(alpha=1.0), dict(inf=0.5), dict(), dict(inf=0.5, tau=1.0, alpha=1.0, beta=1.0)])
def test_exactly_one_keyword_form(kw):
    with pytest.raises(ValueError, match="state 'w'"):
        _problem(_with_init(lambda self: self.add_state("w", 0.0, **kw)))


def test_a_ninth_aux_field_is_refused():
    def eight_states(self):
        self.s = [self.add_state(f"s{k}", 0.0, rhs=1.0) for k in range(KNP_MAX_AUX)]
        self.extra = fem.Function(self.problem.V, "extra")
    reads_ninth = lambda self, ion_idx: self.problem.phi_m_prev * self.extra
    with pytest.raises(ValueError, match=f"more than {KNP_MAX_AUX} auxiliary"):
        _problem(_with_init(eight_states, _eval=reads_ninth))
    with pytest.raises(ValueError, match=f"more than {KNP_MAX_AUX} auxiliary"):
        _problem(_with_init(lambda self: [self.add_state(f"s{k}", 0.0, rhs=1.0) for k in range(KNP_MAX_AUX + 1)]))
    p = _problem(_with_init(eight_states))           # eight are fine
    assert len(p.state_variables) == len(p.aux_functions) == KNP_MAX_AUX


def test_the_register_limit_is_the_compilers():
    def deep(self):
        ph = self.problem.phi_m_prev
        e = ph
        for k in range(KNP_MAX_PROG_REGS + 4):      # every left operand stays live until the innermost term is done
            e = (ph * float(k + 2)) - e
        self.add_state("deep", 0.0, rhs=e)
    with pytest.raises(ValueError, match=f"more than {KNP_MAX_PROG_REGS} registers"):
        _problem(_with_init(deep))


def test_models_must_agree_on_the_ode_settings():
    a = type("A", (_Bare,), {"_init": lambda self: self.add_state("a", 0.0, rhs=1.0), "time_steps_ODE": 25})
    b = type("B", (_Bare,), {"_init": lambda self: self.add_state("b", 0.0, rhs=1.0), "time_steps_ODE": 10})
    with pytest.raises(ValueError, match="disagree on use_Rush_Larsen / time_steps_ODE"):
        _problem(lambda p: [a(p), b(p)])
    b.time_steps_ODE = 25
    b.use_Rush_Larsen = False
    with pytest.raises(ValueError, match="disagree"):
        _problem(lambda p: [a(p), b(p)])
    b.use_Rush_Larsen = True
    assert len(_problem(lambda p: [a(p), b(p)]).state_variables) == 2
    with pytest.raises(ValueError, match="declared twice"):
        _problem(lambda p: [a(p), a(p)])


def test_steady_state_initial_conditions_do_not_know_declared_states():
    from cgx_hip.problem import ProblemKNPEMI
    cfg = ci_config(N=8, steps=1)
    del cfg["initial_conditions"]
    p = ProblemKNPEMI(cfg)
    assert p.find_initial_conditions
    model = _with_init(lambda self: self.add_state("ca", 0.0, rhs=1.0))(p)
    with pytest.raises(NotImplementedError, match="'ca'"):
        p.init_ionic_models(model)


def test_zero_rates_keep_a_rush_larsen_gate_and_inf_tau_is_built_once():
    p = _problem(lambda q: [M.MaskedGate(q)])
    m = p.ionic_models[0]
    assert m.calls == 1                                   # the callable of inf= is called once, its expression shared by alpha and beta
    n = p.mesh.num_vertices
    x = [p.mesh.geometry.x[:, d] for d in range(2)]
    off = x[0] <= 0.5e-6
    assert 0 < off.sum() < n
    y0 = [np.full(n, 0.4, dtype=LD), np.full(n, 0.2, dtype=LD)]
    w1 = R.state_step(p.state_variables, y0, np.full(n, -0.06), 1e-3, True, 25, x=x)[0]
    assert np.all(np.isfinite(w1)) and np.all(w1[off] == y0[0][off])
    want = LD(0.8) + (LD(0.4) - LD(0.8)) * np.exp(-LD(1e-3) * 100)
    assert np.max(np.abs(w1[~off] - want)) <= 1e-17


def test_names_of_checkpoint_keys_are_refused():
    for name in ("t", "coords", "phi_m", "K_e", "phi_i"):
        with pytest.raises(ValueError, match=f"state '{name}'.*checkpoints"):
            _problem(_with_init(lambda self, name=name: self.add_state(name, 0.0, rhs=1.0)))
    from cgx_hip.ionic_models import ATPPump, NeuronalCotransporters
    clash = _with_init(lambda self: self.add_state("n", 0.0, rhs=1.0))
    with pytest.raises(ValueError, match="state 'n'.*built-in"):
        _problem(lambda q: [NeuronalCotransporters(q), HodgkinHuxley(q), ATPPump(q)] + clash(q))


def test_emi_models_have_the_same_surface():
    from cgx_hip.emi_problem import ProblemEMI
    cfg = {"problem_type": "EMI", "dt": 5e-5, "time_steps": 2, "cell_tag_file": "square8.xdmf", "facet_tag_file": "square8.xdmf",
           "ics_tags": [1], "ecs_tags": [2], "membrane_tags": [4], "quiet": True}
    p = ProblemEMI(cfg)
    p.init_ionic_model([M.HHStatesEMI(p)])
    assert [st.name for st in p.state_variables] == ["n", "m", "h"] and not hasattr(p, "n")
    assert (p.state_rush_larsen, p.state_substeps) == (True, 25)
    p.compile_programs()
    assert [st.aux_index for st in p.state_variables] == [0, 1, 2] and len(p.aux_functions) == 3
    rng = np.random.default_rng(9)
    phim = M.away_from_singularities(rng, 200, M.HHStatesEMI.H.V_rest).astype(LD)
    y = [rng.uniform(0.01, 0.99, 200).astype(LD) for _ in range(3)]
    got = R.state_step(p.state_variables, y, phim, 5e-5, True, 25)
    want = M.hh_closed_form(phim, *y, 5e-5, M.HHStatesEMI.H.V_rest, True, 25)
    assert max(float(np.max(np.abs(g - w))) for g, w in zip(got, want)) <= 1e-14
    import inspect
    from cgx_hip import emi_models, ionic_models
    assert inspect.signature(emi_models.IonicModel.add_state) == inspect.signature(ionic_models.IonicModel.add_state)
    with pytest.raises(ValueError, match="state 'w'"):
        M.HHStatesEMI(p).add_state("w", 0.0, alpha=1.0, rhs=1.0)
    with pytest.raises(ValueError, match="state 'phi_e'.*checkpoints"):
        M.HHStatesEMI(p).add_state("phi_e", 0.0, rhs=1.0)
    # n, m, h of HH_model and six states: nine aux fields
    q = ProblemEMI(cfg)
    q.add_ionic_model("HH")
    extra = M.HHStatesEMI(q)
    extra._init = lambda: [extra.add_state(f"s{k}", 0.0, rhs=1.0) for k in range(6)]
    q.ionic_models.append(extra)
    q.init_ionic_model()
    with pytest.raises(ValueError, match=f"more than {KNP_MAX_AUX} auxiliary"):
        q.compile_programs()
