"""csrc/knp_step_state.hpp on the host alone (no GPU): tools/step_state_check.cpp drives the step-boundary protocol through scripted
sequences and a walk of 20 000 random events and prints every event with what it returned and the state after it.  The rules are restated
here (Model), every printed line is replayed through them, and the scripted sequences are judged against what the protocol promises.

Where the entry points' behaviour at the parent of this change differed from its comments, the code's behaviour is what is restated:
a matrix assembly that runs the copy pass leaves `armed` as it was; a speculation dropped at the top of an assembly whose fields still
qualify for the skip of the copy pass (other phi_m, other dt, form no longer eligible -- but promise and concentration pointers in place)
re-arms the context in the same call, so only the drop for a missing promise ends disarmed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ("fields_current", "knod_current", "promise", "knod_skipped", "armed", "pending", "tail_x", "n_tail", "n_skip", "n_adopted", "n_discarded")


class Model:
    """The table of knp_step_state.hpp."""

    def __init__(self):
        self.fields_current = self.knod_current = self.promise = self.knod_skipped = self.armed = self.pending = 0
        self.tail_x = -1
        self.n_tail = self.n_skip = self.n_adopted = self.n_discarded = 0
        self.ahead = None

    def state(self):
        return tuple(int(getattr(self, k)) for k in FLAGS)

    def drop(self):
        if not self.pending:
            return 0
        self.pending = self.armed = 0
        self.n_discarded += 1
        return 1

    def X(self):
        self.fields_current = self.knod_current = 0
        return [self.drop()]

    def T(self):
        self.promise = 0
        return self.X()

    def I(self):
        return [self.drop()]

    def P(self):
        self.promise = 1
        return []

    def D(self, x, w):
        self.tail_x, self.fields_current, self.knod_current = x, 1, w
        self.n_tail += 1
        return []

    def M(self):
        return [int(self.armed and self.knod_current and not self.pending)]

    def S(self, *a):
        self.pending, self.ahead = 1, (a[:7], a[7])
        return []

    def A(self, matrix, *a):
        f, (nodal_copy, have_target, class_timing, form_ok, dt), target = a[:7], a[7:12], a[12:18]
        dropped = 0
        if matrix and self.pending:
            if self.promise and self.knod_current and form_ok and self.ahead == (f, dt):
                self.pending = self.promise = self.knod_current = 0
                self.knod_skipped = self.armed = 1
                self.n_skip += 1
                self.n_adopted += 1
                return ["ADOPT", 0]
            dropped = self.drop()
        skip = int(bool(matrix and nodal_copy and self.promise and self.knod_current and have_target and not class_timing and f[:6] == target))
        self.promise = self.knod_current = 0
        if matrix:
            self.knod_skipped = skip
        if skip:
            self.n_skip += 1
            self.armed = 1
        return ["SKIP_COPY" if skip else "RUN", dropped]

    def U(self, x, same_target):
        return [int(self.fields_current and x == self.tail_x and same_target)]

    def R(self):
        self.n_tail = self.n_skip = self.n_adopted = self.n_discarded = 0
        return []


def _num(t):
    return int(t) if t.lstrip("-").isdigit() else t


@pytest.fixture(scope="module")
def seqs(tmp_path_factory):
    """{sequence name: [(event, args, returned, state after)]} as the program printed them."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    probe = subprocess.run("echo 'int main(){return 0;}' | g++ -x c++ -fsanitize=address,undefined - -o /dev/null", shell=True, capture_output=True)
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if probe.returncode == 0 else []
    exe = str(tmp_path_factory.mktemp("step_state") / "step_state_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + san + ["-I" + os.path.join(ROOT, "knp-emi-cgx_amd", "csrc"),
                    os.path.join(ROOT, "tools", "step_state_check.cpp"), "-o", exe], check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out, cur = {}, None
    for ln in r.stdout.splitlines():
        t = ln.split()
        if t[0] == "seq":
            assert t[1] not in out
            cur = out[t[1]] = []
            continue
        assert t[0] == "ev", ln
        bar, eq = t.index("|"), t.index("=")
        cur.append((t[1], tuple(map(_num, t[2:bar])), list(map(_num, t[bar + 1:eq])), tuple(map(int, t[eq + 1:]))))
    return out


def test_every_line_follows_the_table(seqs):
    n = 0
    for name, events in seqs.items():
        m = Model()
        for i, (ev, args, ret, state) in enumerate(events):
            if ev == "S":
                assert m.M() == [1], (name, i, "a speculation where the protocol allows none")
            want = getattr(m, ev)(*args)
            assert ret == want, (name, i, ev, args, ret, want)
            assert state == m.state(), (name, i, ev, args, dict(zip(FLAGS, state)), dict(zip(FLAGS, m.state())))
            n += 1
    assert n > 10000


def test_the_walk_reaches_every_event_and_every_outcome(seqs):
    walk = seqs["walk"]
    assert len(walk) >= 10000
    assert {ev for ev, *_ in walk} == set("XTIPDMSAUR")
    count = {}
    for ev, args, ret, _ in walk:
        key = (ev, args[0] if ev == "A" else None, tuple(ret))
        count[key] = count.get(key, 0) + 1
    for key in [("A", 1, ("ADOPT", 0)), ("A", 1, ("SKIP_COPY", 0)), ("A", 1, ("SKIP_COPY", 1)), ("A", 1, ("RUN", 0)), ("A", 1, ("RUN", 1)), ("A", 0, ("RUN", 0)),
                ("X", None, (0,)), ("X", None, (1,)), ("T", None, (1,)), ("I", None, (1,)), ("M", None, (0,)), ("M", None, (1,)), ("U", None, (0,)), ("U", None, (1,))]:
        assert count.get(key, 0) >= 10, (key, count.get(key, 0))
    assert not any(k[0] == "A" and k[1] == 0 and k[2] != ("RUN", 0) for k in count), "the preconditioner's pass only ever runs"


def _last(seqs, name):
    ev, args, ret, state = seqs[name][-1]
    return ret, dict(zip(FLAGS, state))


def _returns(seqs, name, ev):
    return [ret for e, _, ret, _ in seqs[name] if e == ev]


def test_rows_of_the_table(seqs):
    ret, s = _last(seqs, "row_x_changing")
    assert ret == [1] and (s["fields_current"], s["knod_current"], s["pending"], s["armed"], s["n_discarded"]) == (0, 0, 0, 0, 1)
    ret, s = _last(seqs, "row_target_changing")
    assert ret == [1] and (s["fields_current"], s["knod_current"], s["promise"], s["pending"], s["n_discarded"]) == (0, 0, 0, 0, 1)
    ret, s = _last(seqs, "row_inputs_changing")
    assert ret == [1] and (s["fields_current"], s["knod_current"], s["promise"], s["pending"], s["armed"], s["n_discarded"]) == (1, 1, 1, 0, 0, 1)
    assert _last(seqs, "row_promise")[1]["promise"] == 1
    _, s = _last(seqs, "row_tail_done")
    assert (s["tail_x"], s["fields_current"], s["knod_current"], s["n_tail"]) == (9, 1, 0, 2)
    assert seqs["row_speculated"][-1][0] == "S" and _last(seqs, "row_speculated")[1]["pending"] == 1
    assert _last(seqs, "row_begin_assembly")[0] == ["SKIP_COPY", 0]
    assert _last(seqs, "row_unpack_is_current")[0] == [1]
    before, after = seqs["row_reset_counters"][-2][3], seqs["row_reset_counters"][-1][3]
    assert before[:6] == (1,) * 6 and all(c > 0 for c in before[7:]), "every flag set and every counter counting before the reset"
    assert after[:7] == before[:7] and after[7:] == (0, 0, 0, 0)


def test_the_copy_pass_is_skipped_only_on_promise_current_copy_and_the_targets_pointers(seqs):
    ret, s = _last(seqs, "skip_copy")
    assert ret == ["SKIP_COPY", 0] and (s["armed"], s["n_skip"], s["knod_skipped"], s["promise"], s["knod_current"]) == (1, 1, 1, 0, 0)
    for name in ("skip_no_promise", "skip_other_conc", "skip_no_knod", "skip_no_nodal_copy", "skip_no_target", "skip_class_timing"):
        ret, s = _last(seqs, name)
        assert ret == ["RUN", 0] and (s["armed"], s["n_skip"], s["knod_skipped"], s["promise"], s["knod_current"]) == (0, 0, 0, 0, 0), name
    assert _last(seqs, "skip_other_phim_still_skips")[0] == ["SKIP_COPY", 0]   # the copy holds concentrations only
    assert _returns(seqs, "promise_consumed_by_run", "A") == [["RUN", 0], ["RUN", 0]]
    assert _returns(seqs, "promise_consumed_by_skip", "A") == [["SKIP_COPY", 0], ["RUN", 0]]
    ret, s = _last(seqs, "run_leaves_armed")
    assert ret == ["RUN", 0] and (s["armed"], s["knod_skipped"]) == (1, 0)
    ret, s = _last(seqs, "precond_pass")
    assert ret == ["RUN", 0] and (s["knod_current"], s["promise"], s["knod_skipped"], s["armed"], s["fields_current"], s["n_skip"]) == (0, 0, 1, 1, 1, 1)


def test_adoption_and_the_ways_to_lose_it(seqs):
    ret, s = _last(seqs, "adopt")
    assert ret == ["ADOPT", 0]
    assert (s["pending"], s["armed"], s["knod_skipped"], s["promise"], s["knod_current"], s["n_skip"], s["n_adopted"], s["n_discarded"]) == (0, 1, 1, 0, 0, 2, 1, 0)
    ret, s = _last(seqs, "drop_no_promise")
    assert ret == ["RUN", 1] and (s["pending"], s["armed"], s["n_discarded"], s["n_adopted"], s["n_skip"]) == (0, 0, 1, 0, 1)
    for name in ("drop_other_phim", "drop_other_dt", "drop_form"):   # dropped, joined, counted -- and the copy pass still skipped, which arms again
        ret, s = _last(seqs, name)
        assert ret == ["SKIP_COPY", 1] and (s["pending"], s["armed"], s["n_discarded"], s["n_adopted"], s["n_skip"]) == (0, 1, 1, 0, 2), name
    assert _returns(seqs, "drop_twice", "I") == [[1], [0]] and _returns(seqs, "drop_twice", "X") == [[0], [0]] and _returns(seqs, "drop_twice", "T") == [[0]]
    assert _last(seqs, "drop_twice")[1]["n_discarded"] == 1
    ret, s = _last(seqs, "precond_pass_ignores_pending")
    assert ret == ["RUN", 0] and (s["pending"], s["armed"], s["n_discarded"]) == (1, 1, 0)


def test_invalidating_events_between_tail_and_assembly(seqs):
    assert _last(seqs, "between_x")[0] == ["RUN", 0]
    assert _last(seqs, "between_target")[0] == ["RUN", 0]
    assert _returns(seqs, "between_inputs", "U") == [[1]] and _last(seqs, "between_inputs")[0] == ["SKIP_COPY", 0]
    assert _returns(seqs, "between_precond", "U") == [[1]] and _last(seqs, "between_precond")[0] == ["RUN", 0]


def test_unpack_shortcut(seqs):
    assert _returns(seqs, "unpack", "U") == [[0], [1], [0], [0], [0]]
