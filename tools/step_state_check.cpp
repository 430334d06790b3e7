// Host check of csrc/knp_step_state.hpp (tests/test_step_state_host.py compiles and runs it, under ASan/UBSan where they link).
// Scripted sequences, then a long walk over the whole event alphabet.  `seq NAME` starts from a fresh state; then one line per event:
//   ev X | ...                 x_changing()              -> dropped
//   ev T | ...                 target_changing()         -> dropped
//   ev I | ...                 inputs_changing()         -> dropped
//   ev P | ...                 promise()
//   ev D x w | ...             tail_done(x, w)
//   ev M | ...                 may_speculate()           -> yes
//   ev S f[7] dt | ...         speculated(f, dt)
//   ev A matrix f[7] nodal_copy have_target class_timing form_ok dt target[6] | ...   begin_assembly -> RUN / SKIP_COPY / ADOPT, dropped
//   ev U x same_target | ...   unpack_is_current         -> yes
//   ev R | ...                 reset_counters()
// and after the bar: the return values, `=`, then fields_current knod_current promise knod_skipped armed pending tail_x and the four
// counters (fused tails, skips, adopted, discarded).  Pointers print as indices into a pool, -1 for null; dt as an integer (tenths).
#include <cstdint>
#include <cstdio>

#include "knp_step_state.hpp"

static double pool[16];
static int id(const double* p) { return p ? (int)(p - pool) : -1; }

struct Fields { int v[7]; };   // k_i[3], k_e[3], phi_m as pool indices
static KnpStepFields fields(const Fields& f) {
    KnpStepFields s;
    for (int j = 0; j < 3; ++j) { s.k_i[j] = pool + f.v[j]; s.k_e[j] = pool + f.v[3 + j]; }
    s.phi_m = pool + f.v[6];
    return s;
}
static const Fields TARGET = {{0, 1, 2, 3, 4, 5, 6}};

struct Checker {
    KnpStepState s;
    void state() {
        std::printf(" = %d %d %d %d %d %d %d %lld %lld %lld %lld\n", s.fields_current(), s.knod_current(), s.promised(), s.copy_pass_skipped(), s.armed(),
                    s.pending(), id(s.tail_x()), (long long)s.fused_tails(), (long long)s.knod_skips(), (long long)s.ahead_adopted(),
                    (long long)s.ahead_discarded());
    }
    void seq(const char* name) { s = KnpStepState(); std::printf("seq %s\n", name); }
    void X() { const bool d = s.x_changing(); std::printf("ev X | %d", d); state(); }
    void T() { const bool d = s.target_changing(); std::printf("ev T | %d", d); state(); }
    void I() { const bool d = s.inputs_changing(); std::printf("ev I | %d", d); state(); }
    void P() { s.promise(); std::printf("ev P |"); state(); }
    void D(int x, bool w) { s.tail_done(pool + x, w); std::printf("ev D %d %d |", x, w); state(); }
    bool M() { const bool y = s.may_speculate(); std::printf("ev M | %d", y); state(); return y; }
    void S(const Fields& f, int dt) {
        s.speculated(fields(f), 0.1 * dt);
        std::printf("ev S");
        for (int v : f.v) std::printf(" %d", v);
        std::printf(" %d |", dt);
        state();
    }
    void A(bool matrix, const Fields& f, int dt, bool form_ok = true, bool nodal_copy = true, bool have_target = true, bool class_timing = false,
           const Fields& target = TARGET) {
        KnpAsmInputs in;
        in.nodal_copy = nodal_copy; in.have_target = have_target; in.class_timing = class_timing; in.form_ok = form_ok;
        in.dt = 0.1 * dt;
        in.target = fields(target);
        const KnpAsmBegin b = s.begin_assembly(matrix, fields(f), in);
        std::printf("ev A %d", matrix);
        for (int v : f.v) std::printf(" %d", v);
        std::printf(" %d %d %d %d %d", nodal_copy, have_target, class_timing, form_ok, dt);
        for (int j = 0; j < 6; ++j) std::printf(" %d", target.v[j]);
        std::printf(" | %s %d", b.what == KnpAsmDecision::ADOPT ? "ADOPT" : b.what == KnpAsmDecision::SKIP_COPY ? "SKIP_COPY" : "RUN", b.dropped);
        state();
    }
    void U(int x, bool same_target) { const bool y = s.unpack_is_current(pool + x, same_target); std::printf("ev U %d %d | %d", x, same_target, y); state(); }
    void R() { s.reset_counters(); std::printf("ev R |"); state(); }
    // a step that ended in the tail and whose next assembly took the skip path: the context is armed
    void arm() { D(8, true); P(); A(true, TARGET, 1); }
    // ... and the next solve's tail has assembled ahead
    void speculate() { arm(); X(); D(8, true); if (M()) S(TARGET, 1); }
};

static Fields with(Fields f, int slot, int v) { f.v[slot] = v; return f; }

int main() {
    Checker c;
    // one per row of the table
    c.seq("row_x_changing"); c.speculate(); c.X();
    c.seq("row_target_changing"); c.speculate(); c.P(); c.T();
    c.seq("row_inputs_changing"); c.speculate(); c.P(); c.I();
    c.seq("row_promise"); c.P(); c.P();
    c.seq("row_tail_done"); c.D(8, true); c.D(9, false);
    c.seq("row_speculated"); c.speculate();
    c.seq("row_begin_assembly"); c.arm();
    c.seq("row_unpack_is_current"); c.D(8, true); c.U(8, true);
    // (every flag set and every counter above zero when the reset comes)
    c.seq("row_reset_counters"); c.speculate(); c.P(); c.A(true, TARGET, 1); c.X(); c.D(8, true); c.M(); c.S(TARGET, 1); c.I();
    c.P(); c.A(true, TARGET, 1); c.X(); c.D(8, true); c.M(); c.S(TARGET, 1); c.P(); c.R();
    // the skip of the copy pass
    c.seq("skip_copy"); c.D(8, true); c.P(); c.A(true, TARGET, 1);
    c.seq("skip_no_promise"); c.D(8, true); c.A(true, TARGET, 1);
    c.seq("skip_other_conc"); c.D(8, true); c.P(); c.A(true, with(TARGET, 4, 12), 1);
    c.seq("skip_other_phim_still_skips"); c.D(8, true); c.P(); c.A(true, with(TARGET, 6, 12), 1);
    c.seq("skip_no_knod"); c.D(8, false); c.P(); c.A(true, TARGET, 1);
    c.seq("skip_no_nodal_copy"); c.D(8, true); c.P(); c.A(true, TARGET, 1, true, false);
    c.seq("skip_no_target"); c.D(8, true); c.P(); c.A(true, TARGET, 1, true, true, false);
    c.seq("skip_class_timing"); c.D(8, true); c.P(); c.A(true, TARGET, 1, true, true, true, true);
    c.seq("promise_consumed_by_run"); c.D(8, true); c.P(); c.A(true, with(TARGET, 0, 12), 1); c.D(8, true); c.A(true, TARGET, 1);
    c.seq("promise_consumed_by_skip"); c.D(8, true); c.P(); c.A(true, TARGET, 1); c.D(8, true); c.A(true, TARGET, 1);
    c.seq("run_leaves_armed"); c.arm(); c.A(true, TARGET, 1);
    c.seq("precond_pass"); c.arm(); c.D(8, true); c.P(); c.A(false, TARGET, 1);
    // adoption and the four ways to lose it
    c.seq("adopt"); c.speculate(); c.P(); c.A(true, TARGET, 1);
    c.seq("drop_no_promise"); c.speculate(); c.A(true, TARGET, 1);
    c.seq("drop_other_phim"); c.speculate(); c.P(); c.A(true, with(TARGET, 6, 12), 1);
    c.seq("drop_other_dt"); c.speculate(); c.P(); c.A(true, TARGET, 2);
    c.seq("drop_form"); c.speculate(); c.P(); c.A(true, TARGET, 1, false);
    c.seq("drop_twice"); c.speculate(); c.I(); c.I(); c.X(); c.T();
    c.seq("precond_pass_ignores_pending"); c.speculate(); c.P(); c.A(false, TARGET, 1);
    // every invalidating event between tail and assembly
    c.seq("between_x"); c.D(8, true); c.P(); c.X(); c.A(true, TARGET, 1);
    c.seq("between_target"); c.D(8, true); c.P(); c.T(); c.A(true, TARGET, 1);
    c.seq("between_inputs"); c.D(8, true); c.P(); c.I(); c.U(8, true); c.A(true, TARGET, 1);
    c.seq("between_precond"); c.D(8, true); c.P(); c.I(); c.A(false, TARGET, 1); c.U(8, true); c.P(); c.A(true, TARGET, 1);
    // the shortcut of knp_unpack
    c.seq("unpack"); c.U(8, true); c.D(8, false); c.U(8, true); c.U(9, true); c.U(8, false); c.X(); c.U(8, true);
    // the long walk: a small LCG picks the events; fields, dt and the context's inputs mostly as a steady caller passes them
    c.seq("walk");
    uint64_t lcg = 0x2545f4914f6cdd1dull;
    auto rnd = [&](int n) { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (int)((lcg >> 33) % (uint64_t)n); };
    auto some_fields = [&]() { return rnd(5) == 0 ? with(TARGET, rnd(7), 10 + rnd(3)) : TARGET; };
    for (int n = 0; n < 20000; ++n) {
        const int e = rnd(32);
        if (e < 7) c.D(8 + (rnd(8) == 0), rnd(8) != 0);
        else if (e < 13) c.P();
        else if (e < 20) c.A(rnd(12) != 0, some_fields(), rnd(8) == 0 ? 2 : 1, rnd(10) != 0, rnd(10) != 0, rnd(10) != 0, rnd(10) == 0, rnd(12) == 0 ? some_fields() : TARGET);
        else if (e < 25) { if (c.M()) c.S(some_fields(), rnd(8) == 0 ? 2 : 1); }
        else if (e < 27) c.U(8 + (rnd(4) == 0), rnd(4) != 0);
        else if (e < 28) c.X();
        else if (e < 29) c.I();
        else if (e < 30) c.T();
        else if (e < 31) c.R();
        else c.A(false, some_fields(), 1);
    }
    return 0;
}
