// The bookkeeping between the end of one solve and the next step's assembly, in one place (host code only; no HIP includes and no
// knp_ctx, so that the host compiler alone can test it: tools/step_state_check.cpp).  knp_ctx has one member of this type, `step`,
// and nothing outside this header reads or writes a flag of it: the entry points call the transitions below and ask the queries.
//
// What the flags mean.  The tail of a solve (k_lincomb_unpack) leaves the fields of the registered unpack target equal to
// unpack(tail_x) (`fields_current`) and, where the assembly keeps a node-indexed concentration copy, that copy equal to the
// concentrations of tail_x (`knod_current`).  `promise`: the caller vouches that nobody wrote the concentration fields since
// (knp_fields_unchanged); one shot.  `knod_skipped`: the last matrix assembly did not run the copy pass k_nodal_conc
// (knp_get_traffic_model).  `armed`: set by every matrix assembly that skipped the copy pass or adopted a speculation, cleared by
// every discard and by nothing else -- a matrix assembly that runs the copy pass leaves it as it was.  While armed, the tail of a
// solve may enqueue the next step's matrix assembly on the assembly stream (`pending`, with the field pointers and dt it read).
//
//   event (who raises it)                                          effect
//   x_changing()       krylov_begin, knp_project_nullspace,        clears fields_current and knod_current; drops a pending speculation
//                      knp_pack, knp_set_dirichlet, knp_pc_setup,
//                      a knp_unpack that runs k_unpack
//   target_changing()  knp_set_unpack_target                       as x_changing(), and clears the promise
//   inputs_changing()  knp_set_params; knp_assemble_precond        drops a pending speculation only
//                      before it rewrites the concentration copy
//   promise()          knp_fields_unchanged                        sets the promise
//   tail_done(x, w)    behind k_lincomb_unpack                     tail_x = x, fields_current, knod_current = w, counts a fused tail
//   speculated(f, dt)  end of speculate_asm                        records f and dt; pending
//   begin_assembly()   top of knp_assemble_matrix(_async);         decides ADOPT / SKIP_COPY / RUN (below) and says whether a speculation
//                      the cell-means pass of                      was dropped on the way; consumes the promise and knod_current whatever
//                      knp_assemble_precond (matrix = false)       the outcome; sets knod_skipped for the matrix form only; arms on
//                                                                  SKIP_COPY and ADOPT; counts skips, adoptions, discards
//   unpack_is_current(x, same_target)   knp_unpack                 true: the tail has written exactly this, nothing to launch
//   may_speculate()    speculate_asm                               armed, knod_current, nothing pending
//   reset_counters()   knp_profile_reset                           the four counters only
//
// A transition that can drop a speculation returns true when it did: the caller then joins the assembly stream (drop_ahead in
// knp_kernels.hip), since the dropped kernels read the fields and the concentration copy and use the facet matrices as scratch.
// Nothing here touches a stream.
#pragma once
#include <cstdint>

// the field pointers an assembly reads (knp_fields without the auxiliary fields)
struct KnpStepFields {
    const double* k_i[3] = {nullptr, nullptr, nullptr};
    const double* k_e[3] = {nullptr, nullptr, nullptr};
    const double* phi_m = nullptr;
    template <typename F>   // knp_fields, knp_fields_out
    static KnpStepFields of(const F& f) {
        KnpStepFields s;
        for (int j = 0; j < 3; ++j) { s.k_i[j] = f.k_i[j]; s.k_e[j] = f.k_e[j]; }
        s.phi_m = f.phi_m;
        return s;
    }
    bool same_conc(const KnpStepFields& o) const {
        for (int j = 0; j < 3; ++j)
            if (k_i[j] != o.k_i[j] || k_e[j] != o.k_e[j]) return false;
        return true;
    }
};

// what begin_assembly needs from the context
struct KnpAsmInputs {
    bool nodal_copy = false;     // the assembly reads the node-indexed concentration copy (asm_dmax > 0)
    bool have_target = false;    // an unpack target is registered
    bool class_timing = false;   // kernel classes beyond the SpMV's are being timed: every pass runs, so that it is timed
    bool form_ok = false;        // the assembly asked for is the form that may run ahead (ahead_form_ok)
    double dt = 0.0;
    KnpStepFields target;        // the concentration fields of the unpack target (meaningful with have_target)
};

enum class KnpAsmDecision {
    RUN,         // launch the copy pass (or the per-cell means) and the assembly
    SKIP_COPY,   // the concentration copy is the tail's: launch the assembly without the copy pass
    ADOPT        // the speculative assembly is the one asked for: swap the buffers, launch nothing
};
struct KnpAsmBegin {
    KnpAsmDecision what;
    bool dropped;   // a pending speculation was discarded: join the assembly stream
};

class KnpStepState {
public:
    bool x_changing() {
        fields_current_ = knod_current_ = false;
        return drop();
    }
    bool target_changing() {
        promise_ = false;
        return x_changing();
    }
    bool inputs_changing() { return drop(); }
    void promise() { promise_ = true; }
    void tail_done(const double* x, bool knod_written) {
        tail_x_ = x;
        fields_current_ = true;
        knod_current_ = knod_written;
        ++n_fused_tail_;
    }
    void speculated(const KnpStepFields& f, double dt) {
        pending_ = true;
        ahead_ = f;
        ahead_dt_ = dt;
    }
    // ADOPT: a speculation is pending, the caller gave the promise, the concentration copy is still the tail's, the form is still
    // eligible and these are the recorded pointers (phi_m included) and dt.  A pending speculation that fails any of these is
    // dropped, and the decision goes on as if there had been none.  SKIP_COPY: promise, copy current, these are the concentration
    // fields of the unpack target, no class timing.  The preconditioner's pass (matrix = false) always runs.
    KnpAsmBegin begin_assembly(bool matrix, const KnpStepFields& f, const KnpAsmInputs& in) {
        KnpAsmBegin r{KnpAsmDecision::RUN, false};
        if (matrix && pending_) {
            if (promise_ && knod_current_ && in.form_ok && ahead_dt_ == in.dt && f.phi_m == ahead_.phi_m && f.same_conc(ahead_)) {
                pending_ = promise_ = knod_current_ = false;
                knod_skipped_ = armed_ = true;   // (armed already: only an armed context speculates, and every disarming drops)
                ++n_knod_skip_;                  // counted where the caller's assembly is: the copy pass it would have run is the one skipped
                ++n_ahead_adopted_;
                r.what = KnpAsmDecision::ADOPT;
                return r;
            }
            r.dropped = drop();
        }
        const bool skip = matrix && in.nodal_copy && promise_ && knod_current_ && in.have_target && !in.class_timing && f.same_conc(in.target);
        promise_ = knod_current_ = false;
        if (matrix) knod_skipped_ = skip;
        if (skip) {
            ++n_knod_skip_;
            armed_ = true;   // the next solve's tail may assemble ahead
            r.what = KnpAsmDecision::SKIP_COPY;
        }
        return r;
    }
    bool unpack_is_current(const double* x, bool same_target) const { return fields_current_ && x == tail_x_ && same_target; }
    bool may_speculate() const { return armed_ && knod_current_ && !pending_; }
    void reset_counters() { n_fused_tail_ = n_knod_skip_ = n_ahead_adopted_ = n_ahead_discarded_ = 0; }

    // read-outs (knp_get_stats, knp_get_traffic_model, the host test)
    bool fields_current() const { return fields_current_; }
    bool knod_current() const { return knod_current_; }
    bool promised() const { return promise_; }
    bool copy_pass_skipped() const { return knod_skipped_; }
    bool armed() const { return armed_; }
    bool pending() const { return pending_; }
    const double* tail_x() const { return tail_x_; }
    int64_t fused_tails() const { return n_fused_tail_; }          // solves that ended in k_lincomb_unpack
    int64_t knod_skips() const { return n_knod_skip_; }            // matrix assemblies that skipped k_nodal_conc, adopted ones included
    int64_t ahead_adopted() const { return n_ahead_adopted_; }
    int64_t ahead_discarded() const { return n_ahead_discarded_; }

private:
    bool drop() {   // a second drop of the same speculation does nothing
        if (!pending_) return false;
        pending_ = armed_ = false;
        ++n_ahead_discarded_;
        return true;
    }
    const double* tail_x_ = nullptr;
    bool fields_current_ = false, knod_current_ = false, promise_ = false;
    bool knod_skipped_ = false, armed_ = false, pending_ = false;
    KnpStepFields ahead_;
    double ahead_dt_ = 0.0;
    int64_t n_fused_tail_ = 0, n_knod_skip_ = 0, n_ahead_adopted_ = 0, n_ahead_discarded_ = 0;
};
