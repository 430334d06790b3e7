// Membrane state variables (knp_state_*): every state a mechanism declares is one bytecode program (the opcodes of knp_set_program),
// and one kernel advances all of them by one PDE step at every vertex.  Included at the end of knp_kernels.hip, after run_program and the
// host helpers (validate_program, dev_upload, dev_free) it uses.
//
// One PDE step (the reference's Hodgkin-Huxley update, KNPEMIx_ionic_model.py:605-671, for any mechanism):
//   gate (kind 0, OUT 0 = alpha, OUT 1 = beta), dy/dt = alpha (1 - y) - beta y: alpha and beta are evaluated once, from the values at
//     the start of the step.  Rush-Larsen: y <- y_inf + (y - y_inf) exp(-dt (alpha + beta)) at the end of the step (the sub-steps of a
//     frozen-rate exponential step collapse, as in k_hh_update); where alpha + beta == 0 the gate stays as it is.  Forward Euler: `substeps` steps y += dto alpha (1 - y) - dto beta y.
//   general state (kind 1, OUT 0 = dy/dt): `substeps` forward-Euler steps, the program evaluated again in each.
//   In a sub-step every program reads the states as they stood at its beginning; all states advance at its end.
//
// k_state_update: one vertex per lane, STATE_BT lanes per block.  Dynamic LDS: [n_regs][STATE_BT] register file of the interpreter (one
// column per lane, as in k_diag_facets) | the constants of all programs | the code of all programs, staged once per block.  The block
// runs the programs one after the other, so every wave executes the same instruction words (run_program's contract).  Lanes past
// `count` stay alive -- there is a barrier after the staging -- shadow vertex count-1 and store nothing.  The states live in registers
// across the sub-steps: one load and one store per state and vertex.  Per-lane arrays are indexed by unrolled loops only (no scratch).
// LDS: at most 48 registers x 128 lanes x 8 B = 48 KiB, 1 KiB of constants and 12 KiB of code: 61 KiB.

static constexpr int STATE_BT = 128;
struct StateArgs {
    double consts[KNP_STATE_MAX_CONSTS];   // the programs' constants, one after the other in slot order
    double* y[KNP_MAX_AUX];                // the state buffers, by slot
    const double* aux[KNP_MAX_AUX];        // aux fields that are not states (null: a state's slot, or absent -- read as 0)
    const double* ki[3];
    const double* ke[3];                   // read only when use_k
    int32_t code_off[KNP_MAX_AUX], n_instr[KNP_MAX_AUX], const_off[KNP_MAX_AUX], kind[KNP_MAX_AUX], aux_index[KNP_MAX_AUX];
};

template <int DIM, bool FUNCS = false>
__global__ void __launch_bounds__(STATE_BT) k_state_update(int count, int n_states, int n_iter, StateArgs S, const double* __restrict__ phim,
                                                           int use_k, const double* __restrict__ coords, const int32_t* __restrict__ code,
                                                           int total_instr, int total_consts, int n_regs, double dt, double dto,
                                                           int rush_larsen) {
    extern __shared__ __align__(16) double ssmem[];
    double* sk = ssmem + (size_t)n_regs * STATE_BT;
    int32_t* scode = reinterpret_cast<int32_t*>(sk + ((total_consts + 1) & ~1));   // even: the code stays 16-B aligned
    for (int i = threadIdx.x; i < total_consts; i += STATE_BT) sk[i] = S.consts[i];
    for (int i = threadIdx.x; i < total_instr; i += STATE_BT)
        reinterpret_cast<int4*>(scode)[i] = reinterpret_cast<const int4*>(code)[i];
    __syncthreads();      // the only barrier: no lane has left before it, none leaves before the stores at the end
    const int i = blockIdx.x * STATE_BT + threadIdx.x;
    const bool live = i < count;
    const int v = live ? i : count - 1;   // idle lanes shadow the last vertex: the interpreter's wave stays uniform
    double kiq[1][3], keq[1][3], phq[1], auxq[1][KNP_MAX_AUX], xq[1][3], Iout[1][3];
    phq[0] = phim[v];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        kiq[0][j] = use_k ? S.ki[j][v] : 0.0;
        keq[0][j] = use_k ? S.ke[j][v] : 0.0;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) xq[0][d] = d < DIM ? coords[(size_t)v * DIM + d] : 0.0;
#pragma unroll
    for (int k = 0; k < KNP_MAX_AUX; ++k) auxq[0][k] = S.aux[k] ? S.aux[k][v] : 0.0;
    double y[KNP_MAX_AUX], o0[KNP_MAX_AUX], o1[KNP_MAX_AUX];   // state, OUT 0 and OUT 1 of its program
#pragma unroll
    for (int s = 0; s < KNP_MAX_AUX; ++s) {
        y[s] = s < n_states ? S.y[s][v] : 0.0;
        o0[s] = o1[s] = 0.0;
    }
    double* reg = ssmem + threadIdx.x;
    for (int it = 0; it < n_iter; ++it) {
#pragma unroll
        for (int s = 0; s < KNP_MAX_AUX; ++s)      // the states as the programs of this sub-step read them
#pragma unroll
            for (int k = 0; k < KNP_MAX_AUX; ++k)
                if (s < n_states && S.aux_index[s] == k) auxq[0][k] = y[s];
        for (int s = 0; s < n_states; ++s) {
            if (it > 0 && S.kind[s] == 0) continue;      // a gate's rates are those of the start of the step
            Iout[0][0] = Iout[0][1] = Iout[0][2] = 0.0;
            run_program<1, STATE_BT, FUNCS>(scode + 4 * S.code_off[s], S.n_instr[s], sk + S.const_off[s], kiq, keq, phq, auxq, xq, Iout, reg);
#pragma unroll
            for (int j = 0; j < KNP_MAX_AUX; ++j)
                if (j == s) { o0[j] = Iout[0][0]; o1[j] = Iout[0][1]; }
        }
#pragma unroll
        for (int s = 0; s < KNP_MAX_AUX; ++s) {
            if (s >= n_states) continue;
            if (S.kind[s] == 1) y[s] += dto * o0[s];
            else if (!rush_larsen) y[s] += dto * o0[s] * (1.0 - y[s]) - dto * o1[s] * y[s];
        }
    }
#pragma unroll
    for (int s = 0; s < KNP_MAX_AUX; ++s) {
        if (s >= n_states) continue;
        if (rush_larsen && S.kind[s] == 0) {
            const double t = o0[s] + o1[s], yinf = o0[s] / t;
            if (t != 0.0) y[s] = yinf + (y[s] - yinf) * exp(-dt * t);      // both rates zero: dy/dt = 0, not 0 / 0
        }
        if (live) S.y[s][i] = y[s];
    }
}

void knp_state_free(knp_ctx* ctx) {
    dev_free(ctx->states.d_code);
    ctx->states.progs.clear();
    ctx->states.dirty = true;
}

static int state_slot(knp_ctx* ctx, int32_t slot) {
    if (slot < 0 || slot >= (int)ctx->states.progs.size()) { ctx->err = "state slot out of range (knp_state_reset sets the number of states)"; return KNP_E_ARG; }
    return KNP_OK;
}

extern "C" {

int knp_state_reset(knp_ctx* ctx, int32_t n_states) {
    CHECK_CTX(ctx);
    if (n_states < 0 || n_states > KNP_MAX_AUX) { ctx->err = "the number of states must be 0.." + std::to_string(KNP_MAX_AUX) + " (each takes an aux slot)"; return KNP_E_ARG; }
    HIPCHK(hipStreamSynchronize(ctx->stream));   // an update in flight may still read the old code
    knp_state_free(ctx);
    ctx->states.progs.resize((size_t)n_states);
    return KNP_OK;
}

int knp_state_set_program(knp_ctx* ctx, int32_t slot, int32_t kind, int32_t aux_index, int32_t n_instr, const int32_t* code, int32_t n_consts,
                          const double* consts) {
    CHECK_CTX(ctx);
    KCHK(state_slot(ctx, slot));
    KnpStates& st = ctx->states;
    if (kind != 0 && kind != 1) { ctx->err = "state kind must be 0 (gate) or 1 (general)"; return KNP_E_ARG; }
    if (aux_index < 0 || aux_index >= KNP_MAX_AUX) { ctx->err = "state aux_index must be below KNP_MAX_AUX"; return KNP_E_ARG; }
    if (n_instr <= 0 || !code || n_consts < 0 || (n_consts && !consts)) { ctx->err = "bad state program arguments"; return KNP_E_ARG; }
    int64_t instr = n_instr, nc = n_consts;
    for (int s = 0; s < (int)st.progs.size(); ++s) {
        if (s == slot || !st.progs[s].set) continue;
        if (st.progs[s].aux_index == aux_index) { ctx->err = "two states share aux slot " + std::to_string(aux_index); return KNP_E_ARG; }
        instr += (int)st.progs[s].code.size() / 4;
        nc += (int)st.progs[s].consts.size();
    }
    if (instr > KNP_STATE_MAX_INSTR || nc > KNP_STATE_MAX_CONSTS) {
        ctx->err = "state programs too long: together at most " + std::to_string(KNP_STATE_MAX_INSTR) + " instructions and " +
                   std::to_string(KNP_STATE_MAX_CONSTS) + " constants";
        return KNP_E_ARG;
    }
    int n_regs = 0;
    KCHK(validate_program(ctx, n_instr, code, n_consts, &n_regs));
    KnpStateProg& p = st.progs[slot];
    p.kind = kind;
    p.aux_index = aux_index;
    p.n_regs = n_regs;
    p.uses_k = false;
    p.funcs = program_uses_funcs(n_instr, code);
    for (int i = 0; i < n_instr; ++i) p.uses_k = p.uses_k || code[4 * i] == KNP_OP_KI || code[4 * i] == KNP_OP_KE;
    p.code.assign(code, code + (size_t)4 * n_instr);
    p.consts.assign(consts, consts + n_consts);
    p.set = true;
    st.dirty = true;
    return KNP_OK;
}

int knp_state_set_constants(knp_ctx* ctx, int32_t slot, int32_t n_consts, const double* consts) {
    CHECK_CTX(ctx);
    KCHK(state_slot(ctx, slot));
    KnpStateProg& p = ctx->states.progs[slot];
    if (!p.set || n_consts != (int)p.consts.size() || (n_consts && !consts)) { ctx->err = "state program / constant count mismatch"; return KNP_E_ARG; }
    for (int i = 0; i < n_consts; ++i) p.consts[i] = consts[i];   // kernel arguments of the next update: nothing to copy
    return KNP_OK;
}

int knp_state_update(knp_ctx* ctx, const knp_fields* fields, double* const* state, int32_t count, double dt, int32_t rush_larsen,
                     int32_t substeps) {
    CHECK_CTX(ctx);
    KnpStates& st = ctx->states;
    const int n_states = (int)st.progs.size();
    if (n_states == 0) { ctx->err = "no states (knp_state_reset / knp_state_set_program)"; return KNP_E_STATE; }
    for (int s = 0; s < n_states; ++s)
        if (!st.progs[s].set) { ctx->err = "state program " + std::to_string(s) + " not set (knp_state_set_program)"; return KNP_E_STATE; }
    if (!fields || !fields->phi_m) { ctx->err = "null fields or null phi_m field"; return KNP_E_ARG; }
    if (!state) { ctx->err = "null state pointer array"; return KNP_E_ARG; }
    if (count < 0 || count > ctx->g.n_v) { ctx->err = "state count must be 0..the number of local vertices"; return KNP_E_ARG; }
    if (substeps < 1 || !(dt > 0)) { ctx->err = "bad state_update arguments (dt > 0, substeps >= 1)"; return KNP_E_ARG; }
    StateArgs S;
    std::memset(&S, 0, sizeof(S));
    bool use_k = false, any_general = false, funcs = false;
    int n_regs = 1, total_instr = 0, total_consts = 0;
    for (int k = 0; k < KNP_MAX_AUX; ++k) S.aux[k] = fields->aux[k];
    for (int s = 0; s < n_states; ++s) {
        const KnpStateProg& p = st.progs[s];
        if (!state[s]) { ctx->err = "null state buffer " + std::to_string(s); return KNP_E_ARG; }
        S.y[s] = state[s];
        S.aux[p.aux_index] = nullptr;     // the programs read the state itself under this slot
        S.code_off[s] = total_instr;
        S.n_instr[s] = (int)p.code.size() / 4;
        S.const_off[s] = total_consts;
        S.kind[s] = p.kind;
        S.aux_index[s] = p.aux_index;
        for (size_t i = 0; i < p.consts.size(); ++i) S.consts[total_consts + i] = p.consts[i];
        total_instr += S.n_instr[s];
        total_consts += (int)p.consts.size();
        n_regs = std::max(n_regs, p.n_regs);
        use_k = use_k || p.uses_k;
        funcs = funcs || p.funcs;
        any_general = any_general || p.kind == 1;
    }
    if (use_k)
        for (int j = 0; j < 3; ++j) {
            if (!fields->k_i[j] || !fields->k_e[j]) { ctx->err = "a state program reads a concentration: null concentration field"; return KNP_E_ARG; }
            S.ki[j] = fields->k_i[j];
            S.ke[j] = fields->k_e[j];
        }
    if (count == 0) return KNP_OK;
    if (st.dirty) {
        std::vector<int32_t> all;
        for (const KnpStateProg& p : st.progs) all.insert(all.end(), p.code.begin(), p.code.end());
        HIPCHK(hipStreamSynchronize(ctx->stream));
        dev_free(st.d_code);
        KCHK(dev_upload(ctx, &st.d_code, all));
        st.dirty = false;
    }
    // Rush-Larsen gates alone: one evaluation, the exponential step at the end; else one pass per sub-step
    const int n_iter = (any_general || !rush_larsen) ? substeps : 1;
    const size_t lds = ((size_t)n_regs * STATE_BT + ((total_consts + 1) & ~1)) * sizeof(double) + (size_t)total_instr * 4 * sizeof(int32_t);
    ProfScope ps(ctx, 4);
    const unsigned nb = (unsigned)((count + STATE_BT - 1) / STATE_BT);
    by_dim(ctx->g.dim, [&](auto D) {
        with_flag(funcs, [&](auto M) {
            hipLaunchKernelGGL((k_state_update<D(), M()>), dim3(nb), dim3(STATE_BT), lds, ctx->stream, count, n_states, n_iter, S, fields->phi_m,
                               use_k ? 1 : 0, ctx->d_coords, st.d_code, total_instr, total_consts, n_regs, dt, dt / substeps,
                               rush_larsen ? 1 : 0);
        });
    });
    HIPCHK(hipGetLastError());
    return KNP_OK;
}

}  // extern "C"
