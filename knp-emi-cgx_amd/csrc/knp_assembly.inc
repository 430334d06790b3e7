// Host side of the assembly (included by knp_kernels.hip, inside its extern "C" block, behind the kernels it launches): the field checks,
// the matrix assembly on a stream, its speculative form ahead of the caller (KNP_ASM_AHEAD) with the glue to the step state
// (knp_step_state.hpp), and the entry points knp_assemble_matrix, knp_assemble_matrix_async, knp_assemble_precond, knp_assemble_rhs.

static int check_fields(knp_ctx* ctx, const knp_fields* f, bool need_phim) {
    if (!f) { ctx->err = "null fields"; return KNP_E_ARG; }
    for (int j = 0; j < 3; ++j)
        if (!f->k_i[j] || !f->k_e[j]) { ctx->err = "null concentration field"; return KNP_E_ARG; }
    if (need_phim && !f->phi_m) { ctx->err = "null phi_m field"; return KNP_E_ARG; }
    if (!(ctx->dt > 0)) { ctx->err = "knp_set_params has not been called"; return KNP_E_STATE; }
    return KNP_OK;
}

// cc = psi / (sum_j z_j^2 k_j) / M_lumped at every owned node (Schur term of the block-triangular preconditioner)
// Only the block-triangular forms read cc (k_level_up MODE 1, k_schur_fin): skipped for the kinds that never do.  Before knp_pc_setup
// (kind NONE) it is written, so that a block-triangular setup after the first assembly finds it.
static void launch_schur_diag(knp_ctx* ctx, const FieldPtrs& f) {
    if (ctx->pc_kind == KNP_PC_AMG || ctx->pc_kind == KNP_PC_VBJACOBI) { ctx->have_cc = false; return; }
    const KnpHostGraph& g = ctx->g;
    hipLaunchKernelGGL(k_schur_diag, dim3(nblocks(g.n_nodes_owned)), dim3(NT), 0, ctx->stream, g.n_nodes_owned, ctx->psi, ctx->z[0], ctx->z[1],
                       ctx->z[2], ctx->d_node_vertex, ctx->d_node_side, f, ctx->d_ML, ctx->d_cc);
    ctx->have_cc = true;
}

// join the matrix assembly that runs on its own stream (knp_assemble_matrix_async): everything that reads A, or writes what
// that assembly reads or uses as scratch (the cell means, the facet matrices), calls this first
static int join_asm(knp_ctx* ctx) {
    if (ctx->asm_pending) {
        HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_asm, 0));
        ctx->asm_pending = false;
    }
    return KNP_OK;
}

// `at`, `ax`: where the solution-dependent entries go (ctx->d_at / d_ax, or the alternate pair of a speculative assembly, which is
// the time-dependent form only).  `knod_ready`: d_knod holds these fields' concentrations already (begin_assembly said SKIP_COPY, or
// the speculation runs right behind the tail that wrote it)
static int assemble_matrix_on_stream(knp_ctx* ctx, const knp_fields* fields, bool with_schur_diag, double* at, double* ax, bool knod_ready) {
    const KnpHostGraph& g = ctx->g;
    const DevParams P = make_params(ctx);
    FieldPtrs f = make_fields(fields);
    ProfScope ps(ctx, 3);
    if (!knod_ready) launch_cell_means(ctx, f);
    // The (k,k) and (phi,k) blocks do not depend on the previous solution (SURVEY 3.2 obs. 1): after the first
    // assembly only the K[k_prev]-type and membrane entries are rewritten, unless KNP_ASM_FULL=1 asks for the
    // reference's behaviour (A.zeroEntries() + full re-assembly, KNPEMIx_solver.py:110-115).
    const bool td_only = ctx->have_A && !ctx->asm_full && ctx->asm_dt == ctx->dt;
    if (td_only) launch_assemble_nodes<false, true>(ctx, P, at, ctx->d_ac);
    else launch_assemble_nodes<false, false>(ctx, P, at, ctx->d_ac);
    ctx->asm_dt = ctx->dt;
    if (g.n_g > 0) {
        if (g.dim == 2)
            hipLaunchKernelGGL((k_gamma_facets<2, true, false, 8, 1, NT, 1>), dim3(nblocks((int64_t)g.n_g * 8)), dim3(NT), 0, ctx->stream, g.n_g, g.n_q, P,
                               ctx->d_fv, ctx->d_fmeas, ctx->d_qp, ctx->d_qw, f, 0, ctx->d_coords, ctx->d_gamma_prog,
                               (const int32_t* const*)nullptr, (const int32_t*)nullptr, (const double* const*)nullptr,
                               (const int32_t*)nullptr, 0, 0, ctx->d_fmat, ctx->d_fvec);
        else if (gamma_many(g)) {  // 4 lanes per facet: the 36 points exactly (see gamma_many)
            // (matrix part: 9 points in flight per lane 0.76 ms on 1.5 M facets, 3 points 0.82, 1 point 0.95 -- unlike the mechanism currents)
            hipLaunchKernelGGL((k_gamma_facets<3, true, false, 4, 9, 64, 1>), dim3((unsigned)(((int64_t)g.n_g * 4 + 63) / 64)), dim3(64), 0, ctx->stream, g.n_g, g.n_q, P,
                               ctx->d_fv, ctx->d_fmeas, ctx->d_qp, ctx->d_qw, f, 0, ctx->d_coords, ctx->d_gamma_prog,
                               (const int32_t* const*)nullptr, (const int32_t*)nullptr, (const double* const*)nullptr,
                               (const int32_t*)nullptr, 0, 0, ctx->d_fmat, ctx->d_fvec);
        }
        else
            hipLaunchKernelGGL((k_gamma_facets<3, true, false, 16, 3, 64, 2>), dim3((unsigned)(((int64_t)g.n_g * 16 + 63) / 64)), dim3(64), 0, ctx->stream, g.n_g, g.n_q, P,
                               ctx->d_fv, ctx->d_fmeas, ctx->d_qp, ctx->d_qw, f, 0, ctx->d_coords, ctx->d_gamma_prog,
                               (const int32_t* const*)nullptr, (const int32_t*)nullptr, (const double* const*)nullptr,
                               (const int32_t*)nullptr, 0, 0, ctx->d_fmat, ctx->d_fvec);
        if (ctx->n_gp)
            hipLaunchKernelGGL((k_gamma_pairs<false>), dim3(nblocks(ctx->n_gp)), dim3(NT), 0, ctx->stream, ctx->n_gp, g.n_g, g.dim, P,
                               ctx->d_grow, ctx->d_gptr, ctx->d_gv_node_i, ctx->d_gv_node_e, ctx->d_gq_i, ctx->d_gq_e,
                               ctx->d_gcptr, ctx->d_gc_facet, ctx->d_gc_lab, ctx->d_fmeas, ctx->d_fmat, ctx->d_pair_ptr,
                               at, ax);
    }
    if (ctx->n_bc > 0)
        hipLaunchKernelGGL(k_dirichlet_rows_A, dim3(nblocks(ctx->n_bc)), dim3(NT), 0, ctx->stream, ctx->n_bc, ctx->d_bc_dofs, ctx->d_pair_ptr,
                           ctx->d_pair_col, ctx->d_node_gv, ctx->d_node_side, ctx->d_gptr, ctx->d_ac, at, ax);
    // The Schur diagonal depends on the fields only.  knp_assemble_rhs of the same step has already written it; while a
    // side-stream preconditioner application (knp_gmres_prepare) is in flight it READS d_cc, so it must not be rewritten here
    // (nor by the asynchronous form, which runs next to the right-hand side assembly that writes it).
    if (with_schur_diag && !ctx->prep.left()) launch_schur_diag(ctx, f);
    HIPCHK(hipGetLastError());
    ctx->have_A = true;
    if (ctx->pc_kind == KNP_PC_VBJACOBI) {
        hipLaunchKernelGGL(k_vbj_extract, dim3(nblocks(g.n_nodes_owned)), dim3(NT), 0, ctx->stream, g.n_nodes_owned,
                           ctx->d_pair_ptr, ctx->d_pair_col, ctx->d_ac, at, ax, ctx->d_node_gv, ctx->d_node_side,
                           ctx->d_gdiag, ctx->d_vbj);
        HIPCHK(hipGetLastError());
    }
    return KNP_OK;
}

// ---- matrix assembly ahead of the caller (KNP_ASM_AHEAD) ----
// The form that may run ahead, and be adopted: the time-dependent entries only, no Dirichlet rows, one GPU without hooks or
// peer-to-peer plans, an AMG preconditioner (vertex-block Jacobi consumes A at assembly time), no kernel-class timing beyond the SpMV's.
// (Deflation is not asked about: it changes the solve, not what the assembly reads or writes.)
static bool ahead_form_ok(const knp_ctx* ctx) {
    return ctx->asm_ahead && ctx->have_A && !ctx->asm_full && ctx->asm_dt == ctx->dt && ctx->n_bc == 0 && exchange_free(ctx) &&
           (ctx->pc_kind == KNP_PC_AMG || ctx->pc_kind == KNP_PC_AMG_BT || ctx->pc_kind == KNP_PC_AMG_LT) && !class_timing(ctx);
}
static bool asm_async_off() {   // KNP_ASM_ASYNC=0: no assembly on a stream of its own, asked for or ahead
    static const bool off = getenv("KNP_ASM_ASYNC") && atoi(getenv("KNP_ASM_ASYNC")) == 0;
    return off;
}
static int ensure_asm_stream(knp_ctx* ctx) {
    if (!ctx->stream_asm) {
        HIPCHK(hipStreamCreateWithFlags(&ctx->stream_asm, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&ctx->ev_fork_asm, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ctx->ev_asm, hipEventDisableTiming));
    }
    return KNP_OK;
}
// `dropped`: what a transition of ctx->step returned.  A speculative assembly whose inputs are about to change, or that nobody can
// use, has been counted and the context disarmed there; it is joined here (its kernels read the fields and d_knod and use the facet
// matrices as scratch)
static int drop_ahead(knp_ctx* ctx, bool dropped) { return dropped ? join_asm(ctx) : KNP_OK; }
// At the top of an assembly from `fields`: what ctx->step decides (knp_step_state.hpp).  ADOPT: the speculative result is the assembly
// asked for.  SKIP_COPY: d_knod is the tail's.  Otherwise a pending speculation has been dropped and the assembly runs as ever.
static KnpAsmBegin begin_assembly(knp_ctx* ctx, const knp_fields* fields, bool matrix) {
    KnpAsmInputs in;
    in.nodal_copy = ctx->asm_dmax > 0;
    in.have_target = ctx->have_tail_target;
    in.class_timing = class_timing(ctx);
    in.form_ok = ahead_form_ok(ctx);
    in.dt = ctx->dt;
    in.target = KnpStepFields::of(ctx->tail_target);
    return ctx->step.begin_assembly(matrix, KnpStepFields::of(*fields), in);
}
// Called by knp_gmres_solve right behind k_lincomb_unpack, which has left the fields of the registered target and d_knod as the next
// matrix assembly reads them: that assembly goes to the assembly stream now, into the alternate buffers (A of this step stays where
// every reader finds it).  Nothing here waits; the first call allocates the alternate buffers.
static int speculate_asm(knp_ctx* ctx) {
    if (!ctx->step.may_speculate() || !ahead_form_ok(ctx) || !ctx->have_tail_target || ctx->asm_pending || ctx->prep.left() || ctx->asm_alt_failed ||
        asm_async_off())
        return KNP_OK;
    // Two copies of the solution-dependent entries alternate from step to step.  Where the SpMV's streams (52 B per node pair) and
    // the second copy (32 B per pair, 64 B per membrane vertex pair) do not fit the 256 MiB Infinity Cache together, the assembly
    // into the other copy can evict what the next solve reads, and the host hole it fills is a fixed ~10 us: 512^2 (155 MB) gains,
    // cube 64^3 (344 MB) showed no gain -- 7 of 8 alternated pairs 2-20 us slower in three jobs, level in a fourth (DESIGN section
    // 3) -- so such contexts keep assembling when asked, and allocate no second buffer.  KNP_ASM_AHEAD=2 lifts the bound.
    if (ctx->asm_ahead < 2 && 84.0 * (double)ctx->n_pairs + 128.0 * (double)ctx->n_gp > 256.0 * 1048576.0) return KNP_OK;
    KCHK(ensure_asm_stream(ctx));
    if (!ctx->d_at_alt) {
        const size_t nat = (size_t)std::max<int64_t>(4 * ctx->n_pairs, 2) * sizeof(double), nax = (size_t)std::max<int64_t>(8 * ctx->n_gp, 2) * sizeof(double);
        if (hipMalloc((void**)&ctx->d_at_alt, nat) != hipSuccess || hipMalloc((void**)&ctx->d_ax_alt, nax) != hipSuccess) {
            (void)hipGetLastError();   // no room for a second buffer: this context assembles when asked, as before
            dev_free(ctx->d_at_alt); dev_free(ctx->d_ax_alt);
            ctx->asm_alt_failed = true;
            return KNP_OK;
        }
        // NaN (all bits set) wherever the assembly does not write
        HIPCHK(hipMemsetAsync(ctx->d_at_alt, 0xff, nat, ctx->stream_asm));
        HIPCHK(hipMemsetAsync(ctx->d_ax_alt, 0xff, nax, ctx->stream_asm));
    }
    knp_fields f = {};
    for (int j = 0; j < 3; ++j) { f.k_i[j] = ctx->tail_target.k_i[j]; f.k_e[j] = ctx->tail_target.k_e[j]; }
    f.phi_m = ctx->tail_target.phi_m;
    HIPCHK(hipEventRecord(ctx->ev_fork_asm, ctx->stream));
    HIPCHK(hipStreamWaitEvent(ctx->stream_asm, ctx->ev_fork_asm, 0));
    {
        StreamScope on_asm(ctx, ctx->stream_asm);
        KCHK(assemble_matrix_on_stream(ctx, &f, false, ctx->d_at_alt, ctx->d_ax_alt, true));
    }
    HIPCHK(hipEventRecord(ctx->ev_asm, ctx->stream_asm));
    ctx->asm_pending = true;
    ctx->step.speculated(KnpStepFields::of(f), ctx->dt);
    return KNP_OK;
}
// begin_assembly said ADOPT: the speculative result is taken by swapping the buffers; nothing is launched and asm_pending stays as it
// is (the next reader of A joins)
static void adopt_ahead(knp_ctx* ctx) {
    std::swap(ctx->d_at, ctx->d_at_alt);
    std::swap(ctx->d_ax, ctx->d_ax_alt);
}

int knp_assemble_matrix(knp_ctx* ctx, const knp_fields* fields) {
    CHECK_CTX(ctx);
    KCHK(check_fields(ctx, fields, false));
    const KnpAsmBegin b = begin_assembly(ctx, fields, true);
    KCHK(join_asm(ctx));   // whatever is on the assembly stream: the adopted speculation or a dropped one (b.dropped) among it
    if (b.what == KnpAsmDecision::ADOPT) {   // the in-line form also refreshes the Schur diagonal (see assemble_matrix_on_stream)
        adopt_ahead(ctx);
        if (!ctx->prep.left()) launch_schur_diag(ctx, make_fields(fields));
        HIPCHK(hipGetLastError());
        return KNP_OK;
    }
    return assemble_matrix_on_stream(ctx, fields, true, ctx->d_at, ctx->d_ax, b.what == KnpAsmDecision::SKIP_COPY);
}

// The same assembly on the library's own stream: it depends on the previous solution only, not on the gating update or the
// right-hand side of the step, so the caller may enqueue the right-hand side chain (and knp_gmres_prepare) on the main stream
// while it runs.  Every later call that needs A joins it (join_asm).  Falls back to the in-line form where the matrix is consumed
// at once (vertex-block Jacobi extracts its blocks) or every kernel class is being timed.
int knp_assemble_matrix_async(knp_ctx* ctx, const knp_fields* fields) {
    CHECK_CTX(ctx);
    KCHK(check_fields(ctx, fields, false));
    const KnpAsmBegin b = begin_assembly(ctx, fields, true);
    if (b.what == KnpAsmDecision::ADOPT) {   // already on the assembly stream, since the end of the last solve
        adopt_ahead(ctx);
        return KNP_OK;
    }
    KCHK(join_asm(ctx));   // (a dropped speculation, b.dropped, included)
    const bool knod_ready = b.what == KnpAsmDecision::SKIP_COPY;
    if (asm_async_off() || ctx->pc_kind == KNP_PC_VBJACOBI || class_timing(ctx) || !ctx->have_A || ctx->prep.left())
        return assemble_matrix_on_stream(ctx, fields, true, ctx->d_at, ctx->d_ax, knod_ready);
    KCHK(ensure_asm_stream(ctx));
    HIPCHK(hipEventRecord(ctx->ev_fork_asm, ctx->stream));            // after everything that wrote the fields (unpack)
    HIPCHK(hipStreamWaitEvent(ctx->stream_asm, ctx->ev_fork_asm, 0));
    {
        StreamScope on_asm(ctx, ctx->stream_asm);
        KCHK(assemble_matrix_on_stream(ctx, fields, false, ctx->d_at, ctx->d_ax, knod_ready));
    }
    HIPCHK(hipEventRecord(ctx->ev_asm, ctx->stream_asm));
    ctx->asm_pending = true;
    return KNP_OK;
}

int knp_assemble_precond(knp_ctx* ctx, const knp_fields* fields) {
    CHECK_CTX(ctx);
    side_discard(ctx);
    KCHK(drop_ahead(ctx, ctx->step.inputs_changing()));   // d_knod is rewritten below
    KCHK(join_asm(ctx));
    KCHK(check_fields(ctx, fields, false));
    const KnpHostGraph& g = ctx->g;
    const DevParams P = make_params(ctx);
    FieldPtrs f = make_fields(fields);
    ProfScope ps(ctx, 3);
    (void)begin_assembly(ctx, fields, false);   // always RUN: the promise and what the tail left in d_knod end here
    launch_cell_means(ctx, f);
    launch_assemble_nodes<true, false>(ctx, P, ctx->d_p_vals, nullptr);
    if (g.n_g > 0 && ctx->n_gp)
        hipLaunchKernelGGL((k_gamma_pairs<true>), dim3(nblocks(ctx->n_gp)), dim3(NT), 0, ctx->stream, ctx->n_gp, g.n_g, g.dim, P,
                           ctx->d_grow, ctx->d_gptr, ctx->d_gv_node_i, ctx->d_gv_node_e, ctx->d_gq_i, ctx->d_gq_e,
                           ctx->d_gcptr, ctx->d_gc_facet, ctx->d_gc_lab, ctx->d_fmeas, ctx->d_fmat, ctx->d_pair_ptr,
                           ctx->d_p_vals, nullptr, ctx->pc_coupled_phi ? ctx->d_px : nullptr);
    if (ctx->n_bc > 0)
        hipLaunchKernelGGL(k_dirichlet_rows_P, dim3(nblocks(ctx->n_bc)), dim3(NT), 0, ctx->stream, ctx->n_bc, ctx->d_bc_dofs, ctx->d_pair_ptr,
                           ctx->d_pair_col, ctx->d_p_vals);
    HIPCHK(hipGetLastError());
    ctx->have_P = true;
    return KNP_OK;
}

int knp_assemble_rhs(knp_ctx* ctx, const knp_fields* fields, double* b) {
    CHECK_CTX(ctx);
    side_discard(ctx);
    KCHK(check_fields(ctx, fields, true));
    if (!b) { ctx->err = "null b"; return KNP_E_ARG; }
    const KnpHostGraph& g = ctx->g;
    const DevParams P = make_params(ctx);
    FieldPtrs f = make_fields(fields);
    int n_aux = 0;
    for (int k = 0; k < KNP_MAX_AUX; ++k)
        if (fields->aux[k]) n_aux = k + 1;
    for (int k = 0; k < n_aux; ++k)
        if (!fields->aux[k]) { ctx->err = "aux fields must be contiguous from index 0"; return KNP_E_ARG; }
    if (g.n_g > 0) {
        KCHK(sync_program_table(ctx));
        // every facet's program must exist
        if ((int)ctx->progs.size() <= ctx->max_prog) { ctx->err = "a membrane facet refers to a program that was not set (knp_set_program)"; return KNP_E_STATE; }
        for (int i = 0; i <= ctx->max_prog; ++i)
            if (!ctx->progs[i].d_code) { ctx->err = "membrane program " + std::to_string(i) + " not set"; return KNP_E_STATE; }
    }
    ProfScope ps(ctx, 3);
    if (g.n_g > 0) {
        // dynamic LDS: register file [n_regs][NT] | constants | code of the block's program
        const int n_regs = std::max(ctx->prog_regs, 1), ccap = (std::max(ctx->prog_consts_cap, 1) + 1) & ~1;   // even: code stays 16-B aligned
#define GF_LAUNCH(D, L, Q, B, O, M)                                                                                            \
    do {                                                                                                                      \
        const size_t lds = ((size_t)n_regs * Q * B + ccap) * sizeof(double) + (size_t)4 * std::max(ctx->prog_len_cap, 1) * sizeof(int32_t); \
        if (lds > 160 * 1024) { ctx->err = "membrane programs need more LDS than a CU has"; return KNP_E_STATE; }             \
        if (lds != ctx->gamma_lds_set || M != ctx->gamma_lds_funcs)                                                           \
            HIPCHK(hipFuncSetAttribute((const void*)k_gamma_facets<D, false, true, L, Q, B, O, M>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        ctx->gamma_lds_set = lds;                                                                                             \
        ctx->gamma_lds_funcs = M;                                                                                             \
        hipLaunchKernelGGL((k_gamma_facets<D, false, true, L, Q, B, O, M>), dim3((unsigned)(((int64_t)g.n_g * L + B - 1) / B)), dim3(B), lds, \
                           ctx->stream, g.n_g, g.n_q, P, ctx->d_fv, ctx->d_fmeas, ctx->d_qp, ctx->d_qw, f, n_aux, ctx->d_coords,  \
                           ctx->d_gamma_prog, (const int32_t* const*)ctx->d_prog_code, (const int32_t*)ctx->d_prog_len,         \
                           (const double* const*)ctx->d_prog_consts, (const int32_t*)ctx->d_prog_nconsts, n_regs, ccap,        \
                           ctx->d_fmat, ctx->d_fvec);                                                                          \
    } while (0)
        // measured on MI355X (cube64: 12 288 facets x 36 points; square512: 1 024 facets x 6 points): 3 points per lane and 16
        // lanes per facet in 3D (258 -> 170 us vs one point per lane), one point per lane in 2D
        void* jit = ctx->jit_fn[g.dim == 2 ? 0 : 1];
        const bool many = gamma_many(g) && ctx->jit_fn[2];
        if (many) jit = ctx->jit_fn[2];
        if (jit) {   // run-time compiled programs (knp_jit.cpp): same kernel source, native mechanism code, no LDS register file
            int n_g = g.n_g, n_q = g.n_q, n_aux_ = n_aux, nr = 0, cc0 = 0;
            DevParams Pp = P;
            FieldPtrs ff = f;
            const int32_t* fv = ctx->d_fv; const double* fmeas = ctx->d_fmeas; const double* qp = ctx->d_qp; const double* qw = ctx->d_qw;
            const double* coords = ctx->d_coords; const int32_t* gp = ctx->d_gamma_prog;
            const int32_t* const* pc = (const int32_t* const*)ctx->d_prog_code; const int32_t* pl = ctx->d_prog_len;
            const double* const* pk = (const double* const*)ctx->d_prog_consts; const int32_t* pn = ctx->d_prog_nconsts;
            double* fmat = ctx->d_fmat; double* fvec = ctx->d_fvec;
            void* args[] = {&n_g, &n_q, &Pp, &fv, &fmeas, &qp, &qw, &ff, &n_aux_, &coords, &gp, &pc, &pl, &pk, &pn, &nr, &cc0, &fmat, &fvec};
            const int L = g.dim == 2 ? 8 : many ? 4 : 16;
            HIPCHK(hipModuleLaunchKernel((hipFunction_t)jit, (unsigned)(((int64_t)g.n_g * L + 63) / 64), 1, 1, 64, 1, 1, 0, ctx->stream, args, nullptr));
        } else if (g.dim == 2) {
            if (ctx->prog_funcs) GF_LAUNCH(2, 8, 1, 64, 2, true);
            else GF_LAUNCH(2, 8, 1, 64, 2, false);
        } else if (ctx->prog_funcs) GF_LAUNCH(3, 16, 3, 64, 2, true);
        else GF_LAUNCH(3, 16, 3, 64, 2, false);
#undef GF_LAUNCH
    }
    FieldPtrs src;
    for (int j = 0; j < 3; ++j) { src.ki[j] = ctx->src_i[j]; src.ke[j] = ctx->src_e[j]; }
    src.phim = nullptr;
    for (int k = 0; k < KNP_MAX_AUX; ++k) src.aux[k] = nullptr;
    if (g.n_nodes_owned > 0) {
        with_lanes<4, 32>(ctx->pc_group, [&](auto G) {
            hipLaunchKernelGGL((k_rhs<G()>), dim3(nblocks((int64_t)g.n_nodes_owned * G())), dim3(NT), 0, ctx->stream, g.n_nodes_owned, g.n_g, g.dim, ctx->dt,
                               ctx->d_node_vertex, ctx->d_node_side, ctx->d_pair_ptr, ctx->d_pair_col, ctx->d_pair_M, f, src,
                               ctx->have_sources ? 1 : 0, ctx->d_node_gv, ctx->d_gdiag, ctx->d_gcptr, ctx->d_gc_facet, ctx->d_gc_lab, ctx->d_fvec, b);
        });
    }
    launch_schur_diag(ctx, f);   // before a possible knp_gmres_prepare forks the side stream (it reads d_cc)
    HIPCHK(hipGetLastError());
    return KNP_OK;
}
