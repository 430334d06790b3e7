// Krylov host layer, included by knp_kernels.hip (same translation unit; the kernels it launches -- GmLayout, k_givens, k_reduce_fin,
// k_multi_dot, ... -- stay there, next to the AMG legs that share them).
//   * the side stream that computes the norm of the next solve's right-hand side (knp_gmres_prepare / knp_fgmres_prepare);
//   * the Arnoldi core both drivers share: argument checks and workspace (krylov_begin), the one-reduction Gram-Schmidt step with its
//     Givens rotation, read-back and cancellation fallback (arnoldi_step_finish), the stop tests, x += basis * y, the epilogue;
//   * knp_gmres_solve: left preconditioning, ||B r||;  knp_fgmres_solve: right preconditioning with a second basis Z, ||r||.

// slot layout of d_red: 0 .. restart+1 = the Gram-Schmidt coefficients, the gauge coefficient and w.w of one iteration (nred = j + 2 + ns
// <= restart + 2 values), GM_EXPL = 57 the explicit norm of the cancellation fallback, 58..63 norms / flags, 64.. deflation, 100.. the mirror
// of the residual estimate and flag of the last Givens step, 120.. the side stream (SIDE_SLOT), FB_SLOT ||b||^2 of the flexible solve
static constexpr int GM_RES = 100, GM_EXPL = 57, GM_MAX_RESTART = GM_EXPL - 2;
static constexpr int FB_SLOT = 124;   // (knp_fgmres_prepare on the side stream, or in line)
static_assert(GM_RES + 2 <= RED_SLOTS && DEFL_SLOT0 + DEFL_MAX <= GM_RES, "reduction slot layout");
static constexpr double GM_DTOL = 1e5;   // divergence: residual above GM_DTOL times the reference of the driver

// ---- ||B b|| of the next solve on a side stream ------------------------------------------------------------------------
// The first preconditioner application of a solve only needs the right-hand side, not the matrix: started right after the
// right-hand side is assembled it overlaps the matrix assembly of the same timestep (separate HIP streams; the V-cycle's
// coarse levels are launch-latency bound, the assembly is bandwidth bound).
static void side_discard(knp_ctx* ctx) {   // any call that could touch what the side stream uses joins it first
    switch (ctx->prep.kind) {
        case KnpSidePrep::NONE:
        case KnpSidePrep::LEFT_DEFERRED: break;   // deferred: nothing was enqueued yet
        default: (void)hipEventSynchronize(ctx->ev_join);
    }
    ctx->prep.kind = KnpSidePrep::NONE;
}
static int ensure_side_stream(knp_ctx* ctx) {
    if (ctx->stream2) return KNP_OK;
    HIPCHK(hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    return KNP_OK;
}

static bool exchanges_all_native(const knp_ctx* ctx) {
    if (!ctx->p2p || ctx->p2p_fine < 0 || ctx->p2p_red < 0 || ctx->defl_m > 0) return false;
    const int nh = ctx->pc_kind == KNP_PC_AMG ? 1 : (ctx->pc_kind == KNP_PC_AMG_BT || ctx->pc_kind == KNP_PC_AMG_LT) ? 2 : 0;
    for (int h = 0; h < nh; ++h)
        for (int l = 0; l < ctx->hier[h].levels; ++l) {
            const KnpAmgLevel& L = ctx->hier[h].lv[l];
            if (L.dist && L.p2p_halo < 0) return false;
            if (L.repl_n > 0 && L.p2p_repl < 0) return false;
        }
    return true;
}

// contexts without an exchange between the partial sums and their use: the reduction finishes in one single-block kernel
static bool fin_ok(const knp_ctx* ctx) {
    static const bool off = getenv("KNP_FIN") && atoi(getenv("KNP_FIN")) == 0;
    return !off && !ctx->allreduce && ctx->p2p_red < 0;
}
static bool fused_norm_possible(const knp_ctx* ctx, int64_t cnt) {
    static const bool off = getenv("KNP_NO_FUSED_NORM") != nullptr;
    return ctx->ns_on && cnt > 0 && !off && ctx->defl_m == 0;
}
// z = B r and the squared norm of its gauge-projected part with ONE reduction: {sum of the potential entries, z.z} are reduced
// together and |z - ns (ns.z)|^2 = z.z - s^2/cnt (k_proj_norm; slot 60 = the norm, 61 = its cancellation flag, 62 = s).  z itself is
// left UNPROJECTED (*fused = true): the caller subtracts the mean when it normalises (k_scale_rsqrt_proj) or does not need z at
// all (||B b||).  Without a null space: the plain sequence, *fused = false.
// side = true: the side-stream form of knp_gmres_prepare's concurrent mode -- partial sums in d_partial_s, reduced values in slots
// 122/123 -> {norm, flag} in 120/121 (+ pinned mirror), and NO sequence word (the solve joins it with an event): nothing the main
// stream uses is touched.  Requires fused_norm_possible.
static int pc_apply_norm(knp_ctx* ctx, const double* r, double* z, int64_t cnt, bool* fused, bool side = false) {
    if (side) {
        *fused = true;
        DotReq dq{0, true, (int64_t)ctx->n_dof_local, ctx->d_V, ctx->d_partial_s};
        KCHK(pc_apply_proj(ctx, r, z, 0, (ctx->fused_dots && fin_ok(ctx)) ? &dq : nullptr));   // (as the in-line form below)
        ProfScope ps(ctx, 1);
        const int nb = dq.done ? dq.nb : ctx->n_red_blocks;
        if (!dq.done)
            hipLaunchKernelGGL((k_multi_dot<8, true, true>), dim3(nb), dim3(NT), 0, ctx->stream, ctx->n_dof_owned, (int64_t)ctx->n_dof_local, 0, 0,
                               ctx->d_V, z, ctx->d_partial_s);
        ++ctx->n_allreduce;
        hipLaunchKernelGGL(k_reduce_fin, dim3(1), dim3(NT), 0, ctx->stream, 2, nb, 2, ctx->d_partial_s, ctx->d_red, SIDE_SLOT + 2, GmLayout{1}, 0, 0,
                           1.0 / (double)cnt, (double*)nullptr, SIDE_SLOT, GM_CANCEL, ctx->mirror(), (volatile int64_t*)nullptr, (int64_t)0,
                           dq.done ? RED_WIDE : RED_BLOCKS);
        HIPCHK(hipGetLastError());
        return KNP_OK;
    }
    if (!fused_norm_possible(ctx, cnt)) {
        *fused = false;
        KCHK(pc_apply_proj(ctx, r, z, cnt));
        return dot_to_slot(ctx, z, z, 60);
    }
    *fused = true;
    DotReq dq{0, true, (int64_t)ctx->n_dof_local, ctx->d_V, ctx->d_partial};
    KCHK(pc_apply_proj(ctx, r, z, 0, (ctx->fused_dots && fin_ok(ctx)) ? &dq : nullptr));   // (k_reduce_partials takes no stride)
    ProfScope ps(ctx, 1);
    const int nb = dq.done ? dq.nb : ctx->n_red_blocks;
    if (!dq.done)
        hipLaunchKernelGGL((k_multi_dot<8, true, true>), dim3(nb), dim3(NT), 0, ctx->stream, ctx->n_dof_owned, (int64_t)ctx->n_dof_local, 0, 0,
                           ctx->d_V, z, ctx->d_partial);
    if (fin_ok(ctx)) {
        ++ctx->n_allreduce;
        hipLaunchKernelGGL(k_reduce_fin, dim3(1), dim3(NT), 0, ctx->stream, 2, nb, 2, ctx->d_partial, ctx->d_red, 62, GmLayout{1}, 0, 0, 1.0 / (double)cnt,
                           (double*)nullptr, 60, GM_CANCEL, ctx->mirror(), ctx->mirror() ? ctx->h_seq_dev : nullptr, ++ctx->seq_counter,
                           dq.done ? RED_WIDE : RED_BLOCKS);
        HIPCHK(hipGetLastError());
        return KNP_OK;
    }
    hipLaunchKernelGGL(k_reduce_partials, dim3(2), dim3(NT), 0, ctx->stream, nb, ctx->d_partial, ctx->d_red, 62, (double*)nullptr);
    KCHK(allreduce_slots(ctx, 62, 2));
    hipLaunchKernelGGL(k_proj_norm, dim3(1), dim3(64), 0, ctx->stream, ctx->d_red, 62, 60, 1.0 / (double)cnt, GM_CANCEL, ctx->mirror(),
                       ctx->mirror() ? ctx->h_seq_dev : nullptr, ++ctx->seq_counter);
    HIPCHK(hipGetLastError());
    return KNP_OK;
}
// the host side of it: read {norm^2, flag}; on cancellation project z explicitly and reduce again (*fused becomes false)
static int pc_norm_read(knp_ctx* ctx, double* z, int64_t cnt, bool* fused) {
    KCHK(read_slots(ctx, 60, *fused ? 2 : 1, ctx->seq_counter));
    if (*fused && ctx->h_red[61] != 0.0) {
        ++ctx->n_norm_fallback;
        const int no = ctx->g.n_nodes_owned;
        hipLaunchKernelGGL(k_phi_sub, dim3(nblocks(no)), dim3(NT), 0, ctx->stream, no, ctx->d_red + 62, 1.0 / (double)cnt, z);
        *fused = false;
        KCHK(dot_to_slot(ctx, z, z, 60));
        KCHK(read_slots(ctx, 60, 1, ctx->seq_counter));
    }
    return KNP_OK;
}

// second set of work vectors for the cycle that runs on the side stream while the main stream applies the same hierarchies
static int ensure_side_ws(knp_ctx* ctx) {
    if (ctx->side_ws) return KNP_OK;
    auto zalloc = [&](double** p, size_t n) -> int {
        HIPCHK(hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(double)));
        HIPCHK(hipMemsetAsync(*p, 0, std::max<size_t>(n, 1) * sizeof(double), ctx->stream));
        return KNP_OK;
    };
    for (int h = 0; h < KNP_MAX_HIER; ++h)
        for (int l = 0; l < ctx->hier[h].levels; ++l) {
            KnpAmgLevel& L = ctx->hier[h].lv[l];
            const size_t n = (size_t)std::max(L.n_loc, L.n);
            if (n == 0) continue;
            if (!L.xs) { KCHK(zalloc(&L.xs, n)); KCHK(zalloc(&L.bs, n)); KCHK(zalloc(&L.rs, n)); KCHK(zalloc(&L.ds, n)); KCHK(zalloc(&L.r2s, n)); }
            if (L.cat && !L.cats) KCHK(zalloc(&L.cats, (size_t)L.n + (size_t)L.n_coarse));
        }
    const size_t nl = (size_t)std::max(ctx->n_dof_local, 1);
    if (!ctx->d_t2_s) { KCHK(zalloc(&ctx->d_t2_s, nl)); KCHK(zalloc(&ctx->d_w2_s, nl)); }
    if (!ctx->d_wb) KCHK(zalloc(&ctx->d_wb, nl));
    if (!ctx->d_partial_s) KCHK(zalloc(&ctx->d_partial_s, (size_t)RED_SLOTS * RED_BLOCKS));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->side_ws = true;
    return KNP_OK;
}
static void swap_side_ws(knp_ctx* ctx) {   // host-side pointer swap: kernel arguments are taken at launch
    for (int h = 0; h < KNP_MAX_HIER; ++h)
        for (int l = 0; l < ctx->hier[h].levels; ++l) {
            KnpAmgLevel& L = ctx->hier[h].lv[l];
            if (!L.xs) continue;
            std::swap(L.x, L.xs); std::swap(L.b, L.bs); std::swap(L.r, L.rs); std::swap(L.d, L.ds); std::swap(L.r2, L.r2s);
            if (L.cat && L.cats) std::swap(L.cat, L.cats);
        }
    if (ctx->d_t2 && ctx->d_t2_s) { std::swap(ctx->d_t2, ctx->d_t2_s); std::swap(ctx->d_w2, ctx->d_w2_s); }
}
// the side-stream cycle may run next to the solve's own first preconditioner application: one GPU, fused cycles (their work
// vectors are exactly the per-level sets swapped above), gauge-projected norm from one reduction, pinned mirror for the result
static bool side_concurrent_ok(const knp_ctx* ctx, int64_t cnt) {
    static const bool off = getenv("KNP_SIDE_CONCURRENT") && atoi(getenv("KNP_SIDE_CONCURRENT")) == 0;
    // (deflation: fused_norm_possible asks below; class timing: knp_gmres_prepare, the only caller, has returned on it before it asks here)
    if (off || !exchange_free(ctx) || ctx->n_bc > 0 || !ctx->h_red_dev) return false;
    if (!fused_norm_possible(ctx, cnt)) return false;
    if (ctx->pc_kind == KNP_PC_AMG) return ctx->hier[0].fused != 0;
    if (ctx->pc_kind == KNP_PC_AMG_BT || ctx->pc_kind == KNP_PC_AMG_LT) return ctx->hier[0].fused && ctx->hier[1].fused;
    return false;
}

int knp_gmres_prepare(knp_ctx* ctx, const double* b) {
    CHECK_CTX(ctx);
    if (!b) return KNP_E_ARG;
    side_discard(ctx);
    // single-GPU contexts only (the exchanges of a distributed preconditioner are ordered on the main stream), and only
    // once the Krylov workspace exists (second solve onwards)
    const bool off = getenv("KNP_NO_PREPARE") != nullptr;
    // vertex-block Jacobi takes its blocks from the matrix that knp_assemble_matrix is about to rewrite: nothing to overlap
    if (ctx->pc_kind == KNP_PC_VBJACOBI) return KNP_OK;
    // Distributed contexts: legal when EVERY exchange of the preconditioner runs in the library (native peer-to-peer plans):
    // those kernels are launched on ctx->stream, i.e. on the side stream here, in the same order on every rank, and the main
    // stream does no exchange until the solve joins.  With torch.distributed hooks (ordered on torch's stream) it stays a no-op.
    if (off || ctx->gm_restart <= 0 || class_timing(ctx)) return KNP_OK;
    if (!exchange_free(ctx) && !exchanges_all_native(ctx)) return KNP_OK;
    KCHK(ensure_side_stream(ctx));
    int rc = KNP_OK;
    const int64_t cnt = ctx->ns_on ? global_phi_count(ctx, &rc) : 0;
    KCHK(rc);
    const bool conc = side_concurrent_ok(ctx, cnt);
    HIPCHK(hipEventRecord(ctx->ev_fork, ctx->stream));
    if (conc) {
        // Concurrent form: only the fork point is fixed here (b is final).  The cycle itself is enqueued by knp_gmres_solve BEHIND the
        // launches of its own first residual chain, so that the host feeds the critical path first and this cycle overlaps it.
        KCHK(ensure_side_ws(ctx));
        ctx->prep = {KnpSidePrep::LEFT_DEFERRED, b, true};
        return KNP_OK;
    }
    HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
    bool fused_norm = false;
    {
        StreamScope on_side(ctx, ctx->stream2);
        KCHK(pc_apply_norm(ctx, b, ctx->d_w, cnt, &fused_norm));
    }
    HIPCHK(hipEventRecord(ctx->ev_join, ctx->stream2));
    ctx->prep = {KnpSidePrep::LEFT_ENQUEUED, b, fused_norm};
    return KNP_OK;
}

// second basis Z of the flexible driver
static int ensure_z(knp_ctx* ctx, int restart) {
    if (ctx->d_Z && ctx->z_cap >= restart) return KNP_OK;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    dev_free(ctx->d_Z);
    const size_t bytes = (size_t)restart * std::max(ctx->n_dof_local, 1) * sizeof(double);
    HIPCHK(hipMalloc((void**)&ctx->d_Z, bytes));
    HIPCHK(hipMemset(ctx->d_Z, 0, bytes));
    ctx->z_cap = restart;
    return KNP_OK;
}

int knp_fgmres_prepare(knp_ctx* ctx, const double* b) {
    CHECK_CTX(ctx);
    if (!b) return KNP_E_ARG;
    side_discard(ctx);
    // one GPU only: on distributed contexts ||b|| needs an all-reduce, which the solve does in line
    if (getenv("KNP_NO_PREPARE") || class_timing(ctx) || !exchange_free(ctx)) return KNP_OK;
    KCHK(ensure_side_stream(ctx));
    if (!ctx->d_partial_s) {
        HIPCHK(hipMalloc((void**)&ctx->d_partial_s, (size_t)RED_SLOTS * RED_BLOCKS * sizeof(double)));
        HIPCHK(hipMemset(ctx->d_partial_s, 0, (size_t)RED_SLOTS * RED_BLOCKS * sizeof(double)));
    }
    const int nb = ctx->n_red_blocks;
    HIPCHK(hipEventRecord(ctx->ev_fork, ctx->stream));
    HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
    hipLaunchKernelGGL(k_dot, dim3(nb), dim3(NT), 0, ctx->stream2, ctx->n_dof_owned, b, b, ctx->d_partial_s);
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(NT), 0, ctx->stream2, nb, ctx->d_partial_s, ctx->d_red, FB_SLOT, ctx->mirror(),
                       (volatile int64_t*)nullptr, (int64_t)0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ctx->ev_join, ctx->stream2));
    ctx->prep = {KnpSidePrep::FLEX, b, false};
    return KNP_OK;
}

// ---- the Arnoldi core of both drivers -----------------------------------------------------------------------------------
// What one solve keeps fixed, on the driver's stack.  `ns`/`inv_cnt`: the (unnormalised) null-space vector takes part in the
// Gram-Schmidt pass as one more "basis vector" (left GMRES with a null space); the flexible driver leaves them off.
struct KrylovSolve {
    knp_ctx* ctx;
    GmLayout GL;
    double* gm;
    int n;             // owned rows
    int64_t ldv;       // leading dimension of the bases
    int nb, vec_blocks;
    bool ns;
    double inv_cnt;
    double ttol, atol, dref;   // stop: res <= max(rtol * reference norm, atol); divergence: res > GM_DTOL * dref
};

// argument and state checks, the workspace (V, Z for the flexible driver, gm) and the global number of potential unknowns
static int krylov_begin(knp_ctx* ctx, const double* b, double* x, int32_t max_it, int32_t restart, int32_t* its, double* rnorm, int32_t* reason,
                        bool flexible, KrylovSolve* K, int64_t* cnt) {
    if (!b || !x || !its || !rnorm || !reason) return KNP_E_ARG;
    if (!ctx->have_A) { ctx->err = "matrix not assembled"; return KNP_E_STATE; }
    if (restart < 1 || restart > GM_MAX_RESTART || max_it < 0) {
        ctx->err = "restart must be in [1," + std::to_string(GM_MAX_RESTART) + "] and max_it >= 0";
        return KNP_E_ARG;
    }
    KCHK(drop_ahead(ctx, ctx->step.x_changing()));   // x is about to change
    KCHK(ensure_work(ctx, restart));
    if (flexible && ctx->pc_kind != KNP_PC_NONE) KCHK(ensure_z(ctx, restart));   // with no preconditioner Z is V: nothing is allocated or copied
    prof_collect_ready(ctx);
    int rc;
    *cnt = ctx->ns_on ? global_phi_count(ctx, &rc) : 0;
    if (ctx->ns_on) KCHK(rc);
    const GmLayout GL{restart};
    if (ctx->gm_cap < GL.size()) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        dev_free(ctx->d_gm);
        HIPCHK(hipMalloc((void**)&ctx->d_gm, (size_t)GL.size() * sizeof(double)));
        HIPCHK(hipMemset(ctx->d_gm, 0, (size_t)GL.size() * sizeof(double)));
        ctx->gm_cap = GL.size();
    }
    const int n = ctx->n_dof_owned;
    *K = KrylovSolve{ctx, GL, ctx->d_gm, n, (int64_t)ctx->n_dof_local, ctx->n_red_blocks, std::min(nblocks(n), 2048), false, 0.0, 0.0, 0.0, 0.0};
    return KNP_OK;
}

// residual estimate and flag of the last k_givens: pinned mirror (slots GM_RES, GM_RES+1) + sequence word, or a copy on the hook path
static int gm_read_state(const KrylovSolve& K, double* res, int* flag) {
    knp_ctx* ctx = K.ctx;
    ++ctx->n_readback;
    if (ctx->mirror() && ctx->h_seq_dev) {
        KCHK(read_slots_inner(ctx, GM_RES, 2, ctx->seq_counter));
        if (ctx->p2p) KCHK(knp_p2p_check(ctx));
        *res = ctx->h_red[GM_RES];
        *flag = (int)ctx->h_red[GM_RES + 1];
    } else {
        double tmp[3];
        HIPCHK(hipMemcpyAsync(tmp, K.gm + K.GL.st(), 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        *res = tmp[2];
        *flag = (int)tmp[1];
    }
    return KNP_OK;
}

// Iteration j, from w = (B) A (B) v_j to v_{j+1} = vn and the residual estimate: classical Gram-Schmidt of w against V_0..V_j with
// ONE reduction -- the j+1 Gram-Schmidt coefficients, the gauge coefficient (K.ns) and w.w; the norm of the orthogonalised vector
// follows by Pythagoras (explicit norm only when that would cancel, see k_givens).  The first stage of the reduction (partial sums per
// block in d_partial) is either already there -- first_nb > 0 blocks at row stride first_stride, written by the kernel that produced
// w: the preconditioner's last leg (RED_WIDE) or the SpMV (SPMV_WIDE) -- or runs here in k_multi_dot.
// Two halves: arnoldi_step_enqueue launches the reduction, the Givens step and v_{j+1} and waits for nothing;
// arnoldi_step_read waits for the residual estimate and flag (`have`: the caller has read them already, they are in *res, *flag)
// and runs the cancellation fallback.  arnoldi_step_finish is both, back to back.
// `early` > 0: the stop threshold of the solve, with which k_update_scale skips v_{j+1} on the converging iteration (nothing reads
// that vector after a converged stop: arnoldi_step_read touches vn only under the cancellation flag, which excludes the early
// return, and the update of x uses V_0..V_j); 0: the vector is always built.
static int arnoldi_step_enqueue(const KrylovSolve& K, int j, const double* w, double* vn, int first_nb, int first_stride, double early = 0.0) {
    knp_ctx* ctx = K.ctx;
    hipStream_t st = ctx->stream;
    const GmLayout GL = K.GL;
    double* gm = K.gm;
    const int n = K.n, nb = K.nb, nsi = K.ns ? 1 : 0;
    const int64_t ldv = K.ldv;
    ProfScope ps(ctx, 1);
    const bool done = first_nb > 0;
    const int nbr = done ? first_nb : nb;   // partial blocks of the first stage, and their row stride
    const int pst = done ? first_stride : RED_BLOCKS;
    for (int i0 = 0; i0 <= j && !done; i0 += 8) {   // owned rows; the first launch also takes the gauge coefficient and w.w
        if (i0 == 0 && K.ns)
            hipLaunchKernelGGL((k_multi_dot<8, true, true>), dim3(nb), dim3(NT), 0, st, n, ldv, i0, j + 1, ctx->d_V, w, ctx->d_partial);
        else if (i0 == 0)
            hipLaunchKernelGGL((k_multi_dot<8, false, true>), dim3(nb), dim3(NT), 0, st, n, ldv, i0, j + 1, ctx->d_V, w, ctx->d_partial);
        else
            hipLaunchKernelGGL((k_multi_dot<8, false, false>), dim3(nb), dim3(NT), 0, st, n, ldv, i0, j + 1, ctx->d_V, w, ctx->d_partial);
    }
    const int nred = j + 2 + nsi;
    if (fin_ok(ctx)) {   // one GPU: second reduction stage + Givens step in one single-block kernel
        ++ctx->n_allreduce;
        hipLaunchKernelGGL(k_reduce_fin, dim3(1), dim3(NT), 0, st, 1, nbr, nred, ctx->d_partial, ctx->d_red, 0, GL, j, nsi, K.inv_cnt, gm,
                           0, 0.0, ctx->mirror() ? ctx->h_red_dev + GM_RES : nullptr, ctx->mirror() ? ctx->h_seq_dev : nullptr, ++ctx->seq_counter,
                           pst);
    } else {   // (a first stage done elsewhere implies fin_ok -- k_reduce_partials takes no stride -- so nbr = nb here)
        hipLaunchKernelGGL(k_reduce_partials, dim3(nred), dim3(NT), 0, st, nbr, ctx->d_partial, ctx->d_red, 0, (double*)nullptr);
        KCHK(allreduce_slots(ctx, 0, nred));
        hipLaunchKernelGGL(k_givens, dim3(1), dim3(64), 0, st, GL, j, nsi, K.inv_cnt, ctx->d_red, -1, gm,
                           ctx->mirror() ? ctx->h_red_dev + GM_RES : nullptr, ctx->mirror() ? ctx->h_seq_dev : nullptr, ++ctx->seq_counter);
    }
    hipLaunchKernelGGL(k_update_scale, dim3(nb), dim3(NT), 0, st, n, ldv, j + 1, ctx->d_V, ctx->d_red, w, gm + GL.st(), K.inv_cnt, vn, early);
    HIPCHK(hipGetLastError());
    return KNP_OK;
}
static int arnoldi_step_read(const KrylovSolve& K, int j, double* vn, double* res, int* flag, bool have = false) {
    knp_ctx* ctx = K.ctx;
    hipStream_t st = ctx->stream;
    const GmLayout GL = K.GL;
    double* gm = K.gm;
    const int n = K.n, nb = K.nb, nsi = K.ns ? 1 : 0;
    if (!have) KCHK(gm_read_state(K, res, flag));
    if (*flag == 1) {   // cancellation: explicit norm of the (unnormalised) vector, second reduction of this iteration
        ProfScope ps(ctx, 1);
        ++ctx->n_norm_fallback;
        hipLaunchKernelGGL(k_dot, dim3(nb), dim3(NT), 0, st, n, vn, vn, ctx->d_partial);
        hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(NT), 0, st, nb, ctx->d_partial, ctx->d_red, GM_EXPL, (double*)nullptr);
        KCHK(allreduce_slots(ctx, GM_EXPL, 1));
        hipLaunchKernelGGL(k_givens, dim3(1), dim3(64), 0, st, GL, j, nsi, K.inv_cnt, ctx->d_red, GM_EXPL, gm,
                           ctx->mirror() ? ctx->h_red_dev + GM_RES : nullptr, ctx->mirror() ? ctx->h_seq_dev : nullptr, ++ctx->seq_counter);
        hipLaunchKernelGGL(k_scale_inplace_rsqrt, dim3(K.vec_blocks), dim3(NT), 0, st, n, gm + GL.st(), vn);
        HIPCHK(hipGetLastError());
        KCHK(gm_read_state(K, res, flag));
    }
    return KNP_OK;
}
static int arnoldi_step_finish(const KrylovSolve& K, int j, const double* w, double* vn, int first_nb, int first_stride, double* res, int* flag) {
    KCHK(arnoldi_step_enqueue(K, j, w, vn, first_nb, first_stride));
    return arnoldi_step_read(K, j, vn, res, flag);
}

// after iteration j: counts it, sets *jd to the number of columns the update of x may use; true = the solve ends here (*reason set)
static bool krylov_stop_test(const KrylovSolve& K, int j, int flag, double res, int max_it, int* it, int* jd, int32_t* reason) {
    if (flag != 0 || !std::isfinite(res)) { *reason = KNP_DIVERGED_NANORINF; *jd = j; return true; }
    ++*it;
    *jd = j + 1;
    if (res <= K.ttol) { *reason = (res <= K.atol) ? KNP_CONVERGED_ATOL : KNP_CONVERGED_RTOL; return true; }
    if (*it >= max_it) { *reason = KNP_DIVERGED_ITS; return true; }
    if (res > GM_DTOL * K.dref) { *reason = KNP_DIVERGED_DTOL; return true; }
    return false;
}

// x += basis(:, 0..jd-1) y, with H y = g solved in the same kernel for short cycles
static void krylov_update_plain(const KrylovSolve& K, int jd, const double* basis, double* x) {
    hipStream_t st = K.ctx->stream;
    if (jd <= 8) {
        hipLaunchKernelGGL(k_lincomb_solve, dim3(K.vec_blocks), dim3(NT), 0, st, K.GL, jd, K.gm, K.n, K.ldv, basis, x);
    } else {
        hipLaunchKernelGGL(k_gm_solve_y, dim3(1), dim3(64), 0, st, K.GL, jd, K.gm);
        hipLaunchKernelGGL(k_lincomb, dim3(K.vec_blocks), dim3(NT), 0, st, K.n, K.ldv, jd, basis, K.gm + K.GL.y(), x);
    }
}

static int krylov_end(const KrylovSolve& K, double* x, int it, double res, int32_t* its, double* rnorm) {
    knp_ctx* ctx = K.ctx;
    *its = it;
    *rnorm = res;
    KCHK(halo_update(ctx, x));
    HIPCHK(hipGetLastError());
    if (ctx->p2p) {   // the final halo is two asynchronous kernels: make its outcome (and any timeout) known before returning
        HIPCHK(hipStreamSynchronize(ctx->stream));
        KCHK(knp_p2p_check(ctx));
    }
    if (ctx->comm_rc != KNP_OK) { const int rc2 = ctx->comm_rc; ctx->comm_rc = KNP_OK; return rc2; }
    return KNP_OK;
}

// ---- GMRES(restart), left preconditioning, classical Gram-Schmidt (KSPGMRES semantics) ------
int knp_gmres_solve(knp_ctx* ctx, const double* b, double* x, double rtol, double atol, int32_t max_it, int32_t restart,
                    int32_t* its, double* rnorm, int32_t* reason) {
    CHECK_CTX(ctx);
    KrylovSolve K;
    int64_t cnt;
    KCHK(krylov_begin(ctx, b, x, max_it, restart, its, rnorm, reason, false, &K, &cnt));
    const int n = K.n, m = restart;
    const int64_t ldv = K.ldv;
    const GmLayout GL = K.GL;
    double* gm = K.gm;
    hipStream_t st = ctx->stream;

    // ||M b|| for the relative tolerance (non-zero initial guess, preconditioned norm)
    bool lazy_bnorm = false;
    const bool prepared = ctx->prep.left() && ctx->prep.b == b && restart == ctx->gm_restart;
    if (prepared && ctx->prep.kind != KnpSidePrep::LEFT_ENQUEUED) {
        // concurrent form: the side-stream cycle has its own vectors and slots; it is joined after the first read-back below
        lazy_bnorm = true;
    } else if (prepared) {   // already computed on the side stream (knp_gmres_prepare)
        HIPCHK(hipEventSynchronize(ctx->ev_join));
        ctx->prep.kind = KnpSidePrep::NONE;
        if (!ctx->h_red_dev) {
            HIPCHK(hipMemcpy(ctx->h_red + 60, ctx->d_red + 60, 2 * sizeof(double), hipMemcpyDeviceToHost));
        }
        if (ctx->prep.fused && ctx->h_red[61] != 0.0) {   // cancellation in the one-reduction norm: redo it explicitly, in line
            ++ctx->n_norm_fallback;
            KCHK(pc_apply_proj(ctx, b, ctx->d_w, cnt));
            KCHK(dot_to_slot(ctx, ctx->d_w, ctx->d_w, 60));
            KCHK(read_slots(ctx, 60, 1, ctx->seq_counter));
        }
    } else {
        side_discard(ctx);
        bool fused_norm = false;
        KCHK(pc_apply_norm(ctx, b, ctx->d_w, cnt, &fused_norm));
        KCHK(pc_norm_read(ctx, ctx->d_w, cnt, &fused_norm));
    }
    double bnorm = lazy_bnorm ? 0.0 : std::sqrt(ctx->h_red[60]);
    ctx->last_bnorm = bnorm;
    if (!lazy_bnorm && !std::isfinite(bnorm)) { *its = 0; *rnorm = bnorm; *reason = KNP_DIVERGED_NANORINF; return KNP_OK; }
    K.ttol = std::max(rtol * bnorm, atol);
    K.atol = atol;
    int it = 0;
    double res = 0.0, res0 = -1.0;
    *reason = 0;
    const bool ns = ctx->ns_on && cnt > 0;
    K.ns = ns;
    K.inv_cnt = ns ? 1.0 / (double)cnt : 0.0;
    // one cycle start in its launch pieces: v_0 = B r / beta with g = (beta, 0, ...), and iteration j up to v_{j+1} (no host wait in either)
    auto enqueue_v0 = [&](bool fused_norm) {
        if (fused_norm) {
            hipLaunchKernelGGL(k_scale_rsqrt_proj, dim3(K.vec_blocks), dim3(NT), 0, st, n, ctx->d_w, ctx->d_red + 60, ctx->d_red + 62,
                               1.0 / (double)cnt, ctx->d_V, gm + GL.g(), m);
        } else {
            hipLaunchKernelGGL(k_scale_rsqrt, dim3(K.vec_blocks), dim3(NT), 0, st, n, ctx->d_w, ctx->d_red + 60, ctx->d_V);
            hipLaunchKernelGGL(k_gm_init, dim3(1), dim3(64), 0, st, GL, gm, ctx->d_red + 60);
        }
    };
    auto enqueue_iteration = [&](int j, double early) -> int {
        double* vj = ctx->d_V + (size_t)j * ldv;
        double* vn = ctx->d_V + (size_t)(j + 1) * ldv;
        KCHK(spmv_A(ctx, vj, nullptr, ctx->d_t, false));
        // The null-space removal that follows the preconditioner (KSP_RemoveNullSpace) is folded into the
        // Gram-Schmidt pass: the basis vectors are orthogonal to ns, so h_i = V_i.(w - ns ns.w) = V_i.w, and the
        // projection itself is one more "basis vector" in the update (same reduction, no extra all-reduce).
        // The first stage of that reduction runs in the preconditioner's last leg where that can take it (DotReq), else in
        // k_multi_dot (arnoldi_step_enqueue).
        DotReq dq{j + 1, ns, ldv, ctx->d_V, ctx->d_partial};
        KCHK(pc_apply_proj(ctx, ctx->d_t, ctx->d_w, ns ? 0 : cnt, (ctx->fused_dots && fin_ok(ctx) && j + 1 <= BU_MAX_M) ? &dq : nullptr));
        return arnoldi_step_enqueue(K, j, ctx->d_w, vn, dq.done ? dq.nb : 0, RED_WIDE, early);
    };
    // Enqueue-ahead form of a cycle start: nothing on the device depends on the host's reading of ||B r||, so v_0 and iteration 0 are
    // launched behind the norm's reduction and the host waits ONCE, for iteration 0's k_reduce_fin (stream order: the norm's has
    // finished by then).  The decisions are taken afterwards, the same ones in the same order; an entry that ends or repairs the
    // cycle start discards iteration 0, which has written V_0, V_1, gm, d_t, d_w and reduction slots but not x.  One GPU, no hooks:
    // there every reduction publishes to the pinned mirror and the sequence word, through k_reduce_fin or (KNP_FIN=0) k_proj_norm / k_givens.
    const bool ahead_ok = ctx->gmres_ahead && ctx->mirror() && ctx->h_seq && ctx->h_seq_dev && exchange_free(ctx) && ctx->defl_m == 0 && ctx->n_bc == 0 &&
                          max_it > 0 && !class_timing(ctx);
    // The update after which the solve returns may also unpack x (k_lincomb_unpack): one GPU, nothing between the update and the
    // caller (krylov_end's halo is a no-op there), every unknown reached from a vertex, a registered target, no class timing.
    const bool tail_ok = ctx->fused_tail && ctx->tail_ok && ctx->have_tail_target && exchange_free(ctx) && ctx->defl_m == 0 && ctx->n_bc == 0 &&
                         !class_timing(ctx);
    while (true) {
        // r = M (b - A x)
        KCHK(spmv_A(ctx, x, b, ctx->d_t, true));
        bool fused_norm = false;   // the gauge projection of r rides on the norm's reduction and on the normalisation pass
        KCHK(pc_apply_norm(ctx, ctx->d_t, ctx->d_w, cnt, &fused_norm));
        if (lazy_bnorm && ctx->prep.kind == KnpSidePrep::LEFT_DEFERRED) {   // ||B b||: its cycle goes to the side stream now, behind the launches above
            ctx->prep.kind = KnpSidePrep::LEFT_CONCURRENT;
            HIPCHK(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
            {
                StreamScope on_side(ctx, ctx->stream2);
                bool fn = false;
                swap_side_ws(ctx);
                const int rcs = pc_apply_norm(ctx, b, ctx->d_wb, cnt, &fn, true);
                swap_side_ws(ctx);   // (back before any return)
                KCHK(rcs);
            }
            HIPCHK(hipEventRecord(ctx->ev_join, ctx->stream2));
        }
        bool ahead = ahead_ok && fused_norm;   // true while iteration 0 of this cycle is in flight (or done) and still valid
        double res_a = 0.0;
        int flag_a = 0;
        // the residual chain again, in order, after iteration 0 (or the ||B b|| repair) overwrote d_t and d_w (rare)
        auto redo_residual = [&]() -> int {
            if (ahead) KCHK(spmv_A(ctx, x, b, ctx->d_t, true));
            ahead = false;
            KCHK(pc_apply_norm(ctx, ctx->d_t, ctx->d_w, cnt, &fused_norm));
            return pc_norm_read(ctx, ctx->d_w, cnt, &fused_norm);
        };
        if (ahead) {
            enqueue_v0(true);
            // (||B b|| still on the side stream: the threshold is not known yet, v_1 is built unconditionally)
            KCHK(enqueue_iteration(0, (ctx->update_early && !lazy_bnorm) ? K.ttol : 0.0));
            KCHK(gm_read_state(K, &res_a, &flag_a));   // the one wait; slots 60, 61 of the mirror are the norm's
            if (ctx->h_red[61] != 0.0) KCHK(redo_residual());   // cancellation in the residual norm: pc_norm_read projects explicitly
        } else {
            KCHK(pc_norm_read(ctx, ctx->d_w, cnt, &fused_norm));
        }
        if (lazy_bnorm) {   // join the side stream now: its cycle ran next to the SpMV and the cycle above
            lazy_bnorm = false;
            HIPCHK(hipEventSynchronize(ctx->ev_join));
            ctx->prep.kind = KnpSidePrep::NONE;
            double nb2 = ctx->h_red[SIDE_SLOT];
            if (ctx->h_red[SIDE_SLOT + 1] != 0.0) {   // cancellation in the one-reduction norm: explicit projection and norm, in line
                ++ctx->n_norm_fallback;
                KCHK(pc_apply_proj(ctx, b, ctx->d_wb, cnt));
                KCHK(dot_to_slot(ctx, ctx->d_wb, ctx->d_wb, 60));
                KCHK(read_slots(ctx, 60, 1, ctx->seq_counter));
                nb2 = ctx->h_red[60];
                // ... which used the slots and vectors of the residual norm above: redo that one (rare)
                KCHK(redo_residual());
            }
            bnorm = std::sqrt(nb2);
            ctx->last_bnorm = bnorm;
            if (!std::isfinite(bnorm)) { *its = 0; *rnorm = bnorm; *reason = KNP_DIVERGED_NANORINF; return KNP_OK; }
            K.ttol = std::max(rtol * bnorm, atol);
        }
        const double beta = std::sqrt(ctx->h_red[60]);
        res = beta;
        if (res0 < 0) K.dref = res0 = beta;   // divergence is judged against the first preconditioned residual
        if (!std::isfinite(beta)) { *reason = KNP_DIVERGED_NANORINF; break; }
        if (beta <= K.ttol) { *reason = (beta <= atol) ? KNP_CONVERGED_ATOL : KNP_CONVERGED_RTOL; break; }
        if (it >= max_it) { *reason = KNP_DIVERGED_ITS; break; }
        if (!ahead) enqueue_v0(fused_norm);
        int jd = 0;
        bool stop = false;
        for (int j = 0; j < m; ++j) {
            const bool have = ahead && j == 0;   // iteration 0 ran ahead: its residual estimate and flag were read at the wait above
            int flag = have ? flag_a : 0;
            if (have) res = res_a;
            else KCHK(enqueue_iteration(j, ctx->update_early ? K.ttol : 0.0));
            KCHK(arnoldi_step_read(K, j, ctx->d_V + (size_t)(j + 1) * ldv, &res, &flag, have));
            if (krylov_stop_test(K, j, flag, res, max_it, &it, &jd, reason)) { stop = true; break; }
        }
        if (jd > 0) {
            ProfScope ps(ctx, 1);
            if (stop && tail_ok && jd <= 8) {
                OutPtrs o;
                KCHK(out_ptrs(ctx, &ctx->tail_target, o, true));
                hipLaunchKernelGGL(k_lincomb_unpack, dim3(nblocks(ctx->g.n_v)), dim3(NT), 0, st, GL, jd, gm, ctx->g.n_v, ldv, ctx->d_V, x, ctx->d_node_i,
                                   ctx->d_node_e, o, ctx->asm_dmax > 0 ? ctx->d_knod : nullptr);
                ctx->step.tail_done(x, ctx->asm_dmax > 0);
                KCHK(speculate_asm(ctx));   // the next step's matrix, behind this kernel on the assembly stream
            } else {
                krylov_update_plain(K, jd, ctx->d_V, x);
            }
        }
        if (stop) break;
    }
    return krylov_end(K, x, it, res, its, rnorm);
}

// ---- flexible GMRES(restart), right preconditioning, true-residual norm (KSPFGMRES; KSPGMRES with norm_type unpreconditioned) --------
// Per iteration: z_j = B v_j kept in a second basis Z (B may change between applications), w = A z_j, classical Gram-Schmidt of w
// against V with ONE reduction {V_i.w, w.w} whose first stage runs in the SpMV itself on one GPU (k_spmv_node_dots), Givens step and
// v_{j+1} by the shared arnoldi_step_finish.  Cycle end: x += Z y.  The residual estimate |g_{j+1}| is ||b - A x||_2.
int knp_fgmres_solve(knp_ctx* ctx, const double* b, double* x, double rtol, double atol, int32_t max_it, int32_t restart,
                     int32_t* its, double* rnorm, int32_t* reason) {
    CHECK_CTX(ctx);
    KrylovSolve K;   // K.ns stays off: Gram-Schmidt does not see the null space here (A ns = 0), the correction is projected once per cycle
    int64_t cnt;
    KCHK(krylov_begin(ctx, b, x, max_it, restart, its, rnorm, reason, true, &K, &cnt));
    const bool pc_none = ctx->pc_kind == KNP_PC_NONE;
    const int n = K.n, nb = K.nb, m = restart;
    const int64_t ldv = K.ldv;
    const GmLayout GL = K.GL;
    double* gm = K.gm;
    hipStream_t st = ctx->stream;

    // ||b|| for the relative tolerance (PETSc's KSPConvergedDefault with the unpreconditioned norm, initial guess zero or not)
    if (ctx->prep.kind == KnpSidePrep::FLEX && ctx->prep.b == b) {
        HIPCHK(hipEventSynchronize(ctx->ev_join));
        ctx->prep.kind = KnpSidePrep::NONE;
        if (!ctx->mirror()) HIPCHK(hipMemcpy(ctx->h_red + FB_SLOT, ctx->d_red + FB_SLOT, sizeof(double), hipMemcpyDeviceToHost));
    } else {
        side_discard(ctx);
        KCHK(dot_to_slot(ctx, b, b, FB_SLOT));
        KCHK(read_slots(ctx, FB_SLOT, 1, ctx->seq_counter));
    }
    const double bnorm = std::sqrt(ctx->h_red[FB_SLOT]);
    ctx->last_bnorm = bnorm;
    if (!std::isfinite(bnorm)) { *its = 0; *rnorm = bnorm; *reason = KNP_DIVERGED_NANORINF; return KNP_OK; }
    K.ttol = std::max(rtol * bnorm, atol);
    K.atol = atol;
    int it = 0;
    double res = 0.0, res0 = -1.0;
    *reason = 0;
    const bool ns = ctx->ns_on && cnt > 0;
    double* Zb = pc_none ? ctx->d_V : ctx->d_Z;
    while (true) {
        // r = b - A x and ||r||^2: one launch on one GPU (the residual form of the SpMV with its own norm), else SpMV + dot
        {
            int nbd = 0;
            if (launch_spmv_dots(ctx, x, b, ctx->d_w, 0, ldv, ctx->d_V, &nbd)) {
                ++ctx->n_allreduce;
                hipLaunchKernelGGL(k_reduce_fin, dim3(1), dim3(NT), 0, st, 3, nbd, 1, ctx->d_partial, ctx->d_red, 60, GL, 0, 0, 0.0, (double*)nullptr, 0,
                                   0.0, ctx->mirror(), ctx->mirror() ? ctx->h_seq_dev : nullptr, ++ctx->seq_counter, SPMV_WIDE);
                HIPCHK(hipGetLastError());
            } else {
                KCHK(spmv_A(ctx, x, b, ctx->d_w, true));
                KCHK(dot_to_slot(ctx, ctx->d_w, ctx->d_w, 60));
            }
            KCHK(read_slots(ctx, 60, 1, ctx->seq_counter));
        }
        const double beta = std::sqrt(ctx->h_red[60]);
        res = beta;
        if (res0 < 0) { res0 = beta; K.dref = bnorm > 0.0 ? bnorm : res0; }   // divergence is judged against ||b||
        if (!std::isfinite(beta)) { *reason = KNP_DIVERGED_NANORINF; break; }
        if (beta <= K.ttol) { *reason = (beta <= atol) ? KNP_CONVERGED_ATOL : KNP_CONVERGED_RTOL; break; }
        if (it >= max_it) { *reason = KNP_DIVERGED_ITS; break; }
        // v_0 = r / beta and g = (beta, 0, ..., 0) in one pass (k_scale_rsqrt_proj with a zero mean: r is not projected)
        hipLaunchKernelGGL(k_scale_rsqrt_proj, dim3(K.vec_blocks), dim3(NT), 0, st, n, ctx->d_w, ctx->d_red + 60, ctx->d_red + 60, 0.0, ctx->d_V,
                           gm + GL.g(), m);
        int jd = 0;
        bool stop = false;
        for (int j = 0; j < m; ++j) {
            double* vj = ctx->d_V + (size_t)j * ldv;
            double* vn = ctx->d_V + (size_t)(j + 1) * ldv;
            double* zj = Zb + (size_t)j * ldv;
            // z_j = B v_j, unprojected: A ns = 0, so w = A z_j does not see its gauge part (the correction is projected once per cycle)
            if (!pc_none) KCHK(pc_apply_proj(ctx, vj, zj, 0));
            int nbd = 0, flag = 0;
            const bool folded = j + 1 <= BU_MAX_M && launch_spmv_dots(ctx, zj, nullptr, ctx->d_w, j + 1, ldv, ctx->d_V, &nbd);
            if (!folded) KCHK(spmv_A(ctx, zj, nullptr, ctx->d_w, false));
            KCHK(arnoldi_step_finish(K, j, ctx->d_w, vn, folded ? nbd : 0, SPMV_WIDE, &res, &flag));
            if (krylov_stop_test(K, j, flag, res, max_it, &it, &jd, reason)) { stop = true; break; }
        }
        if (jd > 0) {   // x += Z y, without its null-space component when there is one (x keeps the gauge of the initial guess)
            ProfScope ps(ctx, 1);
            if (ns) {
                if (jd <= 8) {
                    hipLaunchKernelGGL(k_zcorr<true>, dim3(nb), dim3(NT), 0, st, GL, jd, gm, n, ldv, Zb, ctx->d_t, ctx->d_partial);
                } else {
                    hipLaunchKernelGGL(k_gm_solve_y, dim3(1), dim3(64), 0, st, GL, jd, gm);
                    hipLaunchKernelGGL(k_zcorr<false>, dim3(nb), dim3(NT), 0, st, GL, jd, gm, n, ldv, Zb, ctx->d_t, ctx->d_partial);
                }
                hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(NT), 0, st, nb, ctx->d_partial, ctx->d_red, 62, (double*)nullptr);
                KCHK(allreduce_slots(ctx, 62, 1));
                hipLaunchKernelGGL(k_axpy_proj, dim3(K.vec_blocks), dim3(NT), 0, st, n, ctx->d_t, ctx->d_red + 62, 1.0 / (double)cnt, x);
            } else {
                krylov_update_plain(K, jd, Zb, x);
            }
            HIPCHK(hipGetLastError());
        }
        if (stop) break;
    }
    return krylov_end(K, x, it, res, its, rnorm);
}
