// Volume functionals (knp_functional_*): per-tag integrals over cells of a bytecode program evaluated at the points of a simplex
// quadrature rule -- assemble_scalar(<expression> * dx(tag)) for any expression the membrane-program compiler takes.
// Included at the end of knp_kernels.hip, after knp_diagnostics.inc (diag_chunk_partials, the combines, diag_map_set, by_dim,
// simplex_gradients), knp_sample.inc (sample_load_cell, SampleCell) and run_program.
//
// A functional is a plan owned by the context, like a sampling plan: its tag map (owned cells sorted by dense tag index), its rule
// (barycentric points and weights), its program and which field slots the program reads.  Several may be live at once.
//   k_functional   one cell per lane, FN_BT cells per block.  The lane loads its cell's vertices, coordinates and the vertex values of
//                  the fields the program reads once, into registers; per quadrature point it interpolates them, runs the interpreter
//                  (register file in dynamic LDS, [n_regs][FN_BT] doubles) and adds |T| q_w[q] OUT_j.  A slot bound to a derivative
//                  holds sum_b grad(lambda_b)_a (f(v_b) - f(v_0)), constant on the cell, computed from the cell's coordinates.  Fields the
//                  program does not read are never touched: the mask is a kernel argument, the branch uniform.  Idle lanes of the
//                  last block shadow the last cell with weight zero, so the interpreter's wave stays uniform.
// The per-tag reduction is the diagnostics' own: diag_chunk_partials, then k_diag_combine and, for the tags of more than
// FN_WAVE_CHUNKS chunks, k_diag_combine_long.  No atomics: the same inputs give the same bits on every run.

static constexpr int FN_BT = 128;              // cells per block: the interpreter's LDS register file is [n_regs][FN_BT] doubles
static constexpr int FN_WAVE_CHUNKS = 64;      // longer tags take the workgroup combine
// which field slots a program reads: bit j k_i[j], bit 3 + j k_e[j], bit 6 phi_m, bit 7 + k aux[k], bit 15 some slot is a derivative
static constexpr unsigned FN_KI = 1u, FN_KE = 1u << 3, FN_PHIM = 1u << 6, FN_AUX = 1u << 7, FN_DERIV = 1u << 15;
struct FnBind {
    unsigned need;
    int8_t deriv[KNP_MAX_AUX];                 // -1: the slot holds the field's value, a: d/dx_a of the field
};

template <int DIM, int NOUT>
__global__ void __launch_bounds__(FN_BT) k_functional(int n, const int32_t* __restrict__ item, const int32_t* __restrict__ key,
                                                      const int32_t* __restrict__ cells, const double* __restrict__ coords, int n_q,
                                                      const double* __restrict__ qb, const double* __restrict__ qw, FieldPtrs f, FnBind B,
                                                      const int32_t* __restrict__ code, int n_instr, DiagConsts K, int n_consts,
                                                      double* __restrict__ partial) {
    extern __shared__ double dsmem[];     // register file of the interpreter
    __shared__ double sk[KNP_DIAG_MAX_CONSTS];
    for (int i = threadIdx.x; i < n_consts; i += FN_BT) sk[i] = K.v[i];
    __syncthreads();
    const int i = blockIdx.x * FN_BT + threadIdx.x;
    const bool live = i < n;
    const int ii = live ? i : n - 1;      // idle lanes shadow the last cell with weight zero
    int v[DIM + 1];
    double x[DIM + 1][DIM];
    sample_load_cell<DIM>(item[ii], cells, coords, v, x);
    double e[DIM][DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b) e[a][b] = x[a + 1][b] - x[0][b];
    const double det = DIM == 2 ? e[0][0] * e[1][1] - e[0][1] * e[1][0]
                                : e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) - e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]) +
                                      e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
    const double vol = live ? fabs(det) / (DIM == 2 ? 2.0 : 6.0) : 0.0;
    double G[DIM + 1][DIM];               // grad(lambda_a), a >= 1; read only where a slot is a derivative (create refused flat cells then)
#pragma unroll
    for (int a = 0; a <= DIM; ++a)
#pragma unroll
        for (int c = 0; c < DIM; ++c) G[a][c] = 0.0;
    if (B.need & FN_DERIV) {
        SampleCell<DIM> T;
        T.setup(x);
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
            for (int c = 0; c < DIM; ++c) G[a + 1][c] = T.inv[a][c];
    }
    // vertex values of the fields the program reads (0 elsewhere); a derivative slot keeps its one value in av[k][0]
    double kv[2][3][DIM + 1], pv[DIM + 1], av[KNP_MAX_AUX][DIM + 1];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const bool ri = B.need & (FN_KI << j), re = B.need & (FN_KE << j);
#pragma unroll
        for (int a = 0; a <= DIM; ++a) {
            kv[0][j][a] = ri ? f.ki[j][v[a]] : 0.0;
            kv[1][j][a] = re ? f.ke[j][v[a]] : 0.0;
        }
    }
#pragma unroll
    for (int a = 0; a <= DIM; ++a) pv[a] = (B.need & FN_PHIM) ? f.phim[v[a]] : 0.0;
#pragma unroll
    for (int k = 0; k < KNP_MAX_AUX; ++k) {
        const bool r = B.need & (FN_AUX << k);
#pragma unroll
        for (int a = 0; a <= DIM; ++a) av[k][a] = r ? f.aux[k][v[a]] : 0.0;
        if (r && B.deriv[k] >= 0) {
            double d = 0.0;      // sum_b grad(lambda_b) f_b with sum_b grad(lambda_b) = 0: differences first, a field's offset cancels exactly
#pragma unroll
            for (int a = 1; a <= DIM; ++a) {
                double g = 0.0;
#pragma unroll
                for (int c = 0; c < DIM; ++c) g = B.deriv[k] == c ? G[a][c] : g;
                d += g * (av[k][a] - av[k][0]);
            }
            av[k][0] = d;
        }
    }
    double* reg = dsmem + threadIdx.x;
    double acc[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) acc[j] = 0.0;
    for (int q = 0; q < n_q; ++q) {
        double lam[DIM + 1];
#pragma unroll
        for (int a = 0; a <= DIM; ++a) lam[a] = qb[q * (DIM + 1) + a];
        double kiq[1][3], keq[1][3], phq[1] = {0.0}, auxq[1][KNP_MAX_AUX], xq[1][3], Iout[1][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double si = 0.0, se = 0.0;
#pragma unroll
            for (int a = 0; a <= DIM; ++a) {
                si += lam[a] * kv[0][j][a];
                se += lam[a] * kv[1][j][a];
            }
            kiq[0][j] = si;
            keq[0][j] = se;
            Iout[0][j] = 0.0;
        }
#pragma unroll
        for (int a = 0; a <= DIM; ++a) phq[0] += lam[a] * pv[a];
#pragma unroll
        for (int k = 0; k < KNP_MAX_AUX; ++k) {
            double t = 0.0;
#pragma unroll
            for (int a = 0; a <= DIM; ++a) t += lam[a] * av[k][a];
            auxq[0][k] = B.deriv[k] >= 0 ? av[k][0] : t;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double t = 0.0;
            if (d < DIM) {
#pragma unroll
                for (int a = 0; a <= DIM; ++a) t += lam[a] * x[a][d < DIM ? d : 0];
            }
            xq[0][d] = t;
        }
        run_program<1, FN_BT>(code, n_instr, sk, kiq, keq, phq, auxq, xq, Iout, reg);
        const double w = qw[q] * vol;
#pragma unroll
        for (int j = 0; j < NOUT; ++j) acc[j] += w * Iout[0][j];
    }
    DiagSum<NOUT> s;
#pragma unroll
    for (int j = 0; j < NOUT; ++j) s.v[j] = acc[j];
    diag_chunk_partials<DiagSum<NOUT>, FN_BT>(live ? key[i] : -1, live, i == n - 1, s, partial);
}

static void functional_free(KnpFunctional& P) {
    diag_map_free(P.map);
    dev_free(P.d_code); dev_free(P.d_qb); dev_free(P.d_qw);
    P = KnpFunctional();
}
void knp_functional_free(knp_ctx* ctx) {
    for (auto& P : ctx->functionals) functional_free(P);
    ctx->functionals.clear();
}

static int functional_of(knp_ctx* ctx, int32_t id) {
    if (id < 0 || id >= (int)ctx->functionals.size() || !ctx->functionals[(size_t)id].live) {
        ctx->err = "unknown functional " + std::to_string(id);
        return KNP_E_ARG;
    }
    return KNP_OK;
}

// a listed cell whose barycentric gradients do not exist: zero determinant, or one so small that they are not finite
template <int DIM>
static bool functional_flat_cell(const std::vector<int32_t>& cells, const std::vector<double>& coords, const int32_t* list, int n) {
    int64_t bad = 0;
#pragma omp parallel for schedule(static) reduction(+ : bad) num_threads(knp_host_threads())
    for (int i = 0; i < n; ++i) {
        double x[DIM + 1][3], G[DIM + 1][3];
        for (int a = 0; a <= DIM; ++a)
            for (int c = 0; c < DIM; ++c) x[a][c] = coords[(size_t)cells[(size_t)list[i] * (DIM + 1) + a] * DIM + c];
        bool ok = simplex_gradients<DIM>(x, G);
        for (int a = 0; a <= DIM && ok; ++a)
            for (int c = 0; c < DIM; ++c) ok = ok && std::isfinite(G[a][c]);
        if (!ok) ++bad;
    }
    return bad != 0;
}

template <int DIM, int NOUT>
static void functional_launch(knp_ctx* ctx, const KnpFunctional& P, const FieldPtrs& f, const FnBind& B, const DiagConsts& K, size_t lds) {
    const KnpDiagMap& m = P.map;
    hipLaunchKernelGGL((k_functional<DIM, NOUT>), dim3(m.n_chunks), dim3(FN_BT), lds, ctx->stream, m.n, m.d_item, m.d_key, ctx->d_cells,
                       ctx->d_coords, P.n_q, P.d_qb, P.d_qw, f, B, P.d_code, P.n_instr, K, P.n_consts, m.d_partial);
}

extern "C" {

int knp_functional_create(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr, const int32_t* cells, int32_t n_q, const double* q_bary,
                          const double* q_w, int32_t n_instr, const int32_t* code, int32_t n_consts, const double* consts, int32_t n_aux,
                          const int32_t* aux_deriv, int32_t n_out, int32_t* id) {
    CHECK_CTX(ctx);
    const KnpHostGraph& g = ctx->g;
    if (!id || !q_bary || !q_w || !code || (n_consts > 0 && !consts) || (n_aux > 0 && !aux_deriv)) { ctx->err = "functional: null argument"; return KNP_E_ARG; }
    if (n_q < 1 || n_q > KNP_FUNCTIONAL_MAX_Q) { ctx->err = "functional: n_q must be 1.." + std::to_string(KNP_FUNCTIONAL_MAX_Q); return KNP_E_ARG; }
    if (n_out < 1 || n_out > 3) { ctx->err = "functional: n_out must be 1..3"; return KNP_E_ARG; }
    if (n_aux < 0 || n_aux > KNP_MAX_AUX) { ctx->err = "functional: n_aux must be 0.." + std::to_string(KNP_MAX_AUX); return KNP_E_ARG; }
    if (n_instr < 1) { ctx->err = "functional: empty program"; return KNP_E_ARG; }
    if (n_consts < 0 || n_consts > KNP_DIAG_MAX_CONSTS) { ctx->err = "functional: at most " + std::to_string(KNP_DIAG_MAX_CONSTS) + " constants"; return KNP_E_ARG; }
    FnBind B;
    B.need = 0;
    for (int k = 0; k < KNP_MAX_AUX; ++k) {
        B.deriv[k] = -1;
        if (k >= n_aux) continue;
        if (aux_deriv[k] < -1 || aux_deriv[k] >= g.dim) { ctx->err = "functional: aux_deriv must be -1 (value) or an axis below the mesh's dimension"; return KNP_E_ARG; }
        B.deriv[k] = (int8_t)aux_deriv[k];
    }
    int n_regs = 0;
    KCHK(validate_program(ctx, n_instr, code, n_consts, &n_regs));
    for (int i = 0; i < n_instr; ++i) {       // which slots the code reads; the indices are validate_program's
        const int op = code[4 * i], a = code[4 * i + 2];
        if (op == KNP_OP_KI) B.need |= FN_KI << a;
        else if (op == KNP_OP_KE) B.need |= FN_KE << a;
        else if (op == KNP_OP_PHIM) B.need |= FN_PHIM;
        else if (op == KNP_OP_AUX) {
            if (a >= n_aux) { ctx->err = "functional: instruction " + std::to_string(i) + " reads aux slot " + std::to_string(a) + " of " + std::to_string(n_aux); return KNP_E_ARG; }
            B.need |= FN_AUX << a;
            if (B.deriv[a] >= 0) B.need |= FN_DERIV;
        } else if (op == KNP_OP_OUT && a >= n_out) {
            ctx->err = "functional: instruction " + std::to_string(i) + " writes output " + std::to_string(a) + " of " + std::to_string(n_out);
            return KNP_E_ARG;
        }
    }
    KnpFunctional P;
    KCHK(diag_map_set(ctx, P.map, n_tags, seg_ptr, cells, g.n_c_owned, FN_BT, n_out, FN_WAVE_CHUNKS, "functional cell map"));
    const int rc = [&]() -> int {
        if ((B.need & FN_DERIV) && P.map.n > 0) {
            std::vector<int32_t> hc((size_t)g.n_c * (g.dim + 1));
            std::vector<double> hx((size_t)g.n_v * g.dim);
            HIPCHK(hipMemcpy(hc.data(), ctx->d_cells, hc.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(hx.data(), ctx->d_coords, hx.size() * sizeof(double), hipMemcpyDeviceToHost));
            if (by_dim(g.dim, [&](auto D) { return functional_flat_cell<D()>(hc, hx, cells, P.map.n); })) {
                ctx->err = "functional: a derivative is bound and a listed cell is flat";
                return KNP_E_MESH;
            }
        }
        KCHK(dev_upload_raw(ctx, &P.d_code, code, (size_t)4 * n_instr));
        KCHK(dev_upload_raw(ctx, &P.d_qb, q_bary, (size_t)n_q * (g.dim + 1)));
        KCHK(dev_upload_raw(ctx, &P.d_qw, q_w, (size_t)n_q));
        return KNP_OK;
    }();
    if (rc != KNP_OK) {
        functional_free(P);
        return rc;
    }
    P.n_q = n_q; P.n_out = n_out; P.n_instr = n_instr; P.n_regs = n_regs; P.n_consts = n_consts;
    P.need = B.need;
    for (int k = 0; k < KNP_MAX_AUX; ++k) P.aux_deriv[k] = B.deriv[k];
    for (int i = 0; i < n_consts; ++i) P.consts[i] = consts[i];
    P.live = true;
    size_t slot = 0;
    while (slot < ctx->functionals.size() && ctx->functionals[slot].live) ++slot;
    if (slot == ctx->functionals.size()) ctx->functionals.emplace_back();
    ctx->functionals[slot] = P;
    *id = (int32_t)slot;
    return KNP_OK;
}

int knp_functional_set_constants(knp_ctx* ctx, int32_t id, int32_t n_consts, const double* consts) {
    CHECK_CTX(ctx);
    KCHK(functional_of(ctx, id));
    KnpFunctional& P = ctx->functionals[(size_t)id];
    if (n_consts != P.n_consts || (n_consts && !consts)) { ctx->err = "functional: constant count mismatch"; return KNP_E_ARG; }
    for (int i = 0; i < n_consts; ++i) P.consts[i] = consts[i];   // kernel arguments of the next launch: nothing to copy
    return KNP_OK;
}

int knp_functional_eval(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out) {
    CHECK_CTX(ctx);
    KCHK(functional_of(ctx, id));
    const KnpFunctional& P = ctx->functionals[(size_t)id];
    const KnpDiagMap& m = P.map;
    if (m.n_tags == 0) return KNP_OK;
    if (!fields || !out) { ctx->err = "functional: null fields or null output buffer"; return KNP_E_ARG; }
    FieldPtrs f;
    bool missing = false;
    for (int j = 0; j < 3; ++j) {
        f.ki[j] = (P.need & (FN_KI << j)) ? fields->k_i[j] : nullptr;
        f.ke[j] = (P.need & (FN_KE << j)) ? fields->k_e[j] : nullptr;
        missing = missing || ((P.need & (FN_KI << j)) && !f.ki[j]) || ((P.need & (FN_KE << j)) && !f.ke[j]);
    }
    f.phim = (P.need & FN_PHIM) ? fields->phi_m : nullptr;
    missing = missing || ((P.need & FN_PHIM) && !f.phim);
    for (int k = 0; k < KNP_MAX_AUX; ++k) {
        f.aux[k] = (P.need & (FN_AUX << k)) ? fields->aux[k] : nullptr;
        missing = missing || ((P.need & (FN_AUX << k)) && !f.aux[k]);
    }
    if (missing) { ctx->err = "functional: a field the program reads is null"; return KNP_E_ARG; }
    if (m.n > 0) {
        FnBind B;
        B.need = P.need;
        for (int k = 0; k < KNP_MAX_AUX; ++k) B.deriv[k] = P.aux_deriv[k];
        DiagConsts K;
        for (int i = 0; i < KNP_DIAG_MAX_CONSTS; ++i) K.v[i] = i < P.n_consts ? P.consts[i] : 0.0;
        const size_t lds = (size_t)std::max(P.n_regs, 1) * FN_BT * sizeof(double);   // <= 48 registers: 48 KiB
        by_dim(ctx->g.dim, [&](auto D) {
            if (P.n_out == 1) functional_launch<D(), 1>(ctx, P, f, B, K, lds);
            else if (P.n_out == 2) functional_launch<D(), 2>(ctx, P, f, B, K, lds);
            else functional_launch<D(), 3>(ctx, P, f, B, K, lds);
        });
        HIPCHK(hipGetLastError());
    }
    if (P.n_out == 1) return diag_combine<DiagSum<1>>(ctx, m, out);
    if (P.n_out == 2) return diag_combine<DiagSum<2>>(ctx, m, out);
    return diag_combine<DiagSum<3>>(ctx, m, out);
}

int knp_functional_destroy(knp_ctx* ctx, int32_t id) {
    CHECK_CTX(ctx);
    KCHK(functional_of(ctx, id));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // an evaluation in flight may still read the plan
    functional_free(ctx->functionals[(size_t)id]);
    return KNP_OK;
}

}  // extern "C"
