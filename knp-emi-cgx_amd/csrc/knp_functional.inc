// Functionals: per-tag integrals of a bytecode program evaluated at the points of a quadrature rule, for any expression the
// membrane-program compiler takes.  This file holds what the kinds share and the volume kind (knp_functional_*):
// assemble_scalar(<expression> * dx(tag)) over cells.  knp_membrane_functional.inc holds the membrane kind.  Included at the end of
// knp_kernels.hip, after knp_diagnostics.inc (diag_chunk_partials, the combines, diag_map_set, by_dim, simplex_gradients), knp_sample.inc
// (sample_load_cell, SampleCell) and run_program.
//
// A functional is a plan owned by the context, like a sampling plan: its tag map (items sorted by dense tag index), its rule
// (barycentric points and weights), its program, which field slots the program reads and what every aux slot holds (its mode).
// Several of each kind may be live at once; each kind has its own table in the context, so its own ids.
// Shared by the kinds, over NV vertices per item (DIM + 1 of a cell, DIM of a facet):
//   fn_lane         the constants into LDS, the lane's item and its column of the interpreter's register file (dynamic LDS,
//                   [n_regs][FN_BT] doubles).  Idle lanes of the last block shadow the last item with weight zero, so the interpreter's
//                   wave stays uniform.
//   fn_load_fields  the vertex values of the fields the program reads, once, into registers.  Fields the program does not read are
//                   never touched: the mask is a kernel argument, the branch uniform.
//   fn_integrate    per quadrature point it interpolates the values and the coordinates, runs the interpreter and adds
//                   measure q_w[q] OUT_j, every output on its own; a slot of mode >= 0 is one number per item, kept in av[k][0].  Then
//                   the per-tag reduction, the diagnostics' own: diag_chunk_partials, and on the host k_diag_combine and, for the tags of
//                   more than FN_WAVE_CHUNKS chunks, k_diag_combine_long.  No atomics: the same inputs give the same bits on every run.
//                   With ITEMS it ends in a plain store instead (knp_fields.inc): the item's mean sum_q q_w[q] OUT_j, measure not
//                   applied, at dst[i n_out + j] of every live lane.  With LOAD (knp_fields.inc) every quadrature value is weighted
//                   with the P1 test function of each of the item's vertices, measure q_w[q] lambda_a OUT_j, and every live lane stores
//                   its NV x NOUT sums at dst[(i NV + a) n_out + j]: the element vectors of a linear form.
//   fn_create, fn_of, fn_set_constants, fn_eval, fn_destroy, fn_free   the plan's life, with the kind's name in the error texts.
// The volume kind's own:
//   k_functional    one cell per lane, FN_BT cells per block.  The lane loads its cell's vertices and coordinates and forms |T|.  A slot
//                   bound to a derivative holds sum_b grad(lambda_b)_a (f(v_b) - f(v_0)), constant on the cell, computed from the
//                   cell's coordinates; create refuses a flat cell then.

static constexpr int FN_BT = 128;              // items per block: the interpreter's LDS register file is [n_regs][FN_BT] doubles
static constexpr int FN_WAVE_CHUNKS = 64;      // longer tags take the workgroup combine
// which field slots a program reads: bit j k_i[j], bit 3 + j k_e[j], bit 6 phi_m, bit 7 + k aux[k]; from bit 15 up the kind's own
static constexpr unsigned FN_KI = 1u, FN_KE = 1u << 3, FN_PHIM = 1u << 6, FN_AUX = 1u << 7, FN_DERIV = 1u << 15;
enum FnEnd { FN_TAGS, FN_ITEMS, FN_LOAD };     // how fn_integrate ends: the per-tag reduction, the item's mean, the item's load vector
static constexpr int FN_NORMAL = 8;            // slot modes from here up have no field behind them (a membrane plan's normal components)
struct FnBind {
    unsigned need;
    int8_t mode[KNP_MAX_AUX];                  // aux_mode of the plan: -1 the slot holds the field's value, >= 0 one number per item
};
__host__ __device__ static inline bool fn_slot_field(unsigned need, const int8_t* mode, int k) { return (need & (FN_AUX << k)) && mode[k] < FN_NORMAL; }

// ---- the core both kinds share: NV vertices per item (DIM + 1 of a cell, DIM of a facet) -----------------------------------------
template <int NV>
struct FnValues {      // vertex values of the fields the program reads (0 elsewhere); a slot of mode >= 0 keeps its one value in av[k][0]
    double kv[2][3][NV], pv[NV], av[KNP_MAX_AUX][NV];
};
struct FnLane {
    int i, ii;         // the lane's item and the one it loads: idle lanes of the last block shadow the last item with weight zero
    bool live;
    const double* sk;  // the constants, in LDS
    double* reg;       // the lane's column of the interpreter's register file (dynamic LDS)
};

__device__ __forceinline__ FnLane fn_lane(int n, const DiagConsts& K, int n_consts) {
    extern __shared__ double dsmem[];
    __shared__ double sk[KNP_DIAG_MAX_CONSTS];      // 512 B: the dynamic base stays 16-byte aligned
    for (int i = threadIdx.x; i < n_consts; i += FN_BT) sk[i] = K.v[i];
    __syncthreads();
    FnLane L;
    L.i = blockIdx.x * FN_BT + threadIdx.x;
    L.live = L.i < n;
    L.ii = L.live ? L.i : n - 1;
    L.sk = sk;
    L.reg = dsmem + threadIdx.x;
    return L;
}

template <int NV>
__device__ __forceinline__ void fn_load_fields(const FieldPtrs& f, const FnBind& B, const int* v, FnValues<NV>& U) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const bool ri = B.need & (FN_KI << j), re = B.need & (FN_KE << j);
#pragma unroll
        for (int a = 0; a < NV; ++a) {
            U.kv[0][j][a] = ri ? f.ki[j][v[a]] : 0.0;
            U.kv[1][j][a] = re ? f.ke[j][v[a]] : 0.0;
        }
    }
#pragma unroll
    for (int a = 0; a < NV; ++a) U.pv[a] = (B.need & FN_PHIM) ? f.phim[v[a]] : 0.0;
#pragma unroll
    for (int k = 0; k < KNP_MAX_AUX; ++k) {
        const bool field = fn_slot_field(B.need, B.mode, k);
#pragma unroll
        for (int a = 0; a < NV; ++a) U.av[k][a] = field ? f.aux[k][v[a]] : 0.0;
    }
}

// Per quadrature point: interpolate the values and the coordinates x of the item's vertices, run the interpreter and add
// meas q_w[q] OUT_j, every output on its own; then the diagnostics' per-tag reduction of the block (diag_chunk_partials).  The order of
// a in the interpolation sums and of q in the accumulation fixes the bits.  ITEMS: the weight is q_w[q] alone and the end is one store
// per live lane, dst = the caller's [n][NOUT]; key is not read.  LOAD: NV x NOUT sums, acc[a][j] += (meas q_w[q] lam[a]) OUT_j in the same
// order of q, and the end is the store of all of them, dst = the caller's [n][NV][NOUT]: item-major, so that the gather of
// knp_scatter_apply finds the NOUT numbers of an entry (i, a) side by side; key is not read, and there is no reduction.
template <int DIM, int NV, int NOUT, FnEnd END, bool FUNCS>
__device__ __forceinline__ void fn_integrate(const FnLane& L, int n, const int32_t* __restrict__ key, const FnValues<NV>& U,
                                             const double (*x)[DIM], const FnBind& B, int n_q, const double* __restrict__ qp,
                                             const double* __restrict__ qw, double meas, const int32_t* __restrict__ code, int n_instr,
                                             double* __restrict__ partial) {
    constexpr bool ITEMS = END == FN_ITEMS;
    constexpr int NA = END == FN_LOAD ? NV : 1;      // accumulators per output
    double acc[NA][NOUT];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int j = 0; j < NOUT; ++j) acc[a][j] = 0.0;
    for (int q = 0; q < n_q; ++q) {
        double lam[NV];
#pragma unroll
        for (int a = 0; a < NV; ++a) lam[a] = qp[q * NV + a];
        double kiq[1][3], keq[1][3], phq[1] = {0.0}, auxq[1][KNP_MAX_AUX], xq[1][3], Iout[1][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double si = 0.0, se = 0.0;
#pragma unroll
            for (int a = 0; a < NV; ++a) {
                si += lam[a] * U.kv[0][j][a];
                se += lam[a] * U.kv[1][j][a];
            }
            kiq[0][j] = si;
            keq[0][j] = se;
            Iout[0][j] = 0.0;
        }
#pragma unroll
        for (int a = 0; a < NV; ++a) phq[0] += lam[a] * U.pv[a];
#pragma unroll
        for (int k = 0; k < KNP_MAX_AUX; ++k) {
            double t = 0.0;
#pragma unroll
            for (int a = 0; a < NV; ++a) t += lam[a] * U.av[k][a];
            const double one = U.av[k][0];
            auxq[0][k] = B.mode[k] >= 0 ? one : t;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double t = 0.0;
            if (d < DIM) {
#pragma unroll
                for (int a = 0; a < NV; ++a) t += lam[a] * x[a][d < DIM ? d : 0];
            }
            xq[0][d] = t;
        }
        run_program<1, FN_BT, FUNCS>(code, n_instr, L.sk, kiq, keq, phq, auxq, xq, Iout, L.reg);
        const double w = ITEMS ? qw[q] : qw[q] * meas;
        if constexpr (END == FN_LOAD) {
#pragma unroll
            for (int a = 0; a < NV; ++a) {
                const double wa = w * lam[a];
#pragma unroll
                for (int j = 0; j < NOUT; ++j) acc[a][j] += wa * Iout[0][j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < NOUT; ++j) acc[0][j] += w * Iout[0][j];
        }
    }
    if constexpr (END == FN_LOAD) {
        if (L.live) {
#pragma unroll
            for (int a = 0; a < NV; ++a)
#pragma unroll
                for (int j = 0; j < NOUT; ++j) partial[((size_t)L.i * NV + a) * NOUT + j] = acc[a][j];
        }
    } else if constexpr (ITEMS) {
        if (L.live) {
#pragma unroll
            for (int j = 0; j < NOUT; ++j) partial[(size_t)L.i * NOUT + j] = acc[0][j];
        }
    } else {
        DiagSum<NOUT> s;
#pragma unroll
        for (int j = 0; j < NOUT; ++j) s.v[j] = acc[0][j];
        diag_chunk_partials<DiagSum<NOUT>, FN_BT>(L.live ? key[L.i] : -1, L.live, L.i == n - 1, s, partial);
    }
}

// ---- the volume kind's own: the cell load, |T|, grad(lambda) and the derivative slots ---------------------------------------------
template <int DIM, int NOUT, FnEnd END = FN_TAGS, bool FUNCS = false>
__global__ void __launch_bounds__(FN_BT) k_functional(int n, const int32_t* __restrict__ item, const int32_t* __restrict__ key,
                                                      const int32_t* __restrict__ cells, const double* __restrict__ coords, int n_q,
                                                      const double* __restrict__ qb, const double* __restrict__ qw, FieldPtrs f, FnBind B,
                                                      const int32_t* __restrict__ code, int n_instr, DiagConsts K, int n_consts,
                                                      double* __restrict__ partial) {
    const FnLane L = fn_lane(n, K, n_consts);
    int v[DIM + 1];
    double x[DIM + 1][DIM];
    sample_load_cell<DIM>(item[L.ii], cells, coords, v, x);
    double e[DIM][DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int b = 0; b < DIM; ++b) e[a][b] = x[a + 1][b] - x[0][b];
    const double det = DIM == 2 ? e[0][0] * e[1][1] - e[0][1] * e[1][0]
                                : e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) - e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]) +
                                      e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
    const double vol = L.live ? fabs(det) / (DIM == 2 ? 2.0 : 6.0) : 0.0;
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
    FnValues<DIM + 1> U;
    fn_load_fields<DIM + 1>(f, B, v, U);
#pragma unroll
    for (int k = 0; k < KNP_MAX_AUX; ++k) {
        if ((B.need & (FN_AUX << k)) && B.mode[k] >= 0) {
            double d = 0.0;      // sum_b grad(lambda_b) f_b with sum_b grad(lambda_b) = 0: differences first, a field's offset cancels exactly
#pragma unroll
            for (int a = 1; a <= DIM; ++a) {
                double g = 0.0;
#pragma unroll
                for (int c = 0; c < DIM; ++c) g = B.mode[k] == c ? G[a][c] : g;
                d += g * (U.av[k][a] - U.av[k][0]);
            }
            U.av[k][0] = d;
        }
    }
    fn_integrate<DIM, DIM + 1, NOUT, END, FUNCS>(L, n, key, U, x, B, n_q, qb, qw, vol, code, n_instr, partial);
}

// ---- the plan lifecycle both kinds share.  A kind is its name in the error texts and its table of the context: the ids of the two
// ---- kinds are apart, a destroyed slot is taken by the kind's next create
struct FnKind {
    const char* name;
    std::vector<KnpFunctional>& plans;
};
static FnKind fn_volume(knp_ctx* ctx) { return {"functional", ctx->functionals}; }
static FnKind fn_membrane(knp_ctx* ctx) { return {"membrane functional", ctx->membrane_functionals}; }

static void fn_free(KnpFunctional& P) {
    diag_map_free(P.map);
    dev_free(P.d_code); dev_free(P.d_rec); dev_free(P.d_qp); dev_free(P.d_qw);
    P = KnpFunctional();
}
void knp_functional_free(knp_ctx* ctx) {
    for (auto* plans : {&ctx->functionals, &ctx->membrane_functionals}) {
        for (auto& P : *plans) fn_free(P);
        plans->clear();
    }
}

static int fn_of(knp_ctx* ctx, const FnKind& kind, int32_t id) {
    if (id < 0 || id >= (int)kind.plans.size() || !kind.plans[(size_t)id].live) {
        ctx->err = "unknown " + std::string(kind.name) + " " + std::to_string(id);
        return KNP_E_ARG;
    }
    return KNP_OK;
}

// Create of either kind.  The kind supplies mode_ok (is this slot mode one of its own, on this mesh), slot_need (what reading a slot of
// a mode adds to need besides the slot's own bit) and prepare (the checks of the listed items' geometry, and a membrane plan's records);
// nv is the number of barycentric coordinates of a quadrature point.
struct FnCreateArgs {      // the arguments of the two create entry points, in their order
    int32_t n_tags; const int32_t *seg_ptr, *items;
    int32_t n_q; const double *q_pts, *q_w;
    int32_t n_instr; const int32_t* code;
    int32_t n_consts; const double* consts;
    int32_t n_aux; const int32_t* aux_mode;
    int32_t n_out; int32_t* id;
};
template <class ModeOk, class SlotNeed, class Prepare>
static int fn_create(knp_ctx* ctx, const FnKind& kind, const FnCreateArgs& a, int n_items, int nv, const char* map_name, const char* mode_text,
                     ModeOk mode_ok, SlotNeed slot_need, Prepare prepare) {
    const std::string pre = std::string(kind.name) + ": ";
    if (!a.id || !a.q_pts || !a.q_w || !a.code || (a.n_consts > 0 && !a.consts) || (a.n_aux > 0 && !a.aux_mode)) { ctx->err = pre + "null argument"; return KNP_E_ARG; }
    if (a.n_q < 1 || a.n_q > KNP_FUNCTIONAL_MAX_Q) { ctx->err = pre + "n_q must be 1.." + std::to_string(KNP_FUNCTIONAL_MAX_Q); return KNP_E_ARG; }
    if (a.n_out < 1 || a.n_out > 3) { ctx->err = pre + "n_out must be 1..3"; return KNP_E_ARG; }
    if (a.n_aux < 0 || a.n_aux > KNP_MAX_AUX) { ctx->err = pre + "n_aux must be 0.." + std::to_string(KNP_MAX_AUX); return KNP_E_ARG; }
    if (a.n_instr < 1) { ctx->err = pre + "empty program"; return KNP_E_ARG; }
    if (a.n_consts < 0 || a.n_consts > KNP_DIAG_MAX_CONSTS) { ctx->err = pre + "at most " + std::to_string(KNP_DIAG_MAX_CONSTS) + " constants"; return KNP_E_ARG; }
    KnpFunctional P;
    for (int k = 0; k < a.n_aux; ++k) {
        if (!mode_ok(a.aux_mode[k])) { ctx->err = pre + mode_text; return KNP_E_ARG; }
        P.aux_mode[k] = (int8_t)a.aux_mode[k];
    }
    KCHK(validate_program(ctx, a.n_instr, a.code, a.n_consts, &P.n_regs));
    P.funcs = program_uses_funcs(a.n_instr, a.code);
    for (int i = 0; i < a.n_instr; ++i) {       // which slots the code reads; the indices are validate_program's
        const int op = a.code[4 * i], s = a.code[4 * i + 2];
        if (op == KNP_OP_KI) P.need |= FN_KI << s;
        else if (op == KNP_OP_KE) P.need |= FN_KE << s;
        else if (op == KNP_OP_PHIM) P.need |= FN_PHIM;
        else if (op == KNP_OP_AUX) {
            if (s >= a.n_aux) { ctx->err = pre + "instruction " + std::to_string(i) + " reads aux slot " + std::to_string(s) + " of " + std::to_string(a.n_aux); return KNP_E_ARG; }
            P.need |= (FN_AUX << s) | slot_need(P.aux_mode[s]);
        } else if (op == KNP_OP_OUT && s >= a.n_out) {
            ctx->err = pre + "instruction " + std::to_string(i) + " writes output " + std::to_string(s) + " of " + std::to_string(a.n_out);
            return KNP_E_ARG;
        }
    }
    KCHK(diag_map_set(ctx, P.map, a.n_tags, a.seg_ptr, a.items, n_items, FN_BT, a.n_out, FN_WAVE_CHUNKS, map_name));
    const int rc = [&]() -> int {
        KCHK(prepare(P));
        KCHK(dev_upload_raw(ctx, &P.d_code, a.code, (size_t)4 * a.n_instr));
        KCHK(dev_upload_raw(ctx, &P.d_qp, a.q_pts, (size_t)a.n_q * nv));
        KCHK(dev_upload_raw(ctx, &P.d_qw, a.q_w, (size_t)a.n_q));
        return KNP_OK;
    }();
    if (rc != KNP_OK) {
        fn_free(P);
        return rc;
    }
    P.n_q = a.n_q; P.n_out = a.n_out; P.n_instr = a.n_instr; P.n_consts = a.n_consts;
    for (int i = 0; i < a.n_consts; ++i) P.consts[i] = a.consts[i];
    P.live = true;
    size_t slot = 0;
    while (slot < kind.plans.size() && kind.plans[slot].live) ++slot;
    if (slot == kind.plans.size()) kind.plans.emplace_back();
    kind.plans[slot] = P;
    *a.id = (int32_t)slot;
    return KNP_OK;
}

static int fn_set_constants(knp_ctx* ctx, const FnKind& kind, int32_t id, int32_t n_consts, const double* consts) {
    KCHK(fn_of(ctx, kind, id));
    KnpFunctional& P = kind.plans[(size_t)id];
    if (n_consts != P.n_consts || (n_consts && !consts)) { ctx->err = std::string(kind.name) + ": constant count mismatch"; return KNP_E_ARG; }
    for (int i = 0; i < n_consts; ++i) P.consts[i] = consts[i];   // kernel arguments of the next launch: nothing to copy
    return KNP_OK;
}

// Evaluation of either kind: binds the fields the program reads, then launch(D, NOUT, END, M, P, f, B, K, lds, dst) is the kind's kernel
// over the plan's map (M: its FUNCS instantiation, for a program with KNP_OP_SIN / COS / TANH), and the combines write out.  FN_ITEMS / FN_LOAD (knp_fields.inc): the kernel stores every item's mean, or its
// load vector, straight into out (dst = out, [n][n_out] or [n][nv][n_out] in the plan's item order) and there is no combine; otherwise
// dst is the map's partials.
template <FnEnd END, class Launch>
static int fn_eval(knp_ctx* ctx, const FnKind& kind, int32_t id, const knp_fields* fields, double* out, Launch launch) {
    KCHK(fn_of(ctx, kind, id));
    const KnpFunctional& P = kind.plans[(size_t)id];
    const KnpDiagMap& m = P.map;
    constexpr bool ITEMS = END != FN_TAGS;      // the ends that store per item
    if (ITEMS ? m.n == 0 : m.n_tags == 0) return KNP_OK;
    if (!fields || !out) { ctx->err = std::string(kind.name) + ": null fields or null output buffer"; return KNP_E_ARG; }
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
        const bool reads = fn_slot_field(P.need, P.aux_mode, k);
        f.aux[k] = reads ? fields->aux[k] : nullptr;
        missing = missing || (reads && !f.aux[k]);
    }
    if (missing) { ctx->err = std::string(kind.name) + ": a field the program reads is null"; return KNP_E_ARG; }
    if (m.n > 0) {
        FnBind B;
        B.need = P.need;
        for (int k = 0; k < KNP_MAX_AUX; ++k) B.mode[k] = P.aux_mode[k];
        DiagConsts K;
        for (int i = 0; i < KNP_DIAG_MAX_CONSTS; ++i) K.v[i] = i < P.n_consts ? P.consts[i] : 0.0;
        const size_t lds = (size_t)std::max(P.n_regs, 1) * FN_BT * sizeof(double);   // <= 48 registers: 48 KiB
        double* dst = ITEMS ? out : m.d_partial;
        const std::integral_constant<FnEnd, END> items;
        by_dim(ctx->g.dim, [&](auto D) {
            with_flag(P.funcs, [&](auto M) {
                if (P.n_out == 1) launch(D, std::integral_constant<int, 1>(), items, M, P, f, B, K, lds, dst);
                else if (P.n_out == 2) launch(D, std::integral_constant<int, 2>(), items, M, P, f, B, K, lds, dst);
                else launch(D, std::integral_constant<int, 3>(), items, M, P, f, B, K, lds, dst);
            });
        });
        HIPCHK(hipGetLastError());
    }
    if (ITEMS) return KNP_OK;
    if (P.n_out == 1) return diag_combine<DiagSum<1>>(ctx, m, out);
    if (P.n_out == 2) return diag_combine<DiagSum<2>>(ctx, m, out);
    return diag_combine<DiagSum<3>>(ctx, m, out);
}

static int fn_destroy(knp_ctx* ctx, const FnKind& kind, int32_t id) {
    KCHK(fn_of(ctx, kind, id));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // an evaluation in flight may still read the plan
    fn_free(kind.plans[(size_t)id]);
    return KNP_OK;
}

// ---- the volume kind's host part ------------------------------------------------------------------------------------------------------
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

// the volume kind's launch, of either end (fn_eval)
template <FnEnd END>
static int functional_eval(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out) {
    return fn_eval<END>(ctx, fn_volume(ctx), id, fields, out,
                          [&](auto D, auto NOUT, auto I, auto M, const KnpFunctional& P, const FieldPtrs& f, const FnBind& B, const DiagConsts& K,
                              size_t lds, double* dst) {
                              const KnpDiagMap& m = P.map;
                              hipLaunchKernelGGL((k_functional<D(), NOUT(), I(), M()>), dim3(m.n_chunks), dim3(FN_BT), lds, ctx->stream, m.n, m.d_item,
                                                 m.d_key, ctx->d_cells, ctx->d_coords, P.n_q, P.d_qp, P.d_qw, f, B, P.d_code, P.n_instr, K,
                                                 P.n_consts, dst);
                          });
}

extern "C" {

int knp_functional_create(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr, const int32_t* cells, int32_t n_q, const double* q_bary,
                          const double* q_w, int32_t n_instr, const int32_t* code, int32_t n_consts, const double* consts, int32_t n_aux,
                          const int32_t* aux_deriv, int32_t n_out, int32_t* id) {
    CHECK_CTX(ctx);
    const KnpHostGraph& g = ctx->g;
    const FnCreateArgs a = {n_tags, seg_ptr, cells, n_q, q_bary, q_w, n_instr, code, n_consts, consts, n_aux, aux_deriv, n_out, id};
    return fn_create(
        ctx, fn_volume(ctx), a, g.n_c_owned, g.dim + 1, "functional cell map", "aux_deriv must be -1 (value) or an axis below the mesh's dimension",
        [&](int m) { return m >= -1 && m < g.dim; }, [](int m) { return m >= 0 ? FN_DERIV : 0u; },
        [&](KnpFunctional& P) -> int {
            if (!(P.need & FN_DERIV) || P.map.n == 0) return KNP_OK;
            std::vector<int32_t> hc((size_t)g.n_c * (g.dim + 1));
            std::vector<double> hx((size_t)g.n_v * g.dim);
            HIPCHK(hipMemcpy(hc.data(), ctx->d_cells, hc.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(hx.data(), ctx->d_coords, hx.size() * sizeof(double), hipMemcpyDeviceToHost));
            if (by_dim(g.dim, [&](auto D) { return functional_flat_cell<D()>(hc, hx, cells, P.map.n); })) {
                ctx->err = "functional: a derivative is bound and a listed cell is flat";
                return KNP_E_MESH;
            }
            return KNP_OK;
        });
}

int knp_functional_set_constants(knp_ctx* ctx, int32_t id, int32_t n_consts, const double* consts) {
    CHECK_CTX(ctx);
    return fn_set_constants(ctx, fn_volume(ctx), id, n_consts, consts);
}

int knp_functional_eval(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out) {
    CHECK_CTX(ctx);
    return functional_eval<FN_TAGS>(ctx, id, fields, out);
}

int knp_functional_destroy(knp_ctx* ctx, int32_t id) {
    CHECK_CTX(ctx);
    return fn_destroy(ctx, fn_volume(ctx), id);
}

}  // extern "C"
