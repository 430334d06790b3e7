// Membrane functionals (knp_membrane_functional_*): per-tag integrals over membrane facets of a bytecode program evaluated at the
// points of a facet quadrature rule -- assemble_scalar(<expression> * dS(tag)) with one-sided gradients ('+' / '-' restrictions), the
// facet normal and normal derivatives.  Included at the end of knp_kernels.hip, after knp_functional.inc (the FN_* bits, FN_BT), whose
// helpers it shares: diag_chunk_partials, the combines, diag_map_set, by_dim, simplex_gradients, SampleCell and run_program.
//
// A membrane functional is a plan owned by the context, like a volume functional: its facet map (indices into the Gamma list sorted by
// dense tag index), its rule (barycentric points on the facet and weights), its program, what every aux slot holds (its mode) and one
// record per listed facet, in map order:
//   2 x int4 -- the facet's vertices f_0..f_{DIM-1} followed by the opposite vertex, once for the intracellular cell and once for the
//   extracellular one (in 2D the fourth id repeats f_0).  An extracellular cell that does not hold the facet leaves f_0 in the place
//   of its opposite vertex; create refuses such a facet when a mode of that cell is bound.
//   k_membrane_functional   one facet per lane, FN_BT facets per block.  The lane loads its record, the facet's coordinates and the
//                  vertex values of the fields the program reads (mask in a kernel argument, uniform branches).  Only where a slot is
//                  geometric it loads the opposite vertices and forms grad(lambda) of the two cells and the normal
//                  n_i = -grad(lambda_opp) / |grad(lambda_opp)| of the intracellular cell (the rule of flux_records; n_e = -n_i).  A
//                  derivative slot is reduced once per facet to sum_{b>=1} g_b (f(v_b) - f(v_0)), g_b = grad(lambda_b)_a or
//                  grad(lambda_b) . n: differences first, a field's constant offset cancels exactly.  Per quadrature point it
//                  interpolates the values and coordinates on the facet, runs the interpreter (register file in dynamic LDS) and adds
//                  |F| q_w[q] OUT_j, every output on its own.  Idle lanes shadow the last facet with weight zero.
// The per-tag reduction is the diagnostics' own (diag_chunk_partials, k_diag_combine, k_diag_combine_long): no atomics, the same bits
// on every run.

// bits of MfBind::need above the field bits of knp_functional.inc: the cells whose geometry some slot the code reads needs
static constexpr unsigned MF_GEOM_I = 1u << 15, MF_GEOM_E = 1u << 16;
static constexpr int MF_DN_I = 6, MF_DN_E = 7, MF_NORMAL = 8;      // slot modes besides -1 (value), a (d/dx_a, '+' cell), 3 + a ('-' cell)
struct MfBind {
    unsigned need;
    int8_t mode[KNP_MAX_AUX];
};
static inline bool mf_mode_ext(int m) { return (m >= 3 && m < MF_DN_I) || m == MF_DN_E; }            // reads the extracellular cell
static inline bool mf_mode_int(int m) { return (m >= 0 && m < 3) || m == MF_DN_I || m == MF_DN_E || m >= MF_NORMAL; }   // the normal is the intracellular cell's

template <int DIM, int NOUT>
__global__ void __launch_bounds__(FN_BT) k_membrane_functional(int n, const int32_t* __restrict__ item, const int32_t* __restrict__ key,
                                                               const int4* __restrict__ rec, const double* __restrict__ fmeas,
                                                               const double* __restrict__ coords, int n_q, const double* __restrict__ qp,
                                                               const double* __restrict__ qw, FieldPtrs f, MfBind B,
                                                               const int32_t* __restrict__ code, int n_instr, DiagConsts K, int n_consts,
                                                               double* __restrict__ partial) {
    extern __shared__ double dsmem[];     // register file of the interpreter
    __shared__ double sk[KNP_DIAG_MAX_CONSTS];      // 512 B: the dynamic base stays 16-byte aligned
    for (int i = threadIdx.x; i < n_consts; i += FN_BT) sk[i] = K.v[i];
    __syncthreads();
    const int i = blockIdx.x * FN_BT + threadIdx.x;
    const bool live = i < n;
    const int ii = live ? i : n - 1;      // idle lanes shadow the last facet with weight zero
    const int4 ra = rec[2 * (size_t)ii], rb = rec[2 * (size_t)ii + 1];
    const int v[4] = {ra.x, ra.y, ra.z, ra.w};
    const int opp[2] = {DIM == 2 ? ra.z : ra.w, DIM == 2 ? rb.z : rb.w};
    const double meas = live ? fmeas[item[ii]] : 0.0;
    double x[DIM][DIM];                   // the facet's vertices
#pragma unroll
    for (int a = 0; a < DIM; ++a)
#pragma unroll
        for (int c = 0; c < DIM; ++c) x[a][c] = coords[(size_t)v[a] * DIM + c];
    // G[s][b - 1] = grad(lambda_b), b = 1..DIM, on the cell of side s with the vertices (f_0, .., f_{DIM-1}, opposite); nrm = n_i
    double G[2][DIM][DIM], nrm[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) nrm[c] = 0.0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
            for (int c = 0; c < DIM; ++c) G[s][a][c] = 0.0;
        if (B.need & (s ? MF_GEOM_E : MF_GEOM_I)) {      // create refused flat cells then
            double xc[DIM + 1][DIM];
#pragma unroll
            for (int a = 0; a < DIM; ++a)
#pragma unroll
                for (int c = 0; c < DIM; ++c) xc[a][c] = x[a][c];
#pragma unroll
            for (int c = 0; c < DIM; ++c) xc[DIM][c] = coords[(size_t)opp[s] * DIM + c];
            SampleCell<DIM> T;
            T.setup(xc);
#pragma unroll
            for (int a = 0; a < DIM; ++a)
#pragma unroll
                for (int c = 0; c < DIM; ++c) G[s][a][c] = T.inv[a][c];
            if (s == 0) {
                double len = 0.0;
#pragma unroll
                for (int c = 0; c < DIM; ++c) len += G[0][DIM - 1][c] * G[0][DIM - 1][c];
                len = sqrt(len);
#pragma unroll
                for (int c = 0; c < DIM; ++c) nrm[c] = -G[0][DIM - 1][c] / len;
            }
        }
    }
    // values at the facet's vertices of the fields the program reads (0 elsewhere); a geometric slot keeps its one value in av[k][0]
    double kv[2][3][DIM], pv[DIM], av[KNP_MAX_AUX][DIM];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const bool ri = B.need & (FN_KI << j), re = B.need & (FN_KE << j);
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            kv[0][j][a] = ri ? f.ki[j][v[a]] : 0.0;
            kv[1][j][a] = re ? f.ke[j][v[a]] : 0.0;
        }
    }
#pragma unroll
    for (int a = 0; a < DIM; ++a) pv[a] = (B.need & FN_PHIM) ? f.phim[v[a]] : 0.0;
#pragma unroll
    for (int k = 0; k < KNP_MAX_AUX; ++k) {
        const bool r = B.need & (FN_AUX << k);
        const int m = B.mode[k];
        const bool field = r && m < MF_NORMAL;
#pragma unroll
        for (int a = 0; a < DIM; ++a) av[k][a] = field ? f.aux[k][v[a]] : 0.0;
        if (r && m >= MF_NORMAL) {
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                const double nc = nrm[c], keep = av[k][0];
                av[k][0] = m - MF_NORMAL == c ? nc : keep;
            }
        } else if (r && m >= 0) {
            const bool ext = (m >= 3 && m < MF_DN_I) || m == MF_DN_E;
            const int ax = m < 3 ? m : m - 3;      // the axis of the modes below MF_DN_I
            double w[DIM];                         // the direction: e_ax, n_i or n_e = -n_i
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                const double nc = nrm[c];
                w[c] = m == MF_DN_I ? nc : m == MF_DN_E ? -nc : ax == c ? 1.0 : 0.0;
            }
            const int oi = opp[0], oe = opp[1];
            const double fo = f.aux[k][ext ? oe : oi];
            const double f0 = av[k][0];
            double d = 0.0;      // sum_b grad(lambda_b) f_b with sum_b grad(lambda_b) = 0: differences first
#pragma unroll
            for (int b = 1; b <= DIM; ++b) {
                double g = 0.0;
#pragma unroll
                for (int c = 0; c < DIM; ++c) {
                    const double gi = G[0][b - 1][c], ge = G[1][b - 1][c];      // values, not a choice between two addresses
                    g += (ext ? ge : gi) * w[c];
                }
                const double fb = b < DIM ? av[k][b < DIM ? b : 0] : fo;
                d += g * (fb - f0);
            }
            av[k][0] = d;
        }
    }
    double* reg = dsmem + threadIdx.x;
    double acc[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) acc[j] = 0.0;
    for (int q = 0; q < n_q; ++q) {
        double lam[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) lam[a] = qp[q * DIM + a];
        double kiq[1][3], keq[1][3], phq[1] = {0.0}, auxq[1][KNP_MAX_AUX], xq[1][3], Iout[1][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double si = 0.0, se = 0.0;
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                si += lam[a] * kv[0][j][a];
                se += lam[a] * kv[1][j][a];
            }
            kiq[0][j] = si;
            keq[0][j] = se;
            Iout[0][j] = 0.0;
        }
#pragma unroll
        for (int a = 0; a < DIM; ++a) phq[0] += lam[a] * pv[a];
#pragma unroll
        for (int k = 0; k < KNP_MAX_AUX; ++k) {
            double t = 0.0;
#pragma unroll
            for (int a = 0; a < DIM; ++a) t += lam[a] * av[k][a];
            const double one = av[k][0];
            auxq[0][k] = B.mode[k] >= 0 ? one : t;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double t = 0.0;
            if (d < DIM) {
#pragma unroll
                for (int a = 0; a < DIM; ++a) t += lam[a] * x[a][d < DIM ? d : 0];
            }
            xq[0][d] = t;
        }
        run_program<1, FN_BT>(code, n_instr, sk, kiq, keq, phq, auxq, xq, Iout, reg);
        const double w = qw[q] * meas;
#pragma unroll
        for (int j = 0; j < NOUT; ++j) acc[j] += w * Iout[0][j];
    }
    DiagSum<NOUT> s;
#pragma unroll
    for (int j = 0; j < NOUT; ++j) s.v[j] = acc[j];
    diag_chunk_partials<DiagSum<NOUT>, FN_BT>(live ? key[i] : -1, live, i == n - 1, s, partial);
}

static void membrane_functional_free(KnpMembraneFunctional& P) {
    diag_map_free(P.map);
    dev_free(P.d_code); dev_free(P.d_qp); dev_free(P.d_qw); dev_free(P.d_rec);
    P = KnpMembraneFunctional();
}
void knp_membrane_functional_free(knp_ctx* ctx) {
    for (auto& P : ctx->membrane_functionals) membrane_functional_free(P);
    ctx->membrane_functionals.clear();
}

static int membrane_functional_of(knp_ctx* ctx, int32_t id) {
    if (id < 0 || id >= (int)ctx->membrane_functionals.size() || !ctx->membrane_functionals[(size_t)id].live) {
        ctx->err = "unknown membrane functional " + std::to_string(id);
        return KNP_E_ARG;
    }
    return KNP_OK;
}

// the records of k_membrane_functional for the facets of a map, in map order; counts the facets whose extracellular cell does not hold
// them (when ext) and those with a flat or non-finite adjacent cell among the cells the bound modes read
template <int DIM>
static void membrane_functional_records(const KnpHostGraph& g, const std::vector<double>& coords, const int32_t* facets, int n, bool geom_i,
                                        bool geom_e, std::vector<int32_t>& rec, int64_t& n_open, int64_t& n_flat) {
    rec.assign((size_t)n * 8, 0);
    int64_t open = 0, flat = 0;
#pragma omp parallel for schedule(static) reduction(+ : open, flat) num_threads(knp_host_threads())
    for (int i = 0; i < n; ++i) {
        const int F = facets[i];
        int32_t* r = &rec[(size_t)i * 8];
        const int32_t f0 = g.fv[(size_t)F * DIM];
        for (int s = 0; s < 2; ++s) {
            for (int b = 0; b < 4; ++b) r[4 * s + b] = b < DIM ? g.fv[(size_t)F * DIM + b] : f0;
            const int32_t o = g.gopp[(size_t)2 * F + s];
            r[4 * s + DIM] = o >= 0 ? o : f0;
            if (!(s ? geom_e : geom_i)) continue;
            if (o < 0) { ++open; continue; }
            double x[DIM + 1][3], G[DIM + 1][3];
            for (int a = 0; a <= DIM; ++a)
                for (int c = 0; c < DIM; ++c) x[a][c] = coords[(size_t)r[4 * s + a] * DIM + c];
            bool ok = simplex_gradients<DIM>(x, G);
            double len = 0.0;
            for (int c = 0; c < DIM && ok; ++c) len += G[DIM][c] * G[DIM][c];
            ok = ok && std::isfinite(1.0 / std::sqrt(len));
            for (int a = 0; a <= DIM && ok; ++a)
                for (int c = 0; c < DIM; ++c) ok = ok && std::isfinite(G[a][c]);
            if (!ok) ++flat;
        }
    }
    n_open = open;
    n_flat = flat;
}

template <int DIM, int NOUT>
static void membrane_functional_launch(knp_ctx* ctx, const KnpMembraneFunctional& P, const FieldPtrs& f, const MfBind& B, const DiagConsts& K,
                                       size_t lds) {
    const KnpDiagMap& m = P.map;
    hipLaunchKernelGGL((k_membrane_functional<DIM, NOUT>), dim3(m.n_chunks), dim3(FN_BT), lds, ctx->stream, m.n, m.d_item, m.d_key,
                       reinterpret_cast<const int4*>(P.d_rec), ctx->d_fmeas, ctx->d_coords, P.n_q, P.d_qp, P.d_qw, f, B, P.d_code, P.n_instr, K,
                       P.n_consts, m.d_partial);
}

extern "C" {

int knp_membrane_functional_create(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr, const int32_t* facets, int32_t n_q,
                                   const double* q_pts, const double* q_w, int32_t n_instr, const int32_t* code, int32_t n_consts,
                                   const double* consts, int32_t n_aux, const int32_t* aux_mode, int32_t n_out, int32_t* id) {
    CHECK_CTX(ctx);
    const KnpHostGraph& g = ctx->g;
    if (!id || !q_pts || !q_w || !code || (n_consts > 0 && !consts) || (n_aux > 0 && !aux_mode)) { ctx->err = "membrane functional: null argument"; return KNP_E_ARG; }
    if (n_q < 1 || n_q > KNP_FUNCTIONAL_MAX_Q) { ctx->err = "membrane functional: n_q must be 1.." + std::to_string(KNP_FUNCTIONAL_MAX_Q); return KNP_E_ARG; }
    if (n_out < 1 || n_out > 3) { ctx->err = "membrane functional: n_out must be 1..3"; return KNP_E_ARG; }
    if (n_aux < 0 || n_aux > KNP_MAX_AUX) { ctx->err = "membrane functional: n_aux must be 0.." + std::to_string(KNP_MAX_AUX); return KNP_E_ARG; }
    if (n_instr < 1) { ctx->err = "membrane functional: empty program"; return KNP_E_ARG; }
    if (n_consts < 0 || n_consts > KNP_DIAG_MAX_CONSTS) { ctx->err = "membrane functional: at most " + std::to_string(KNP_DIAG_MAX_CONSTS) + " constants"; return KNP_E_ARG; }
    MfBind B;
    B.need = 0;
    for (int k = 0; k < KNP_MAX_AUX; ++k) {
        B.mode[k] = -1;
        if (k >= n_aux) continue;
        const int m = aux_mode[k];
        const int axis = m >= MF_NORMAL ? m - MF_NORMAL : m >= 3 && m < MF_DN_I ? m - 3 : m < 3 ? m : 0;
        if (m < -1 || m > MF_NORMAL + 2 || axis >= g.dim) {
            ctx->err = "membrane functional: aux_mode must be -1 (value), a / 3 + a (d/dx_a on the intra / extracellular cell), 6 / 7 (d/dn) or 8 + a "
                       "(normal component) with an axis a below the mesh's dimension";
            return KNP_E_ARG;
        }
        B.mode[k] = (int8_t)m;
    }
    int n_regs = 0;
    KCHK(validate_program(ctx, n_instr, code, n_consts, &n_regs));
    for (int i = 0; i < n_instr; ++i) {       // which slots the code reads; the indices are validate_program's
        const int op = code[4 * i], a = code[4 * i + 2];
        if (op == KNP_OP_KI) B.need |= FN_KI << a;
        else if (op == KNP_OP_KE) B.need |= FN_KE << a;
        else if (op == KNP_OP_PHIM) B.need |= FN_PHIM;
        else if (op == KNP_OP_AUX) {
            if (a >= n_aux) { ctx->err = "membrane functional: instruction " + std::to_string(i) + " reads aux slot " + std::to_string(a) + " of " + std::to_string(n_aux); return KNP_E_ARG; }
            B.need |= FN_AUX << a;
            if (mf_mode_int(B.mode[a])) B.need |= MF_GEOM_I;
            if (mf_mode_ext(B.mode[a])) B.need |= MF_GEOM_E;
        } else if (op == KNP_OP_OUT && a >= n_out) {
            ctx->err = "membrane functional: instruction " + std::to_string(i) + " writes output " + std::to_string(a) + " of " + std::to_string(n_out);
            return KNP_E_ARG;
        }
    }
    KnpMembraneFunctional P;
    KCHK(diag_map_set(ctx, P.map, n_tags, seg_ptr, facets, g.n_g, FN_BT, n_out, FN_WAVE_CHUNKS, "membrane functional facet map"));
    const int rc = [&]() -> int {
        std::vector<double> hx;
        if ((B.need & (MF_GEOM_I | MF_GEOM_E)) && P.map.n > 0) {
            hx.resize((size_t)g.n_v * g.dim);
            HIPCHK(hipMemcpy(hx.data(), ctx->d_coords, hx.size() * sizeof(double), hipMemcpyDeviceToHost));
        }
        std::vector<int32_t> rec;
        int64_t n_open = 0, n_flat = 0;
        by_dim(g.dim, [&](auto D) {
            membrane_functional_records<D()>(g, hx, facets, P.map.n, B.need & MF_GEOM_I, B.need & MF_GEOM_E, rec, n_open, n_flat);
        });
        if (n_open) { ctx->err = "membrane functional: a slot reads the extracellular cell and a listed facet has an extracellular cell that does not hold it"; return KNP_E_MESH; }
        if (n_flat) { ctx->err = "membrane functional: a gradient or the normal is bound and a listed facet has a flat adjacent cell"; return KNP_E_MESH; }
        if (!rec.empty()) KCHK(dev_upload(ctx, &P.d_rec, rec));
        KCHK(dev_upload_raw(ctx, &P.d_code, code, (size_t)4 * n_instr));
        KCHK(dev_upload_raw(ctx, &P.d_qp, q_pts, (size_t)n_q * g.dim));
        KCHK(dev_upload_raw(ctx, &P.d_qw, q_w, (size_t)n_q));
        return KNP_OK;
    }();
    if (rc != KNP_OK) {
        membrane_functional_free(P);
        return rc;
    }
    P.n_q = n_q; P.n_out = n_out; P.n_instr = n_instr; P.n_regs = n_regs; P.n_consts = n_consts;
    P.need = B.need;
    for (int k = 0; k < KNP_MAX_AUX; ++k) P.aux_mode[k] = B.mode[k];
    for (int i = 0; i < n_consts; ++i) P.consts[i] = consts[i];
    P.live = true;
    size_t slot = 0;
    while (slot < ctx->membrane_functionals.size() && ctx->membrane_functionals[slot].live) ++slot;
    if (slot == ctx->membrane_functionals.size()) ctx->membrane_functionals.emplace_back();
    ctx->membrane_functionals[slot] = P;
    *id = (int32_t)slot;
    return KNP_OK;
}

int knp_membrane_functional_set_constants(knp_ctx* ctx, int32_t id, int32_t n_consts, const double* consts) {
    CHECK_CTX(ctx);
    KCHK(membrane_functional_of(ctx, id));
    KnpMembraneFunctional& P = ctx->membrane_functionals[(size_t)id];
    if (n_consts != P.n_consts || (n_consts && !consts)) { ctx->err = "membrane functional: constant count mismatch"; return KNP_E_ARG; }
    for (int i = 0; i < n_consts; ++i) P.consts[i] = consts[i];   // kernel arguments of the next launch: nothing to copy
    return KNP_OK;
}

int knp_membrane_functional_eval(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out) {
    CHECK_CTX(ctx);
    KCHK(membrane_functional_of(ctx, id));
    const KnpMembraneFunctional& P = ctx->membrane_functionals[(size_t)id];
    const KnpDiagMap& m = P.map;
    if (m.n_tags == 0) return KNP_OK;
    if (!fields || !out) { ctx->err = "membrane functional: null fields or null output buffer"; return KNP_E_ARG; }
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
        const bool reads = (P.need & (FN_AUX << k)) && P.aux_mode[k] < MF_NORMAL;      // a normal component has no field
        f.aux[k] = reads ? fields->aux[k] : nullptr;
        missing = missing || (reads && !f.aux[k]);
    }
    if (missing) { ctx->err = "membrane functional: a field the program reads is null"; return KNP_E_ARG; }
    if (m.n > 0) {
        MfBind B;
        B.need = P.need;
        for (int k = 0; k < KNP_MAX_AUX; ++k) B.mode[k] = P.aux_mode[k];
        DiagConsts K;
        for (int i = 0; i < KNP_DIAG_MAX_CONSTS; ++i) K.v[i] = i < P.n_consts ? P.consts[i] : 0.0;
        const size_t lds = (size_t)std::max(P.n_regs, 1) * FN_BT * sizeof(double);   // <= 48 registers: 48 KiB
        by_dim(ctx->g.dim, [&](auto D) {
            if (P.n_out == 1) membrane_functional_launch<D(), 1>(ctx, P, f, B, K, lds);
            else if (P.n_out == 2) membrane_functional_launch<D(), 2>(ctx, P, f, B, K, lds);
            else membrane_functional_launch<D(), 3>(ctx, P, f, B, K, lds);
        });
        HIPCHK(hipGetLastError());
    }
    if (P.n_out == 1) return diag_combine<DiagSum<1>>(ctx, m, out);
    if (P.n_out == 2) return diag_combine<DiagSum<2>>(ctx, m, out);
    return diag_combine<DiagSum<3>>(ctx, m, out);
}

int knp_membrane_functional_destroy(knp_ctx* ctx, int32_t id) {
    CHECK_CTX(ctx);
    KCHK(membrane_functional_of(ctx, id));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // an evaluation in flight may still read the plan
    membrane_functional_free(ctx->membrane_functionals[(size_t)id]);
    return KNP_OK;
}

}  // extern "C"
