// Membrane functionals (knp_membrane_functional_*): per-tag integrals over membrane facets of a bytecode program evaluated at the
// points of a facet quadrature rule -- assemble_scalar(<expression> * dS(tag)) with one-sided gradients ('+' / '-' restrictions), the
// facet normal and normal derivatives.  Included at the end of knp_kernels.hip, after knp_functional.inc, from which it takes the plan
// (KnpFunctional, FnBind, the FN_* bits, FN_BT), the kernel's shared parts (fn_lane, fn_load_fields, fn_integrate) and the plan's life
// (fn_create, fn_set_constants, fn_eval, fn_destroy); like that file it uses by_dim, simplex_gradients and SampleCell.
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
//                  grad(lambda_b) . n: differences first, a field's constant offset cancels exactly.  The quadrature loop with the
//                  measure |F| and the per-tag reduction are fn_integrate.

// bits of FnBind::need above the field bits of knp_functional.inc: the cells whose geometry some slot the code reads needs
static constexpr unsigned MF_GEOM_I = 1u << 15, MF_GEOM_E = 1u << 16;
static constexpr int MF_DN_I = 6, MF_DN_E = 7, MF_NORMAL = FN_NORMAL;      // slot modes besides -1 (value), a (d/dx_a, '+' cell), 3 + a ('-' cell)
static inline bool mf_mode_ext(int m) { return (m >= 3 && m < MF_DN_I) || m == MF_DN_E; }            // reads the extracellular cell
static inline bool mf_mode_int(int m) { return (m >= 0 && m < 3) || m == MF_DN_I || m == MF_DN_E || m >= MF_NORMAL; }   // the normal is the intracellular cell's

template <int DIM, int NOUT, FnEnd END = FN_TAGS, bool FUNCS = false>
__global__ void __launch_bounds__(FN_BT) k_membrane_functional(int n, const int32_t* __restrict__ item, const int32_t* __restrict__ key,
                                                               const int4* __restrict__ rec, const double* __restrict__ fmeas,
                                                               const double* __restrict__ coords, int n_q, const double* __restrict__ qp,
                                                               const double* __restrict__ qw, FieldPtrs f, FnBind B,
                                                               const int32_t* __restrict__ code, int n_instr, DiagConsts K, int n_consts,
                                                               double* __restrict__ partial) {
    const FnLane L = fn_lane(n, K, n_consts);
    const int4 ra = rec[2 * (size_t)L.ii], rb = rec[2 * (size_t)L.ii + 1];
    const int v[4] = {ra.x, ra.y, ra.z, ra.w};
    const int opp[2] = {DIM == 2 ? ra.z : ra.w, DIM == 2 ? rb.z : rb.w};
    const double meas = L.live ? fmeas[item[L.ii]] : 0.0;
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
    FnValues<DIM> U;
    fn_load_fields<DIM>(f, B, v, U);
#pragma unroll
    for (int k = 0; k < KNP_MAX_AUX; ++k) {      // the slots of one value per facet
        const bool r = B.need & (FN_AUX << k);
        const int m = B.mode[k];
        if (r && m >= MF_NORMAL) {
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                const double nc = nrm[c], keep = U.av[k][0];
                U.av[k][0] = m - MF_NORMAL == c ? nc : keep;
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
            const double f0 = U.av[k][0];
            double d = 0.0;      // sum_b grad(lambda_b) f_b with sum_b grad(lambda_b) = 0: differences first
#pragma unroll
            for (int b = 1; b <= DIM; ++b) {
                double g = 0.0;
#pragma unroll
                for (int c = 0; c < DIM; ++c) {
                    const double gi = G[0][b - 1][c], ge = G[1][b - 1][c];      // values, not a choice between two addresses
                    g += (ext ? ge : gi) * w[c];
                }
                const double fb = b < DIM ? U.av[k][b < DIM ? b : 0] : fo;
                d += g * (fb - f0);
            }
            U.av[k][0] = d;
        }
    }
    fn_integrate<DIM, DIM, NOUT, END, FUNCS>(L, n, key, U, x, B, n_q, qp, qw, meas, code, n_instr, partial);
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

// the membrane kind's launch, of either end (fn_eval)
template <FnEnd END>
static int membrane_functional_eval(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out) {
    return fn_eval<END>(ctx, fn_membrane(ctx), id, fields, out,
                          [&](auto D, auto NOUT, auto I, auto M, const KnpFunctional& P, const FieldPtrs& f, const FnBind& B, const DiagConsts& K,
                              size_t lds, double* dst) {
                              const KnpDiagMap& m = P.map;
                              hipLaunchKernelGGL((k_membrane_functional<D(), NOUT(), I(), M()>), dim3(m.n_chunks), dim3(FN_BT), lds, ctx->stream, m.n,
                                                 m.d_item, m.d_key, reinterpret_cast<const int4*>(P.d_rec), ctx->d_fmeas, ctx->d_coords, P.n_q,
                                                 P.d_qp, P.d_qw, f, B, P.d_code, P.n_instr, K, P.n_consts, dst);
                          });
}

extern "C" {

int knp_membrane_functional_create(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr, const int32_t* facets, int32_t n_q,
                                   const double* q_pts, const double* q_w, int32_t n_instr, const int32_t* code, int32_t n_consts,
                                   const double* consts, int32_t n_aux, const int32_t* aux_mode, int32_t n_out, int32_t* id) {
    CHECK_CTX(ctx);
    const KnpHostGraph& g = ctx->g;
    const FnCreateArgs a = {n_tags, seg_ptr, facets, n_q, q_pts, q_w, n_instr, code, n_consts, consts, n_aux, aux_mode, n_out, id};
    return fn_create(
        ctx, fn_membrane(ctx), a, g.n_g, g.dim, "membrane functional facet map",
        "aux_mode must be -1 (value), a / 3 + a (d/dx_a on the intra / extracellular cell), 6 / 7 (d/dn) or 8 + a "
        "(normal component) with an axis a below the mesh's dimension",
        [&](int m) {
            const int axis = m >= MF_NORMAL ? m - MF_NORMAL : m >= 3 && m < MF_DN_I ? m - 3 : m < 3 ? m : 0;
            return m >= -1 && m <= MF_NORMAL + 2 && axis < g.dim;
        },
        [](int m) { return (mf_mode_int(m) ? MF_GEOM_I : 0u) | (mf_mode_ext(m) ? MF_GEOM_E : 0u); },
        [&](KnpFunctional& P) -> int {
            std::vector<double> hx;
            if ((P.need & (MF_GEOM_I | MF_GEOM_E)) && P.map.n > 0) {
                hx.resize((size_t)g.n_v * g.dim);
                HIPCHK(hipMemcpy(hx.data(), ctx->d_coords, hx.size() * sizeof(double), hipMemcpyDeviceToHost));
            }
            std::vector<int32_t> rec;
            int64_t n_open = 0, n_flat = 0;
            by_dim(g.dim, [&](auto D) {
                membrane_functional_records<D()>(g, hx, facets, P.map.n, P.need & MF_GEOM_I, P.need & MF_GEOM_E, rec, n_open, n_flat);
            });
            if (n_open) { ctx->err = "membrane functional: a slot reads the extracellular cell and a listed facet has an extracellular cell that does not hold it"; return KNP_E_MESH; }
            if (n_flat) { ctx->err = "membrane functional: a gradient or the normal is bound and a listed facet has a flat adjacent cell"; return KNP_E_MESH; }
            if (!rec.empty()) KCHK(dev_upload(ctx, &P.d_rec, rec));
            return KNP_OK;
        });
}

int knp_membrane_functional_set_constants(knp_ctx* ctx, int32_t id, int32_t n_consts, const double* consts) {
    CHECK_CTX(ctx);
    return fn_set_constants(ctx, fn_membrane(ctx), id, n_consts, consts);
}

int knp_membrane_functional_eval(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out) {
    CHECK_CTX(ctx);
    return membrane_functional_eval<FN_TAGS>(ctx, id, fields, out);
}

int knp_membrane_functional_destroy(knp_ctx* ctx, int32_t id) {
    CHECK_CTX(ctx);
    return fn_destroy(ctx, fn_membrane(ctx), id);
}

}  // extern "C"
