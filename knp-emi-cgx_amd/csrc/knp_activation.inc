// Activation map (knp_activation_*, knp_diag_activation): when each membrane vertex fired, how high phi_m peaked there, when it
// repolarised, and how fast the front travelled over each membrane facet.  Included after knp_diagnostics.inc, whose per-tag
// reduction (DiagActivation, diag_chunk_partials, diag_combine, diag_map_set) the summary uses.
//
// The detector keeps no state in the library: v_last [n], state [ACT_ROWS][n] (structure of arrays) and count [n] belong to the
// caller and come by pointer.  One lane per listed vertex; a launch reads 4 + 8 bytes (index, phi_m) and reads and writes
// 8 + 56 + 4 bytes of state per vertex.  All comparisons are plain IEEE: a NaN phi_m fails every one of them, so it records nothing
// in the interval that ends at it nor (as v_last) in the next one, and leaves no false crossing.
enum { ACT_T_FIRST = 0, ACT_T_LAST_UP, ACT_T_REPOL, ACT_V_PEAK, ACT_T_PEAK, ACT_DVDT_MAX, ACT_T_DVDT, ACT_ROWS };

// phi_m at a listed vertex; an index outside the mesh reads as NaN (the list is device data nobody has validated)
__device__ __forceinline__ double act_value(const double* __restrict__ phim, int v, int n_v) {
    return (unsigned)v < (unsigned)n_v ? phim[v] : __builtin_nan("");
}

__global__ void __launch_bounds__(NT) k_activation_arm(int n, int n_v, const int32_t* __restrict__ vertex, const double* __restrict__ phim,
                                                       double t, double* __restrict__ v_last, double* __restrict__ state,
                                                       int32_t* __restrict__ count) {
    const int j = blockIdx.x * NT + threadIdx.x;
    if (j >= n) return;
    const double ph = act_value(phim, vertex[j], n_v);
    const double nan = __builtin_nan("");
    v_last[j] = ph;
    state[(size_t)ACT_T_FIRST * n + j] = nan;
    state[(size_t)ACT_T_LAST_UP * n + j] = nan;
    state[(size_t)ACT_T_REPOL * n + j] = nan;
    state[(size_t)ACT_V_PEAK * n + j] = ph;
    state[(size_t)ACT_T_PEAK * n + j] = t;
    state[(size_t)ACT_DVDT_MAX * n + j] = -HUGE_VAL;
    state[(size_t)ACT_T_DVDT * n + j] = nan;
    count[j] = 0;
}

__global__ void __launch_bounds__(NT) k_activation_step(int n, int n_v, const int32_t* __restrict__ vertex, const double* __restrict__ phim,
                                                        double t0, double t1, double thr_up, double thr_down, double* __restrict__ v_last,
                                                        double* __restrict__ state, int32_t* __restrict__ count) {
    const int j = blockIdx.x * NT + threadIdx.x;
    if (j >= n) return;
    const double v0 = v_last[j], v1 = act_value(phim, vertex[j], n_v), h = t1 - t0;
    int c = count[j];
    // 1. upward crossing: the rule of diagnostics.threshold_crossings
    if (v0 < thr_up && v1 >= thr_up) {
        const double tx = t0 + (thr_up - v0) / (v1 - v0) * h;
        c += 1;
        count[j] = c;
        if (c == 1) state[(size_t)ACT_T_FIRST * n + j] = tx;
        state[(size_t)ACT_T_LAST_UP * n + j] = tx;
    }
    // 2. repolarisation: the first downward crossing after an upward one (v0 > v1 here and v0 < v1 above: never both)
    if (c > 0 && v0 >= thr_down && v1 < thr_down) {
        double* tr = state + (size_t)ACT_T_REPOL * n + j;
        if (isnan(*tr)) *tr = t0 + (v0 - thr_down) / (v0 - v1) * h;
    }
    // 3. peak: strict, the first of equal maxima stays
    if (v1 > state[(size_t)ACT_V_PEAK * n + j]) {
        state[(size_t)ACT_V_PEAK * n + j] = v1;
        state[(size_t)ACT_T_PEAK * n + j] = t1;
    }
    // 4. steepest upstroke
    const double s = (v1 - v0) / h;
    if (s > state[(size_t)ACT_DVDT_MAX * n + j]) {
        state[(size_t)ACT_DVDT_MAX * n + j] = s;
        state[(size_t)ACT_T_DVDT * n + j] = t0 + 0.5 * h;
    }
    v_last[j] = v1;
}

// Velocity of the front over one membrane facet from the nodal activation time T: the surface gradient g of T's P1 interpolant,
// speed = 1 / |g|, direction = g / |g|.  Valid iff every T of the facet is finite and |g|^2 is positive and finite (a facet of
// measure zero is not); what is returned besides:
// the smallest and largest T over the facet's vertices (fmin / fmax: NaN dropped) and the number of its vertices with a finite T.
template <int DIM>
struct FacetFront {
    bool valid;
    double speed, dir[DIM], t_min, t_max;
    int n_finite;
};
template <int DIM>
__device__ __forceinline__ FacetFront<DIM> facet_front(const int32_t* __restrict__ fv, const double* __restrict__ coords,
                                                       const double* __restrict__ T, int g, int n_v) {
    FacetFront<DIM> r;
    int v[DIM];
    double x[DIM][DIM], tt[DIM];
    bool fin = true, in = true;
    r.t_min = HUGE_VAL;
    r.t_max = -HUGE_VAL;
    r.n_finite = 0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        v[a] = fv[(size_t)g * DIM + a];
        in = in && (unsigned)v[a] < (unsigned)n_v;
    }
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        tt[a] = in ? T[v[a]] : __builtin_nan("");
#pragma unroll
        for (int c = 0; c < DIM; ++c) x[a][c] = in ? coords[(size_t)v[a] * DIM + c] : 0.0;
        const bool f = isfinite(tt[a]);
        fin = fin && f;
        r.n_finite += f ? 1 : 0;
        r.t_min = fmin(r.t_min, tt[a]);
        r.t_max = fmax(r.t_max, tt[a]);
    }
    if constexpr (DIM == 2) {
        const double e0 = x[1][0] - x[0][0], e1 = x[1][1] - x[0][1];
        const double L = sqrt(e0 * e0 + e1 * e1), d = tt[1] - tt[0];
        r.valid = fin && d != 0.0 && L > 0.0;
        const double sg = d > 0.0 ? 1.0 : -1.0;
        r.speed = L / fabs(d);
        r.dir[0] = sg * e0 / L;
        r.dir[1] = sg * e1 / L;
    } else {
        double e1[3], e2[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            e1[c] = x[1][c] - x[0][c];
            e2[c] = x[2][c] - x[0][c];
        }
        const double a = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2];
        const double b = e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2];
        const double c = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
        const double det = a * c - b * b;
        const double d1 = tt[1] - tt[0], d2 = tt[2] - tt[0];
        const double gg = (c * d1 * d1 - 2.0 * b * d1 * d2 + a * d2 * d2) / det;
        r.valid = fin && gg > 0.0 && isfinite(gg);      // a flat triangle (det == 0) has no gradient either
        const double len = sqrt(gg), w1 = (c * d1 - b * d2) / det, w2 = (a * d2 - b * d1) / det;
        r.speed = 1.0 / len;
#pragma unroll
        for (int k = 0; k < DIM; ++k) r.dir[k] = (w1 * e1[k] + w2 * e2[k]) / len;
    }
    return r;
}

// out[(1 + DIM) i] = speed, then the unit direction, of the i-th listed facet; NaN in every slot of an invalid facet (and of a listed
// index outside the mesh's membrane facets)
template <int DIM>
__global__ void __launch_bounds__(NT) k_activation_velocity(int n, int n_g, int n_v, const int32_t* __restrict__ facets,
                                                            const int32_t* __restrict__ fv, const double* __restrict__ coords,
                                                            const double* __restrict__ T, double* __restrict__ out) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int g = facets[i];
    const double nan = __builtin_nan("");
    double* o = out + (size_t)i * (1 + DIM);
    bool ok = (unsigned)g < (unsigned)n_g;
    FacetFront<DIM> r;
    if (ok) {
        r = facet_front<DIM>(fv, coords, T, g, n_v);
        ok = r.valid;
    }
    o[0] = ok ? r.speed : nan;
#pragma unroll
    for (int k = 0; k < DIM; ++k) o[1 + k] = ok ? r.dir[k] : nan;
}

// per tag: (sum |F| [valid], sum |F| speed [valid], min T, max T, sum |F|/d #{vertices of F with a finite T}) over the map's facets.
// The shape of k_diag_phim: one facet per lane, DIAG_BT per block, DiagActivation's reduction; idle lanes carry its identity.
template <int DIM>
__global__ void __launch_bounds__(DIAG_BT) k_diag_activation(int n, int n_v, const int32_t* __restrict__ item, const int32_t* __restrict__ key,
                                                             const int32_t* __restrict__ fv, const double* __restrict__ fmeas,
                                                             const double* __restrict__ coords, const double* __restrict__ T,
                                                             double* __restrict__ partial) {
    const int i = blockIdx.x * DIAG_BT + threadIdx.x;
    const bool live = i < n;
    DiagActivation v = DiagActivation::identity();
    int k = -1;
    if (live) {
        k = key[i];
        const int g = item[i];                  // validated by diag_map_set: in [0, n_g)
        const FacetFront<DIM> r = facet_front<DIM>(fv, coords, T, g, n_v);
        const double meas = fmeas[g];
        v.v[0] = r.valid ? meas : 0.0;
        v.v[1] = r.valid ? meas * r.speed : 0.0;
        v.v[2] = r.t_min;
        v.v[3] = r.t_max;
        v.v[4] = meas * (1.0 / DIM) * r.n_finite;
    }
    diag_chunk_partials<DiagActivation, DIAG_BT>(k, live, i == n - 1, v, partial);
}

extern "C" {

int knp_activation_arm(knp_ctx* ctx, int32_t n, const int32_t* vertex, const double* phi_m, double t, double* v_last, double* state,
                       int32_t* count) {
    CHECK_CTX(ctx);
    if (n < 0) { ctx->err = "knp_activation_arm: negative vertex count"; return KNP_E_ARG; }
    if (!vertex || !phi_m || !v_last || !state || !count) { ctx->err = "knp_activation_arm: null pointer"; return KNP_E_ARG; }
    if (n == 0) return KNP_OK;
    hipLaunchKernelGGL(k_activation_arm, dim3((n + NT - 1) / NT), dim3(NT), 0, ctx->stream, n, ctx->g.n_v, vertex, phi_m, t, v_last, state, count);
    HIPCHK(hipGetLastError());
    return KNP_OK;
}

int knp_activation_step(knp_ctx* ctx, int32_t n, const int32_t* vertex, const double* phi_m, double t0, double t1, double thr_up,
                        double thr_down, double* v_last, double* state, int32_t* count) {
    CHECK_CTX(ctx);
    if (n < 0) { ctx->err = "knp_activation_step: negative vertex count"; return KNP_E_ARG; }
    if (!vertex || !phi_m || !v_last || !state || !count) { ctx->err = "knp_activation_step: null pointer"; return KNP_E_ARG; }
    if (!(t1 > t0) || !std::isfinite(t0) || !std::isfinite(t1)) { ctx->err = "knp_activation_step: t1 must be later than t0"; return KNP_E_ARG; }
    if (!std::isfinite(thr_up) || !std::isfinite(thr_down)) { ctx->err = "knp_activation_step: non-finite threshold"; return KNP_E_ARG; }
    if (n == 0) return KNP_OK;
    hipLaunchKernelGGL(k_activation_step, dim3((n + NT - 1) / NT), dim3(NT), 0, ctx->stream, n, ctx->g.n_v, vertex, phi_m, t0, t1, thr_up,
                       thr_down, v_last, state, count);
    HIPCHK(hipGetLastError());
    return KNP_OK;
}

int knp_activation_velocity(knp_ctx* ctx, int32_t n_facets, const int32_t* facets, const double* T, double* out) {
    CHECK_CTX(ctx);
    if (n_facets < 0) { ctx->err = "knp_activation_velocity: negative facet count"; return KNP_E_ARG; }
    if (!facets || !T || !out) { ctx->err = "knp_activation_velocity: null pointer"; return KNP_E_ARG; }
    if (n_facets == 0) return KNP_OK;
    const KnpHostGraph& g = ctx->g;
    by_dim(g.dim, [&](auto D) {
        hipLaunchKernelGGL(k_activation_velocity<D()>, dim3((n_facets + NT - 1) / NT), dim3(NT), 0, ctx->stream, n_facets, g.n_g, g.n_v, facets,
                           ctx->d_fv, ctx->d_coords, T, out);
    });
    HIPCHK(hipGetLastError());
    return KNP_OK;
}

int knp_diag_set_activation_facets(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr, const int32_t* facets) {
    CHECK_CTX(ctx);
    return diag_map_set(ctx, ctx->diag_act, n_tags, seg_ptr, facets, ctx->g.n_g, DIAG_BT, DiagActivation::N, PHIM_WAVE_CHUNKS,
                        "activation facet map");
}

int knp_diag_activation(knp_ctx* ctx, const double* T, double* out) {
    CHECK_CTX(ctx);
    if (!T) { ctx->err = "null activation-time field"; return KNP_E_ARG; }
    const KnpDiagMap& m = ctx->diag_act;
    KCHK(diag_check(ctx, out, m.d_ptr, "no activation facet map (knp_diag_set_activation_facets)"));
    if (m.n > 0) {
        by_dim(ctx->g.dim, [&](auto D) {
            hipLaunchKernelGGL(k_diag_activation<D()>, dim3(m.n_chunks), dim3(DIAG_BT), 0, ctx->stream, m.n, ctx->g.n_v, m.d_item, m.d_key,
                               ctx->d_fv, ctx->d_fmeas, ctx->d_coords, T, m.d_partial);
        });
        HIPCHK(hipGetLastError());
    }
    return diag_combine<DiagActivation>(ctx, m, out);
}

}  // extern "C"
