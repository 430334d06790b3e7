// Diagnostics (knp_diag_*): per-tag volume integrals of the ion fields, per-tag membrane integrals of one bytecode program and
// per-tag trans-membrane ion fluxes, and per-tag integral, minimum and maximum of the membrane potential.
// Included at the end of knp_kernels.hip, after the host helpers (dev_upload, check_fields, validate_program) it uses.
//
// All of them reduce per tag without floating-point atomics.  The items (owned cells / selected membrane facets) are sorted by
// their dense tag index on the host, once; a block takes a fixed-size chunk of consecutive items, sums each run of equal tags inside
// the chunk with a segmented scan in LDS and stores one partial per (chunk, tag) pair at index tag + chunk (unique: consecutive
// chunks share at most their boundary tag).  A second pass folds a tag's partials in a fixed order (k_diag_combine, and for the long
// tags of a map that asks for it k_diag_combine_long).  The work split depends on the item count only, never on how the items fall
// into tags, and the result is the same bits on every run.

// What a reduction reduces: N doubles per item, the operator op(left, right) and its identity.  The scan and the combines below
// are written once, for any such type.
template <int NV>
struct DiagSum {          // NV sums
    static constexpr int N = NV;
    double v[NV];
    __device__ static DiagSum identity() {
        DiagSum r;
#pragma unroll
        for (int j = 0; j < NV; ++j) r.v[j] = 0.0;
        return r;
    }
    __device__ static DiagSum op(const DiagSum& a, const DiagSum& b) {
        DiagSum r;
#pragma unroll
        for (int j = 0; j < NV; ++j) r.v[j] = a.v[j] + b.v[j];
        return r;
    }
};
struct DiagPhim {         // (integral, minimum, maximum) of phi_m
    static constexpr int N = 3;
    double v[3];
    __device__ static DiagPhim identity() { return {{0.0, HUGE_VAL, -HUGE_VAL}}; }
    // fmin / fmax drop a NaN: a NaN phi_m shows in the integral, not in the minimum and maximum (stated in the ABI comment)
    __device__ static DiagPhim op(const DiagPhim& a, const DiagPhim& b) { return {{a.v[0] + b.v[0], fmin(a.v[1], b.v[1]), fmax(a.v[2], b.v[2])}}; }
};
struct DiagActivation {   // (valid area, area x speed, first and last activation time, activated area) of k_diag_activation (knp_activation.inc)
    static constexpr int N = 5;
    double v[5];
    __device__ static DiagActivation identity() { return {{0.0, 0.0, HUGE_VAL, -HUGE_VAL, 0.0}}; }
    // fmin / fmax drop a NaN: a vertex that never fired does not enter the first and last times
    __device__ static DiagActivation op(const DiagActivation& a, const DiagActivation& b) {
        return {{a.v[0] + b.v[0], a.v[1] + b.v[1], fmin(a.v[2], b.v[2]), fmax(a.v[3], b.v[3]), a.v[4] + b.v[4]}};
    }
};

// One partial per run of equal keys inside the block's chunk (keys ascending over the live threads, which form a prefix).
template <class V, int BT>
__device__ __forceinline__ void diag_chunk_partials(int key, bool live, bool last_item, V v, double* __restrict__ partial) {
    __shared__ int skey[BT];
    __shared__ double sv[V::N][BT];
    const int t = threadIdx.x;
    if (!live) v = V::identity();
    skey[t] = live ? key : -1;
#pragma unroll
    for (int j = 0; j < V::N; ++j) sv[j][t] = v.v[j];
    __syncthreads();
    for (int d = 1; d < BT; d <<= 1) {      // inclusive segmented scan, fixed order: v = left (op) v
        const bool same = t >= d && skey[t - d] == skey[t];
        V left = V::identity();
#pragma unroll
        for (int j = 0; j < V::N; ++j) left.v[j] = same ? sv[j][t - d] : left.v[j];
        __syncthreads();
        v = V::op(left, v);
#pragma unroll
        for (int j = 0; j < V::N; ++j) sv[j][t] = v.v[j];
        __syncthreads();
    }
    if (live && (last_item || t == BT - 1 || skey[t + 1] != key)) {
#pragma unroll
        for (int j = 0; j < V::N; ++j) partial[((size_t)key + blockIdx.x) * V::N + j] = v.v[j];
    }
}

// (a) amounts of the three ions per tag: |T|/(d+1) * sum over the cell's vertices of the fields of the cell's side (exact P1 integral)
template <int DIM>
__global__ void __launch_bounds__(NT) k_diag_cells(int n, const int32_t* __restrict__ item, const int32_t* __restrict__ key,
                                                   const int32_t* __restrict__ cells, const uint8_t* __restrict__ cell_side,
                                                   const double* __restrict__ coords, FieldPtrs f, double* __restrict__ partial) {
    const int i = blockIdx.x * NT + threadIdx.x;
    const bool live = i < n;
    DiagSum<3> v = DiagSum<3>::identity();
    int k = -1;
    if (live) {
        const int c = item[i];
        k = key[i];
        int vv[DIM + 1];
#pragma unroll
        for (int a = 0; a <= DIM; ++a) vv[a] = cells[(size_t)c * (DIM + 1) + a];
        double e[DIM][DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
            for (int b = 0; b < DIM; ++b) e[a][b] = coords[(size_t)vv[a + 1] * DIM + b] - coords[(size_t)vv[0] * DIM + b];
        const double det = DIM == 2 ? e[0][0] * e[1][1] - e[0][1] * e[1][0]
                                    : e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) - e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]) +
                                          e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
        const double w = fabs(det) / (DIM == 2 ? 6.0 : 24.0);   // |T| / (d+1) = |det| / (d! (d+1))
        const bool ext = cell_side[c] != 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double* fj = ext ? f.ke[j] : f.ki[j];
            double s = 0.0;
#pragma unroll
            for (int a = 0; a <= DIM; ++a) s += fj[vv[a]];
            v.v[j] = w * s;
        }
    }
    diag_chunk_partials<DiagSum<3>, NT>(k, live, i == n - 1, v, partial);
}

// (b) integral over the selected membrane facets of the sum of a program's outputs: quadrature points q, weights q_w |F|
static constexpr int DIAG_BT = 128;   // facets per block: the interpreter's LDS register file is [n_regs][DIAG_BT] doubles
struct DiagConsts { double v[KNP_DIAG_MAX_CONSTS]; };
template <int DIM, bool FUNCS = false>
__global__ void __launch_bounds__(DIAG_BT) k_diag_facets(int n, const int32_t* __restrict__ item, const int32_t* __restrict__ key,
                                                         const int32_t* __restrict__ fv, const double* __restrict__ fmeas, int n_q,
                                                         const double* __restrict__ qp, const double* __restrict__ qw, FieldPtrs f,
                                                         int n_aux, const double* __restrict__ coords, const int32_t* __restrict__ code,
                                                         int n_instr, DiagConsts K, int n_consts, double* __restrict__ partial) {
    extern __shared__ double dsmem[];     // register file of the interpreter
    __shared__ double sk[KNP_DIAG_MAX_CONSTS];
    for (int i = threadIdx.x; i < n_consts; i += DIAG_BT) sk[i] = K.v[i];
    __syncthreads();
    const int i = blockIdx.x * DIAG_BT + threadIdx.x;
    const bool live = i < n;
    const int ii = live ? i : n - 1;      // idle lanes shadow the last facet with weight zero: the interpreter's wave stays uniform
    const int g = item[ii];
    int v[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) v[a] = fv[(size_t)g * DIM + a];
    const double meas = live ? fmeas[g] : 0.0;
    double* reg = dsmem + threadIdx.x;
    double acc = 0.0;
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
                si += lam[a] * f.ki[j][v[a]];
                se += lam[a] * f.ke[j][v[a]];
            }
            kiq[0][j] = si;
            keq[0][j] = se;
            Iout[0][j] = 0.0;
        }
#pragma unroll
        for (int a = 0; a < DIM; ++a) phq[0] += lam[a] * f.phim[v[a]];
        for (int k = 0; k < n_aux; ++k) {
            double t = 0.0;
#pragma unroll
            for (int a = 0; a < DIM; ++a) t += lam[a] * f.aux[k][v[a]];
            auxq[0][k] = t;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            double t = 0.0;
            if (d < DIM) {
#pragma unroll
                for (int a = 0; a < DIM; ++a) t += lam[a] * coords[(size_t)v[a] * DIM + d];
            }
            xq[0][d] = t;
        }
        run_program<1, DIAG_BT, FUNCS>(code, n_instr, sk, kiq, keq, phq, auxq, xq, Iout, reg);
        acc += qw[q] * meas * (Iout[0][0] + Iout[0][1] + Iout[0][2]);
    }
    diag_chunk_partials<DiagSum<1>, DIAG_BT>(live ? key[i] : -1, live, i == n - 1, DiagSum<1>{{acc}}, partial);
}

// (c) molar flux of every ion through the selected membrane facets, on both sides:
//   flux[s][k] = -D_k (W0 sum_a g^s_a c^s_k(v^s_a) + (z_k/psi) (sum_b W_b c^s_k(f_b)) (sum_a g^s_a phi^s(v^s_a)))
// with g^s_a = grad(lambda_a) . n_s on the side's cell (n_s: unit normal out of that cell), W0 = |F| sum_q w_q m_q and
// W_b = |F| sum_q w_q m_q lambda_b(q) (m: the box mask at the quadrature points).  Everything but the nodal values is time invariant
// and comes from one record per facet, built on the host (flux_records) in the order of the tag map.  The record, in 16-byte units:
//   [0] 4 x int32 vertices of the intracellular cell: the facet's vertices f_0..f_{DIM-1} first, the opposite vertex at DIM
//   [1] the same for the extracellular cell (same facet vertices, its own opposite vertex); in 2D the fourth id is unused
//   then doubles g^0[DIM+1], g^1[DIM+1], W0, W_b[DIM] (2D: one pad) -- 128 B in 3D, 112 B in 2D.
template <int DIM> struct FluxRecord { static constexpr int UNITS = DIM == 3 ? 8 : 7; };
struct FluxCoef { double D[3], zp[3]; };
template <int DIM>
__global__ void __launch_bounds__(NT) k_diag_fluxes(int n, const int32_t* __restrict__ key, const double2* __restrict__ rec, FieldPtrs f,
                                                    const double* __restrict__ phi_i, const double* __restrict__ phi_e, FluxCoef K,
                                                    double* __restrict__ partial) {
    constexpr int UNITS = FluxRecord<DIM>::UNITS, ND = 2 * (UNITS - 2);
    const int i = blockIdx.x * NT + threadIdx.x;
    const bool live = i < n;
    DiagSum<6> v = DiagSum<6>::identity();
    int k = -1;
    if (live) {
        k = key[i];
        const double2* r = rec + (size_t)i * UNITS;
        const int4 ia = *reinterpret_cast<const int4*>(r), ib = *reinterpret_cast<const int4*>(r + 1);
        const int vs[2][4] = {{ia.x, ia.y, ia.z, ia.w}, {ib.x, ib.y, ib.z, ib.w}};
        double d[ND];
#pragma unroll
        for (int u = 0; u < UNITS - 2; ++u) {
            const double2 t = r[2 + u];
            d[2 * u] = t.x;
            d[2 * u + 1] = t.y;
        }
        const double W0 = d[2 * (DIM + 1)];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const double* g = d + s * (DIM + 1);
            const double* ph = s ? phi_e : phi_i;
            double gphi = 0.0;
#pragma unroll
            for (int a = 0; a <= DIM; ++a) gphi += g[a] * ph[vs[s][a]];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double* c = s ? f.ke[j] : f.ki[j];
                double gc = 0.0, wc = 0.0;
#pragma unroll
                for (int a = 0; a <= DIM; ++a) {
                    const double ca = c[vs[s][a]];
                    gc += g[a] * ca;
                    if (a < DIM) wc += d[2 * (DIM + 1) + 1 + a] * ca;
                }
                v.v[3 * s + j] = -K.D[j] * (W0 * gc + K.zp[j] * wc * gphi);
            }
        }
    }
    diag_chunk_partials<DiagSum<6>, NT>(k, live, i == n - 1, v, partial);
}

// (d) per tag the integral, the minimum and the maximum of the nodal phi_m over the selected membrane facets:
//   I = sum_F |F|/d sum_a phi(v_a(F)) (exact P1 integral), min / max over all vertices of the tag's facets.
// The reduction is DiagPhim's: the operator triple (+, min, max) on (I, min, max); idle lanes carry its identity.
template <int DIM>
__global__ void __launch_bounds__(DIAG_BT) k_diag_phim(int n, const int32_t* __restrict__ item, const int32_t* __restrict__ key,
                                                       const int32_t* __restrict__ fv, const double* __restrict__ fmeas,
                                                       const double* __restrict__ phim, double* __restrict__ partial) {
    const int i = blockIdx.x * DIAG_BT + threadIdx.x;
    const bool live = i < n;
    DiagPhim v = DiagPhim::identity();
    int k = -1;
    if (live) {
        k = key[i];
        const int g = item[i];
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            const double ph = phim[fv[(size_t)g * DIM + a]];
            s += ph;
            v.v[1] = fmin(v.v[1], ph);
            v.v[2] = fmax(v.v[2], ph);
        }
        v.v[0] = fmeas[g] * (1.0 / DIM) * s;
    }
    diag_chunk_partials<DiagPhim, DIAG_BT>(k, live, i == n - 1, v, partial);
}

template <class V>
__device__ __forceinline__ V diag_load(const double* __restrict__ partial, int s, int b) {
    V r;
#pragma unroll
    for (int j = 0; j < V::N; ++j) r.v[j] = partial[((size_t)s + b) * V::N + j];
    return r;
}
template <class V>
__device__ __forceinline__ void diag_store(double* __restrict__ out, int s, const V& v) {
#pragma unroll
    for (int j = 0; j < V::N; ++j) out[(size_t)s * V::N + j] = v.v[j];
}

// A tag's partials in a fixed order; empty tags give the identity.  k_diag_combine, one wave per tag: lane l folds the chunks
// first + l, first + l + 64, ... in that order, then a butterfly over the 64 lanes.  A map with wave_chunks > 0 gives its tags of
// more chunks than that to k_diag_combine_long instead, one workgroup per tag of the map's host-built list: thread t folds the
// chunks first + t, first + t + NT, ..., then a fixed-order tree in LDS.  Which kernel takes a tag depends on its chunk count alone.
template <class V>
__global__ void __launch_bounds__(NT) k_diag_combine(int n_tags, int chunk, int wave_chunks, const int32_t* __restrict__ seg_ptr,
                                                     const double* __restrict__ partial, double* __restrict__ out) {
    const int s = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (s >= n_tags) return;              // whole waves
    const int lo = seg_ptr[s], hi = seg_ptr[s + 1];
    V v = V::identity();
    if (hi > lo) {
        const int b0 = lo / chunk, b1 = (hi - 1) / chunk;
        if (wave_chunks > 0 && b1 - b0 + 1 > wave_chunks) return;      // the workgroup kernel's
        for (int b = b0 + lane; b <= b1; b += 64) v = V::op(v, diag_load<V>(partial, s, b));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        V w;
#pragma unroll
        for (int j = 0; j < V::N; ++j) w.v[j] = __shfl_xor(v.v[j], o, 64);
        v = V::op(v, w);
    }
    if (lane == 0) diag_store(out, s, v);
}

template <class V>
__global__ void __launch_bounds__(NT) k_diag_combine_long(const int32_t* __restrict__ long_tags, int chunk,
                                                          const int32_t* __restrict__ seg_ptr, const double* __restrict__ partial,
                                                          double* __restrict__ out) {
    __shared__ double sv[V::N][NT];
    const int s = long_tags[blockIdx.x];
    const int t = threadIdx.x;
    const int b0 = seg_ptr[s] / chunk, b1 = (seg_ptr[s + 1] - 1) / chunk;      // listed tags are not empty
    V v = V::identity();
    for (int b = b0 + t; b <= b1; b += NT) v = V::op(v, diag_load<V>(partial, s, b));
#pragma unroll
    for (int j = 0; j < V::N; ++j) sv[j][t] = v.v[j];
    __syncthreads();
    for (int d = NT / 2; d > 0; d >>= 1) {
        if (t < d) {
            V w;
#pragma unroll
            for (int j = 0; j < V::N; ++j) w.v[j] = sv[j][t + d];
            v = V::op(v, w);
#pragma unroll
            for (int j = 0; j < V::N; ++j) sv[j][t] = v.v[j];
        }
        __syncthreads();
    }
    if (t == 0) diag_store(out, s, v);
}

static void diag_map_free(KnpDiagMap& m) {
    dev_free(m.d_ptr); dev_free(m.d_item); dev_free(m.d_key); dev_free(m.d_partial); dev_free(m.d_long);
    m = KnpDiagMap();
}
void knp_diag_free(knp_ctx* ctx) {
    diag_map_free(ctx->diag_cells);
    diag_map_free(ctx->diag_facets);
    diag_map_free(ctx->diag_flux);
    dev_free(ctx->d_flux_rec);
    diag_map_free(ctx->diag_phim);
    diag_map_free(ctx->diag_act);
    dev_free(ctx->diag_code);
    ctx->diag_n_instr = ctx->diag_n_regs = ctx->diag_n_consts = 0;
    ctx->diag_prog = false;
}

// validate a host tag map (items in [0, n_items), each at most once, seg_ptr non-decreasing from 0) and upload it with its scratch;
// wave_chunks > 0: the tags of more chunks than that go on the list of k_diag_combine_long.  A failed upload leaves no map.
static int diag_map_set(knp_ctx* ctx, KnpDiagMap& m, int n_tags, const int32_t* seg_ptr, const int32_t* items, int n_items, int chunk,
                        int nv, int wave_chunks, const char* what) {
    if (n_tags < 0 || (n_tags > 0 && !seg_ptr)) { ctx->err = std::string(what) + ": bad tag count or null seg_ptr"; return KNP_E_ARG; }
    const int n = n_tags > 0 ? seg_ptr[n_tags] : 0;
    if (n_tags > 0 && seg_ptr[0] != 0) { ctx->err = std::string(what) + ": seg_ptr[0] must be 0"; return KNP_E_ARG; }
    if (n < 0 || n > n_items || (n > 0 && !items)) { ctx->err = std::string(what) + ": more items than the mesh has, or null items"; return KNP_E_ARG; }
    std::vector<int32_t> key((size_t)n), lng;
    std::vector<uint8_t> seen((size_t)std::max(n_items, 1), 0);
    for (int s = 0; s < n_tags; ++s) {
        if (seg_ptr[s + 1] < seg_ptr[s]) { ctx->err = std::string(what) + ": seg_ptr must be non-decreasing"; return KNP_E_ARG; }
        for (int i = seg_ptr[s]; i < seg_ptr[s + 1]; ++i) {
            const int it = items[i];
            if (it < 0 || it >= n_items || seen[it]) { ctx->err = std::string(what) + ": item out of range or listed twice"; return KNP_E_ARG; }
            seen[it] = 1;
            key[i] = s;
        }
        if (wave_chunks > 0 && seg_ptr[s + 1] > seg_ptr[s] && (seg_ptr[s + 1] - 1) / chunk - seg_ptr[s] / chunk + 1 > wave_chunks) lng.push_back(s);
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));   // a diagnostic in flight may still read the old map
    diag_map_free(m);
    std::vector<int32_t> ptr(seg_ptr, seg_ptr + (n_tags > 0 ? n_tags + 1 : 0));
    std::vector<int32_t> itv(items, items + n);
    m.n_tags = n_tags;
    m.n = n;
    m.chunk = chunk;
    m.n_chunks = (n + chunk - 1) / chunk;
    m.wave_chunks = wave_chunks;
    m.n_long = (int)lng.size();
    const size_t np = (size_t)(n_tags + m.n_chunks) * nv;
    const int rc = [&]() -> int {
        KCHK(dev_upload(ctx, &m.d_ptr, ptr));
        KCHK(dev_upload(ctx, &m.d_item, itv));
        KCHK(dev_upload(ctx, &m.d_key, key));
        if (m.n_long > 0) KCHK(dev_upload(ctx, &m.d_long, lng));
        HIPCHK(hipMalloc((void**)&m.d_partial, std::max<size_t>(np, 1) * sizeof(double)));
        return KNP_OK;
    }();
    if (rc != KNP_OK) diag_map_free(m);
    return rc;
}

template <class V>
static int diag_combine(knp_ctx* ctx, const KnpDiagMap& m, double* out) {
    if (m.n_tags == 0) return KNP_OK;
    const unsigned nb = (unsigned)((m.n_tags + NT / 64 - 1) / (NT / 64));
    hipLaunchKernelGGL(k_diag_combine<V>, dim3(nb), dim3(NT), 0, ctx->stream, m.n_tags, m.chunk, m.wave_chunks, m.d_ptr, m.d_partial, out);
    HIPCHK(hipGetLastError());
    if (m.n_long > 0) {
        hipLaunchKernelGGL(k_diag_combine_long<V>, dim3(m.n_long), dim3(NT), 0, ctx->stream, m.d_long, m.chunk, m.d_ptr, m.d_partial, out);
        HIPCHK(hipGetLastError());
    }
    return KNP_OK;
}

// the last two argument checks of every reduction: an output buffer and a map
static int diag_check(knp_ctx* ctx, const double* out, bool have_map, const char* no_map) {
    if (!out) { ctx->err = "null output buffer"; return KNP_E_ARG; }
    if (!have_map) { ctx->err = no_map; return KNP_E_STATE; }
    return KNP_OK;
}

// f(std::integral_constant<int, DIM>()) for the mesh's dimension
template <class F>
static auto by_dim(int dim, F&& f) { return dim == 2 ? f(std::integral_constant<int, 2>()) : f(std::integral_constant<int, 3>()); }

// gradients of the barycentric coordinates of the simplex x[0..DIM] (rows of DIM coordinates): G[a] = grad(lambda_a); false when flat
template <int DIM>
static bool simplex_gradients(const double (*x)[3], double (*G)[3]) {
    double e[3][3] = {{0}};
    for (int a = 0; a < DIM; ++a)
        for (int c = 0; c < DIM; ++c) e[a][c] = x[a + 1][c] - x[0][c];
    if (DIM == 2) {
        const double det = e[0][0] * e[1][1] - e[0][1] * e[1][0];
        if (det == 0.0) return false;
        G[1][0] = e[1][1] / det;  G[1][1] = -e[1][0] / det;
        G[2][0] = -e[0][1] / det; G[2][1] = e[0][0] / det;
    } else {
        double cr[3][3];      // cr[a] = e[a+1] x e[a+2]: grad(lambda_{a+1}) = cr[a] / det
        for (int a = 0; a < 3; ++a) {
            const double *u = e[(a + 1) % 3], *w = e[(a + 2) % 3];
            cr[a][0] = u[1] * w[2] - u[2] * w[1]; cr[a][1] = u[2] * w[0] - u[0] * w[2]; cr[a][2] = u[0] * w[1] - u[1] * w[0];
        }
        const double det = e[0][0] * cr[0][0] + e[0][1] * cr[0][1] + e[0][2] * cr[0][2];
        if (det == 0.0) return false;
        for (int a = 0; a < 3; ++a)
            for (int c = 0; c < 3; ++c) G[a + 1][c] = cr[a][c] / det;
    }
    for (int c = 0; c < DIM; ++c) {
        G[0][c] = 0.0;
        for (int a = 1; a <= DIM; ++a) G[0][c] -= G[a][c];
    }
    return true;
}

// the records of k_diag_fluxes for the facets of a tag map, in map order (host, once per map)
template <int DIM>
static int flux_records(knp_ctx* ctx, const int32_t* facets, int n, const std::vector<double>& coords, const double* q_pts,
                        const double* q_w, const double* lo, const double* hi, std::vector<double2>& rec) {
    constexpr int UNITS = FluxRecord<DIM>::UNITS;
    const KnpHostGraph& g = ctx->g;
    rec.assign((size_t)n * UNITS, make_double2(0.0, 0.0));
    int64_t bad = 0;
#pragma omp parallel for schedule(static) reduction(+ : bad) num_threads(knp_host_threads())
    for (int i = 0; i < n; ++i) {
        const int F = facets[i];
        int32_t ids[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        double d[2 * (UNITS - 2)] = {0.0};
        double xf[DIM + 1][3], G[DIM + 1][3], nrm[3];
        bool ok = g.gopp[(size_t)2 * F + 1] >= 0;
        for (int s = 0; s < 2 && ok; ++s) {
            for (int b = 0; b < DIM; ++b) ids[s][b] = g.fv[(size_t)F * DIM + b];
            ids[s][DIM] = g.gopp[(size_t)2 * F + s];
            for (int a = 0; a <= DIM; ++a)
                for (int c = 0; c < DIM; ++c) xf[a][c] = coords[(size_t)ids[s][a] * DIM + c];
            ok = simplex_gradients<DIM>(xf, G);
            if (!ok) break;
            if (s == 0) {     // grad(lambda_opposite) points into the cell along the facet normal: n_0 = -grad / |grad|, n_1 = -n_0
                double len = 0.0;
                for (int c = 0; c < DIM; ++c) len += G[DIM][c] * G[DIM][c];
                len = std::sqrt(len);
                for (int c = 0; c < DIM; ++c) nrm[c] = -G[DIM][c] / len;
            }
            for (int a = 0; a <= DIM; ++a) {
                double t = 0.0;
                for (int c = 0; c < DIM; ++c) t += G[a][c] * nrm[c];
                d[s * (DIM + 1) + a] = s == 0 ? t : -t;
            }
        }
        if (!ok) { ++bad; continue; }
        double* W = d + 2 * (DIM + 1);     // W0, W_b: the facet rule with the mask at its points (side 1's xf holds the facet vertices first)
        for (int q = 0; q < g.n_q; ++q) {
            bool in = true;
            if (lo)
                for (int c = 0; c < DIM; ++c) {
                    double x = 0.0;
                    for (int b = 0; b < DIM; ++b) x += q_pts[(size_t)q * DIM + b] * xf[b][c];
                    in = in && lo[c] < x && x < hi[c];
                }
            if (!in) continue;
            const double w = g.fmeas[F] * q_w[q];
            W[0] += w;
            for (int b = 0; b < DIM; ++b) W[1 + b] += w * q_pts[(size_t)q * DIM + b];
        }
        double2* r = &rec[(size_t)i * UNITS];
        std::memcpy(r, ids, sizeof(ids));
        std::memcpy(r + 2, d, sizeof(d));
    }
    if (bad) { ctx->err = "flux facet map: a listed facet has a flat cell or an extracellular cell that does not hold the facet"; return KNP_E_MESH; }
    return KNP_OK;
}

extern "C" {

int knp_diag_set_cell_tags(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr, const int32_t* cells) {
    CHECK_CTX(ctx);
    return diag_map_set(ctx, ctx->diag_cells, n_tags, seg_ptr, cells, ctx->g.n_c_owned, NT, 3, 0, "cell tag map");
}

int knp_diag_volume_integrals(knp_ctx* ctx, const knp_fields* fields, double* out) {
    CHECK_CTX(ctx);
    KCHK(check_fields(ctx, fields, false));
    const KnpDiagMap& m = ctx->diag_cells;
    KCHK(diag_check(ctx, out, m.d_ptr, "no cell tag map (knp_diag_set_cell_tags)"));
    const FieldPtrs f = make_fields(fields);
    if (m.n > 0) {
        by_dim(ctx->g.dim, [&](auto D) {
            hipLaunchKernelGGL(k_diag_cells<D()>, dim3(m.n_chunks), dim3(NT), 0, ctx->stream, m.n, m.d_item, m.d_key, ctx->d_cells,
                               ctx->d_cell_side, ctx->d_coords, f, m.d_partial);
        });
        HIPCHK(hipGetLastError());
    }
    return diag_combine<DiagSum<3>>(ctx, m, out);
}

int knp_diag_set_facet_tags(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr, const int32_t* facets) {
    CHECK_CTX(ctx);
    return diag_map_set(ctx, ctx->diag_facets, n_tags, seg_ptr, facets, ctx->g.n_g, DIAG_BT, 1, 0, "facet tag map");
}

int knp_diag_set_program(knp_ctx* ctx, int32_t n_instr, const int32_t* code, int32_t n_consts, const double* consts) {
    CHECK_CTX(ctx);
    if (n_instr < 0 || (n_instr && !code) || n_consts < 0 || n_consts > KNP_DIAG_MAX_CONSTS || (n_consts && !consts)) {
        ctx->err = "bad diagnostic program arguments (at most " + std::to_string(KNP_DIAG_MAX_CONSTS) + " constants)";
        return KNP_E_ARG;
    }
    int n_regs = 0;
    KCHK(validate_program(ctx, n_instr, code, n_consts, &n_regs));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    dev_free(ctx->diag_code);
    KCHK(dev_upload_raw(ctx, &ctx->diag_code, code, (size_t)4 * n_instr));
    ctx->diag_n_instr = n_instr;
    ctx->diag_n_regs = n_regs;
    ctx->diag_funcs = program_uses_funcs(n_instr, code);
    ctx->diag_n_consts = n_consts;
    for (int i = 0; i < n_consts; ++i) ctx->diag_consts[i] = consts[i];
    ctx->diag_prog = true;
    return KNP_OK;
}

int knp_diag_set_program_constants(knp_ctx* ctx, int32_t n_consts, const double* consts) {
    CHECK_CTX(ctx);
    if (!ctx->diag_prog || n_consts != ctx->diag_n_consts || (n_consts && !consts)) { ctx->err = "diagnostic program / constant count mismatch"; return KNP_E_ARG; }
    for (int i = 0; i < n_consts; ++i) ctx->diag_consts[i] = consts[i];   // kernel arguments of the next launch: nothing to copy
    return KNP_OK;
}

int knp_diag_membrane_integral(knp_ctx* ctx, const knp_fields* fields, double* out) {
    CHECK_CTX(ctx);
    KCHK(check_fields(ctx, fields, true));
    const KnpDiagMap& m = ctx->diag_facets;
    KCHK(diag_check(ctx, out, m.d_ptr, "no facet tag map (knp_diag_set_facet_tags)"));
    if (!ctx->diag_prog) { ctx->err = "no diagnostic program (knp_diag_set_program)"; return KNP_E_STATE; }
    int n_aux = 0;
    for (int k = 0; k < KNP_MAX_AUX; ++k)
        if (fields->aux[k]) n_aux = k + 1;
    for (int k = 0; k < n_aux; ++k)
        if (!fields->aux[k]) { ctx->err = "aux fields must be contiguous from index 0"; return KNP_E_ARG; }
    if (m.n > 0) {
        const FieldPtrs f = make_fields(fields);
        DiagConsts K;
        for (int i = 0; i < KNP_DIAG_MAX_CONSTS; ++i) K.v[i] = i < ctx->diag_n_consts ? ctx->diag_consts[i] : 0.0;
        const size_t lds = (size_t)std::max(ctx->diag_n_regs, 1) * DIAG_BT * sizeof(double);   // <= 48 registers: 48 KiB
        const int n_q = ctx->g.n_q;
        by_dim(ctx->g.dim, [&](auto D) {
            with_flag(ctx->diag_funcs, [&](auto M) {
                hipLaunchKernelGGL((k_diag_facets<D(), M()>), dim3(m.n_chunks), dim3(DIAG_BT), lds, ctx->stream, m.n, m.d_item, m.d_key, ctx->d_fv,
                                   ctx->d_fmeas, n_q, ctx->d_qp, ctx->d_qw, f, n_aux, ctx->d_coords, ctx->diag_code, ctx->diag_n_instr, K,
                                   ctx->diag_n_consts, m.d_partial);
            });
        });
        HIPCHK(hipGetLastError());
    }
    return diag_combine<DiagSum<1>>(ctx, m, out);
}

int knp_diag_set_flux_facets(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr, const int32_t* facets, const double* box_lo,
                             const double* box_hi) {
    CHECK_CTX(ctx);
    if ((box_lo == nullptr) != (box_hi == nullptr)) { ctx->err = "flux facet map: box_lo and box_hi must both be given or both be null"; return KNP_E_ARG; }
    const KnpHostGraph& g = ctx->g;
    KCHK(diag_map_set(ctx, ctx->diag_flux, n_tags, seg_ptr, facets, g.n_g, NT, 6, 0, "flux facet map"));
    dev_free(ctx->d_flux_rec);
    const int n = ctx->diag_flux.n;
    std::vector<double> coords((size_t)g.n_v * g.dim), qp((size_t)g.n_q * g.dim), qw((size_t)g.n_q);
    std::vector<double2> rec;
    int rc = KNP_OK;
    if (hipMemcpy(coords.data(), ctx->d_coords, coords.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(qp.data(), ctx->d_qp, qp.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(qw.data(), ctx->d_qw, qw.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
        ctx->err = "flux facet map: reading the mesh back failed";
        rc = KNP_E_HIP;
    }
    if (rc == KNP_OK)
        rc = by_dim(g.dim, [&](auto D) { return flux_records<D()>(ctx, facets, n, coords, qp.data(), qw.data(), box_lo, box_hi, rec); });
    if (rc == KNP_OK) rc = dev_upload(ctx, &ctx->d_flux_rec, rec);
    if (rc != KNP_OK) {     // no half-set map: the next knp_diag_membrane_fluxes reports KNP_E_STATE
        diag_map_free(ctx->diag_flux);
        dev_free(ctx->d_flux_rec);
    }
    return rc;
}

int knp_diag_membrane_fluxes(knp_ctx* ctx, const knp_fields* fields, const double* phi_i, const double* phi_e, const double* D,
                             const double* z_over_psi, double* out) {
    CHECK_CTX(ctx);
    if (!fields) { ctx->err = "null fields"; return KNP_E_ARG; }
    for (int j = 0; j < 3; ++j)
        if (!fields->k_i[j] || !fields->k_e[j]) { ctx->err = "null concentration field"; return KNP_E_ARG; }
    if (!phi_i || !phi_e) { ctx->err = "null potential field (phi_i / phi_e)"; return KNP_E_ARG; }
    if (!D || !z_over_psi) { ctx->err = "null flux coefficients (D / z_over_psi)"; return KNP_E_ARG; }
    const KnpDiagMap& m = ctx->diag_flux;
    KCHK(diag_check(ctx, out, m.d_ptr && ctx->d_flux_rec, "no flux facet map (knp_diag_set_flux_facets)"));
    if (m.n > 0) {
        const FieldPtrs f = make_fields(fields);
        FluxCoef K;
        for (int j = 0; j < 3; ++j) { K.D[j] = D[j]; K.zp[j] = z_over_psi[j]; }
        by_dim(ctx->g.dim, [&](auto D) {
            hipLaunchKernelGGL(k_diag_fluxes<D()>, dim3(m.n_chunks), dim3(NT), 0, ctx->stream, m.n, m.d_key, ctx->d_flux_rec, f, phi_i, phi_e, K,
                               m.d_partial);
        });
        HIPCHK(hipGetLastError());
    }
    return diag_combine<DiagSum<6>>(ctx, m, out);
}

static constexpr int PHIM_WAVE_CHUNKS = 64;      // longer tags take the workgroup combine
int knp_diag_set_phim_facets(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr, const int32_t* facets) {
    CHECK_CTX(ctx);
    return diag_map_set(ctx, ctx->diag_phim, n_tags, seg_ptr, facets, ctx->g.n_g, DIAG_BT, 3, PHIM_WAVE_CHUNKS, "phi_m facet map");
}

int knp_diag_membrane_potential(knp_ctx* ctx, const knp_fields* fields, double* out) {
    CHECK_CTX(ctx);
    if (!fields || !fields->phi_m) { ctx->err = "null fields or null phi_m field"; return KNP_E_ARG; }
    const KnpDiagMap& m = ctx->diag_phim;
    KCHK(diag_check(ctx, out, m.d_ptr, "no phi_m facet map (knp_diag_set_phim_facets)"));
    if (m.n > 0) {
        by_dim(ctx->g.dim, [&](auto D) {
            hipLaunchKernelGGL(k_diag_phim<D()>, dim3(m.n_chunks), dim3(DIAG_BT), 0, ctx->stream, m.n, m.d_item, m.d_key, ctx->d_fv,
                               ctx->d_fmeas, fields->phi_m, m.d_partial);
        });
        HIPCHK(hipGetLastError());
    }
    return diag_combine<DiagPhim>(ctx, m, out);
}

}  // extern "C"
