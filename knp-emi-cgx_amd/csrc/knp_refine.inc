// Uniform red refinement of P1 simplex meshes and the transfer of nodal fields to the refined mesh (knp_refine_*; the numbering,
// the child tables and the diagonal rule are stated in include/knpemi_hip.h).  Context-free: the mesh is refined before a knp_ctx
// exists.  Every kernel is one item per lane (an item = a cell, a facet, an edge or a vertex), wave64, no LDS, no atomics except the
// validation flag and the missing-edge counter; a lane stores all children of its item as consecutive 16-byte words.
//
//   R1  k_refine_edge_keys   a*nv + b of every local edge of a cell / facet; validates the item
//   R2  k_refine_vertices    coarse coordinates, then one midpoint per unique key; (a, b) per key
//   R3  k_refine_cells       2^dim children per cell; edge -> vertex by binary search in the sorted unique keys
//   R4  k_refine_facets      2^(dim-1) children per tagged facet, same search; a miss counts and writes nothing
//   R5  k_refine_prolong     n_fields nodal arrays at once: injection + the mean of the two parents
//
// The edge index is found by BINARY SEARCH in the unique keys, not through the inverse permutation of the sort: the facets need the
// search anyway (their edges may be missing), and the cells then read one array of n_edges keys that stays in L2 instead of a second
// one of n_cells * n_edges indices.

namespace knp_refine {

static constexpr int RNT = 256;
static constexpr int64_t RMAX = 2147483647;       // every count and every index of the fine mesh fits int32

// local edges in key order: 2 nodes 01; 3 nodes 01 02 12; 4 nodes 01 02 03 12 13 23
template <int NV>
__host__ __device__ constexpr int edge_a(int e) { return NV == 4 ? (e < 3 ? 0 : e < 5 ? 1 : 2) : NV == 3 ? (e < 2 ? 0 : 1) : 0; }
template <int NV>
__host__ __device__ constexpr int edge_b(int e) { return NV == 4 ? (e < 3 ? e + 1 : e < 5 ? e - 1 : 3) : NV == 3 ? (e < 2 ? e + 1 : 2) : 1; }
template <int NV>
struct n_edges_of { static constexpr int value = NV * (NV - 1) / 2; };

template <int NV>
__device__ inline bool item_valid(const int32_t (&v)[NV], int64_t nv) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        ok = ok && v[i] >= 0 && (int64_t)v[i] < nv;
#pragma unroll
        for (int j = 0; j < i; ++j) ok = ok && v[i] != v[j];
    }
    return ok;
}

template <int NV>
__device__ inline void load_item(const int32_t* __restrict__ items, int64_t i, int32_t (&v)[NV]) {
    if constexpr (NV == 4) {
        const int4 q = reinterpret_cast<const int4*>(items)[i];
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else if constexpr (NV == 2) {
        const int2 q = reinterpret_cast<const int2*>(items)[i];
        v[0] = q.x; v[1] = q.y;
    } else {
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = items[i * NV + k];
    }
}

__device__ inline int64_t edge_key(int32_t a, int32_t b, int64_t nv) {
    return (int64_t)(a < b ? a : b) * nv + (int64_t)(a < b ? b : a);
}

// position of the first key >= `key` in the sorted array, in [0, n]
__device__ inline int64_t lower_bound(const int64_t* __restrict__ keys, int64_t n, int64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- R1 ----------------------------------------------------------------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(RNT) void k_refine_edge_keys(int64_t n_items, int64_t nv, const int32_t* __restrict__ items,
                                                          int64_t* __restrict__ keys, int32_t* __restrict__ flag) {
    constexpr int NE = n_edges_of<NV>::value;
    const int64_t i = (int64_t)blockIdx.x * RNT + threadIdx.x;
    if (i >= n_items) return;
    int32_t v[NV];
    load_item<NV>(items, i, v);
    const bool ok = item_valid<NV>(v, nv);
    if (!ok) atomicOr(flag, 1);
#pragma unroll
    for (int e = 0; e < NE; ++e) keys[i * NE + e] = ok ? edge_key(v[edge_a<NV>(e)], v[edge_b<NV>(e)], nv) : 0;
}

// ---- R2 ----------------------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(RNT) void k_refine_vertices(int64_t nv, int64_t ne, const int64_t* __restrict__ ukeys,
                                                         const double* __restrict__ x, double* __restrict__ fx, int32_t* __restrict__ ev) {
    const int64_t i = (int64_t)blockIdx.x * RNT + threadIdx.x;
    if (i >= nv + ne) return;
    if (i < nv) {
#pragma unroll
        for (int k = 0; k < DIM; ++k) fx[i * DIM + k] = x[i * DIM + k];
        return;
    }
    const int64_t key = ukeys[i - nv];
    int64_t a = key / nv, b = key - a * nv;
    if (a < 0 || a >= nv) a = b = 0;                  // keys that edge_keys did not write: stay inside the arrays
    reinterpret_cast<int2*>(ev)[i - nv] = make_int2((int32_t)a, (int32_t)b);
#pragma unroll
    for (int k = 0; k < DIM; ++k) fx[i * DIM + k] = (x[a * DIM + k] + x[b * DIM + k]) * 0.5;
}

// ---- R3 ----------------------------------------------------------------------------------------------------------------------------
// the four children of a triangle (a 2D cell, or a tagged facet of a 3D mesh): L = {0, 1, 2, m01, m02, m12}
__device__ inline void store_triangle_children(const int32_t (&L)[6], int32_t* __restrict__ out, int64_t item) {
    int4* o = reinterpret_cast<int4*>(out) + item * 3;
    o[0] = make_int4(L[0], L[3], L[4], L[3]);         // (0 m01 m02) (m01 ..
    o[1] = make_int4(L[1], L[5], L[4], L[5]);         // .. 1 m12) (m02 m12 ..
    o[2] = make_int4(L[2], L[3], L[5], L[4]);         // .. 2) (m01 m12 m02)
}

// the four tetrahedra around diagonal K of the inner octahedron: L = {0, 1, 2, 3, m01, m02, m03, m12, m13, m23}
template <int K>
__device__ inline void store_inner(const int32_t (&L)[10], int4* __restrict__ o) {
    if constexpr (K == 0) {
        o[0] = make_int4(L[4], L[9], L[5], L[6]); o[1] = make_int4(L[4], L[9], L[6], L[8]);
        o[2] = make_int4(L[4], L[9], L[8], L[7]); o[3] = make_int4(L[4], L[9], L[7], L[5]);
    } else if constexpr (K == 1) {
        o[0] = make_int4(L[5], L[8], L[6], L[4]); o[1] = make_int4(L[5], L[8], L[9], L[6]);
        o[2] = make_int4(L[5], L[8], L[7], L[9]); o[3] = make_int4(L[5], L[8], L[4], L[7]);
    } else {
        o[0] = make_int4(L[6], L[7], L[4], L[5]); o[1] = make_int4(L[6], L[7], L[5], L[9]);
        o[2] = make_int4(L[6], L[7], L[9], L[8]); o[3] = make_int4(L[6], L[7], L[8], L[4]);
    }
}

// squared length (times 4) of the diagonal that joins the midpoints of the edges p-q and r-t.  Contraction is off: a fused
// multiply-add rounds once where the rule -- and its restatements -- round twice.
__device__ inline double diagonal_length(const double (&X)[4][3], int p, int q, int r, int t) {
#pragma clang fp contract(off)
    const double d0 = ((X[p][0] + X[q][0]) - X[r][0]) - X[t][0];
    const double d1 = ((X[p][1] + X[q][1]) - X[r][1]) - X[t][1];
    const double d2 = ((X[p][2] + X[q][2]) - X[r][2]) - X[t][2];
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

__device__ inline bool clearly_shorter(double s, double best) {
#pragma clang fp contract(off)
    const double bound = (1.0 - 0x1p-30) * best;
    return s < bound;
}

template <int DIM>
__global__ __launch_bounds__(RNT) void k_refine_cells(int64_t nc, int64_t nv, int64_t ne, const int64_t* __restrict__ ukeys,
                                                      const int32_t* __restrict__ cells, const int32_t* __restrict__ tags,
                                                      const double* __restrict__ x, int32_t* __restrict__ fcells,
                                                      int32_t* __restrict__ ftags, uint8_t* __restrict__ diagonal) {
    constexpr int NV = DIM + 1, NE = n_edges_of<NV>::value;
    const int64_t c = (int64_t)blockIdx.x * RNT + threadIdx.x;
    if (c >= nc) return;
    int32_t v[NV];
    load_item<NV>(cells, c, v);
    if (!item_valid<NV>(v, nv)) return;
    int32_t L[NV + NE];
#pragma unroll
    for (int k = 0; k < NV; ++k) L[k] = v[k];
#pragma unroll
    for (int e = 0; e < NE; ++e) L[NV + e] = (int32_t)(nv + lower_bound(ukeys, ne, edge_key(v[edge_a<NV>(e)], v[edge_b<NV>(e)], nv)));
    const int32_t tag = tags[c];
    if constexpr (DIM == 2) {
        store_triangle_children(L, fcells, c);
        reinterpret_cast<int4*>(ftags)[c] = make_int4(tag, tag, tag, tag);
    } else {
        double X[4][3];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int a = 0; a < 3; ++a) X[k][a] = x[(int64_t)v[k] * 3 + a];
        double best = diagonal_length(X, 0, 1, 2, 3);
        int kd = 0;
        const double s1 = diagonal_length(X, 0, 2, 1, 3);
        if (clearly_shorter(s1, best)) { best = s1; kd = 1; }
        const double s2 = diagonal_length(X, 0, 3, 1, 2);
        if (clearly_shorter(s2, best)) { best = s2; kd = 2; }
        int4* o = reinterpret_cast<int4*>(fcells) + c * 8;
        o[0] = make_int4(L[0], L[4], L[5], L[6]);
        o[1] = make_int4(L[4], L[1], L[7], L[8]);
        o[2] = make_int4(L[5], L[7], L[2], L[9]);
        o[3] = make_int4(L[6], L[8], L[9], L[3]);
        if (kd == 0) store_inner<0>(L, o + 4);
        else if (kd == 1) store_inner<1>(L, o + 4);
        else store_inner<2>(L, o + 4);
        int4* t4 = reinterpret_cast<int4*>(ftags) + c * 2;
        t4[0] = make_int4(tag, tag, tag, tag);
        t4[1] = make_int4(tag, tag, tag, tag);
        diagonal[c] = (uint8_t)kd;
    }
}

// ---- R4 ----------------------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(RNT) void k_refine_facets(int64_t nf, int64_t nv, int64_t ne, const int64_t* __restrict__ ukeys,
                                                       const int32_t* __restrict__ facets, const int32_t* __restrict__ values,
                                                       int32_t* __restrict__ ffacets, int32_t* __restrict__ fvalues,
                                                       int32_t* __restrict__ n_missing) {
    constexpr int NV = DIM, NE = n_edges_of<NV>::value;
    const int64_t f = (int64_t)blockIdx.x * RNT + threadIdx.x;
    if (f >= nf) return;
    int32_t v[NV];
    load_item<NV>(facets, f, v);
    bool ok = item_valid<NV>(v, nv);
    int32_t L[NV + NE];
#pragma unroll
    for (int k = 0; k < NV; ++k) L[k] = v[k];
    if (ok) {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int64_t key = edge_key(v[edge_a<NV>(e)], v[edge_b<NV>(e)], nv);
            const int64_t pos = lower_bound(ukeys, ne, key);
            ok = ok && pos < ne && ukeys[pos] == key;
            L[NV + e] = (int32_t)(nv + pos);
        }
    }
    if (!ok) {
        atomicAdd(n_missing, 1);
        return;
    }
    const int32_t val = values[f];
    if constexpr (DIM == 2) {
        reinterpret_cast<int4*>(ffacets)[f] = make_int4(L[0], L[2], L[2], L[1]);       // (a mab) (mab b)
        reinterpret_cast<int2*>(fvalues)[f] = make_int2(val, val);
    } else {
        store_triangle_children(L, ffacets, f);
        reinterpret_cast<int4*>(fvalues)[f] = make_int4(val, val, val, val);
    }
}

// ---- R5 ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RNT) void k_refine_prolong(int64_t nv, int64_t ne, const int32_t* __restrict__ ev, const double* __restrict__ in,
                                                        int64_t ld_in, double* __restrict__ out, int64_t ld_out) {
    const int64_t i = (int64_t)blockIdx.x * RNT + threadIdx.x;
    if (i >= nv + ne) return;
    const double* f = in + (int64_t)blockIdx.y * ld_in;
    double* g = out + (int64_t)blockIdx.y * ld_out;
    if (i < nv) {
        g[i] = f[i];
        return;
    }
    const int2 ab = reinterpret_cast<const int2*>(ev)[i - nv];
    g[i] = 0.5 * (f[ab.x] + f[ab.y]);
}

static inline unsigned blocks_for(int64_t n) { return (unsigned)((n + RNT - 1) / RNT); }
static inline int launched() { return hipGetLastError() == hipSuccess ? KNP_OK : KNP_E_HIP; }

}  // namespace knp_refine

extern "C" {

int knp_refine_edge_keys(int32_t nodes_per_item, int64_t n_items, int64_t n_vertices, const int32_t* items, int64_t* keys, int32_t* flag,
                         void* stream) {
    using namespace knp_refine;
    if (nodes_per_item < 2 || nodes_per_item > 4 || n_items < 0 || n_items > RMAX || n_vertices < 1 || n_vertices > RMAX || !flag) return KNP_E_ARG;
    if (n_items == 0) return KNP_OK;
    if (!items || !keys) return KNP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(blocks_for(n_items)), block(RNT);
    if (nodes_per_item == 2) hipLaunchKernelGGL(k_refine_edge_keys<2>, grid, block, 0, st, n_items, n_vertices, items, keys, flag);
    else if (nodes_per_item == 3) hipLaunchKernelGGL(k_refine_edge_keys<3>, grid, block, 0, st, n_items, n_vertices, items, keys, flag);
    else hipLaunchKernelGGL(k_refine_edge_keys<4>, grid, block, 0, st, n_items, n_vertices, items, keys, flag);
    return launched();
}

int knp_refine_vertices(int32_t dim, int64_t n_vertices, int64_t n_edges, const int64_t* unique_keys, const double* coords,
                        double* fine_coords, int32_t* edge_vertices, void* stream) {
    using namespace knp_refine;
    if ((dim != 2 && dim != 3) || n_vertices < 1 || n_edges < 0 || n_vertices + n_edges > RMAX || !coords || !fine_coords) return KNP_E_ARG;
    if (n_edges > 0 && (!unique_keys || !edge_vertices)) return KNP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(blocks_for(n_vertices + n_edges)), block(RNT);
    if (dim == 2) hipLaunchKernelGGL(k_refine_vertices<2>, grid, block, 0, st, n_vertices, n_edges, unique_keys, coords, fine_coords, edge_vertices);
    else hipLaunchKernelGGL(k_refine_vertices<3>, grid, block, 0, st, n_vertices, n_edges, unique_keys, coords, fine_coords, edge_vertices);
    return launched();
}

int knp_refine_cells(int32_t dim, int64_t n_cells, int64_t n_vertices, int64_t n_edges, const int64_t* unique_keys, const int32_t* cells,
                     const int32_t* cell_tags, const double* coords, int32_t* fine_cells, int32_t* fine_tags, uint8_t* diagonal, void* stream) {
    using namespace knp_refine;
    if ((dim != 2 && dim != 3) || n_cells < 0 || n_cells > (RMAX >> dim) || n_vertices < 1 || n_edges < 0 || n_vertices + n_edges > RMAX)
        return KNP_E_ARG;
    if (n_cells == 0) return KNP_OK;
    if (!unique_keys || !cells || !cell_tags || !fine_cells || !fine_tags || (dim == 3 && (!coords || !diagonal))) return KNP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(blocks_for(n_cells)), block(RNT);
    if (dim == 2)
        hipLaunchKernelGGL(k_refine_cells<2>, grid, block, 0, st, n_cells, n_vertices, n_edges, unique_keys, cells, cell_tags, coords, fine_cells,
                           fine_tags, diagonal);
    else
        hipLaunchKernelGGL(k_refine_cells<3>, grid, block, 0, st, n_cells, n_vertices, n_edges, unique_keys, cells, cell_tags, coords, fine_cells,
                           fine_tags, diagonal);
    return launched();
}

int knp_refine_facets(int32_t dim, int64_t n_facets, int64_t n_vertices, int64_t n_edges, const int64_t* unique_keys, const int32_t* facets,
                      const int32_t* values, int32_t* fine_facets, int32_t* fine_values, int32_t* n_missing, void* stream) {
    using namespace knp_refine;
    if ((dim != 2 && dim != 3) || n_facets < 0 || n_facets > (RMAX >> (dim - 1)) || n_vertices < 1 || n_edges < 0 || n_vertices + n_edges > RMAX ||
        !n_missing)
        return KNP_E_ARG;
    if (n_facets == 0) return KNP_OK;
    if (!facets || !values || !fine_facets || !fine_values || (n_edges > 0 && !unique_keys)) return KNP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(blocks_for(n_facets)), block(RNT);
    if (dim == 2)
        hipLaunchKernelGGL(k_refine_facets<2>, grid, block, 0, st, n_facets, n_vertices, n_edges, unique_keys, facets, values, fine_facets,
                           fine_values, n_missing);
    else
        hipLaunchKernelGGL(k_refine_facets<3>, grid, block, 0, st, n_facets, n_vertices, n_edges, unique_keys, facets, values, fine_facets,
                           fine_values, n_missing);
    return launched();
}

int knp_refine_prolong(int32_t n_fields, int64_t n_vertices, int64_t n_edges, const int32_t* edge_vertices, const double* in, int64_t ld_in,
                       double* out, int64_t ld_out, void* stream) {
    using namespace knp_refine;
    if (n_fields < 0 || n_fields > 65535 || n_vertices < 1 || n_edges < 0 || n_vertices + n_edges > RMAX || ld_in < n_vertices ||
        ld_out < n_vertices + n_edges)
        return KNP_E_ARG;
    if (n_fields == 0) return KNP_OK;
    if (!in || !out || (n_edges > 0 && !edge_vertices)) return KNP_E_ARG;
    const dim3 grid(blocks_for(n_vertices + n_edges), (unsigned)n_fields), block(RNT);
    hipLaunchKernelGGL(k_refine_prolong, grid, block, 0, (hipStream_t)stream, n_vertices, n_edges, edge_vertices, in, ld_in, out, ld_out);
    return launched();
}

}  // extern "C"
