// Level-set cut of a set of simplices: clipped cell surfaces, slices / iso-surfaces and isolines on membrane facets (knp_surface_*; the
// definitions, the tables and the orientation rule are stated in include/knpemi_hip.h, "level-set surfaces").  Context-free like the
// refinement: every array is device memory, every launch goes to the stream argument, nothing is synchronised.  Every kernel is one
// work item per lane (an item, a boundary facet, an element vertex or an output vertex), wave64, no LDS, no atomics, a grid of at most
// SBLOCKS blocks that strides over longer lists.  Between S2 and S3 the caller sorts and deduplicates the 64-bit vertex keys.
//
//   S0  k_surface_plane      s_v = n . (x_v - o), every operation rounded on its own
//   S1  k_surface_count      elements per item and per boundary facet (the caller scans them)
//   S2  k_surface_emit       elements as vertex keys, with their item, tag and kind, at the scanned offsets
//   S3  k_surface_vertices   unique key -> (a, b, w, side) and the position
//   S4  k_surface_remap      element keys -> output vertex numbers by binary search in the unique keys
//   S5  k_surface_gather     n_fields nodal arrays per side at the output vertices: the per-record kernel
//   S6  k_surface_measure    length / area per element
//
// S1 and S2 classify with the same code (classify<>), so the counts and the elements cannot disagree.

namespace knp_surface {

static constexpr int SNT = 256;
static constexpr int SBLOCKS = 1024;              // 4 blocks = 16 waves per CU of a 256-CU device; longer lists wrap
static constexpr int64_t SMAX = 2147483647;
static int32_t g_info[KNP_SI_COUNT] = {0};

struct SurfaceFieldPtrs {
    const double* p[KNP_SURFACE_MAX_FIELDS];
};

static inline dim3 grid_for(int kernel, int64_t n, unsigned ny = 1) {
    const int64_t want = (n + SNT - 1) / SNT;
    const unsigned blocks = (unsigned)(want < SBLOCKS ? want : SBLOCKS);
    g_info[KNP_SI_KERNEL] = kernel;
    g_info[KNP_SI_BLOCKS] = (int32_t)blocks;
    g_info[KNP_SI_THREADS] = SNT;
    g_info[KNP_SI_N] = (int32_t)(n < SMAX ? n : SMAX);
    g_info[KNP_SI_TRIPS] = (int32_t)((n + (int64_t)blocks * SNT - 1) / ((int64_t)blocks * SNT));
    g_info[KNP_SI_GRID_Y] = (int32_t)ny;
    return dim3(blocks, ny);
}
static inline int launched() { return hipGetLastError() == hipSuccess ? KNP_OK : KNP_E_HIP; }

__device__ inline int64_t vkey(int side, int32_t a, int32_t b, int64_t nv) {
    return ((int64_t)side << 62) + (int64_t)a * nv + (int64_t)b;
}

// what the level does to one simplex of NV vertices: t per vertex, the inside mask, and whether it takes part at all
template <int NV>
struct Cut {
    int32_t v[NV];
    unsigned mask;      // bit k: local vertex k is inside (t >= 0)
    int n_in;
    bool ok;            // every vertex in range and no NaN
};

template <int NV>
__device__ inline Cut<NV> classify(const int32_t* __restrict__ verts, int64_t i, int64_t nv, const double* __restrict__ s, double iso) {
    Cut<NV> c;
    c.mask = 0; c.n_in = 0; c.ok = true;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        c.v[k] = verts[i * NV + k];
        const bool in_range = c.v[k] >= 0 && (int64_t)c.v[k] < nv;
        const double t = in_range ? s[c.v[k]] - iso : 0.0;
        c.ok = c.ok && in_range && t == t;
        if (t >= 0.0) { c.mask |= 1u << k; ++c.n_in; }
    }
    return c;
}

template <int NPI>
__device__ inline int n_cut_elements(int n_in) {
    if constexpr (NPI == 4) return (n_in == 1 || n_in == 3) ? 1 : n_in == 2 ? 2 : 0;
    else return (n_in == 1 || n_in == 2) ? 1 : 0;
}
template <int NB>
__device__ inline int n_boundary_elements(int n_in) {
    if constexpr (NB == 3) return n_in == 2 ? 2 : n_in >= 1 ? 1 : 0;
    else return n_in >= 1 ? 1 : 0;
}

// sign of the permutation q of 0 .. N-1
template <int N>
__device__ inline int parity(const int (&q)[N]) {
    int inv = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) inv += q[j] > q[i];
    return (inv & 1) ? -1 : 1;
}

// sign of the item's signed volume in its stored vertex order; every operation rounded on its own, like the restatements
__device__ inline int volume_sign3(const double* __restrict__ x, const int32_t (&v)[4]) {
#pragma clang fp contract(off)
    double e[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) e[k][c] = x[(int64_t)v[k + 1] * 3 + c] - x[(int64_t)v[0] * 3 + c];
    const double c0 = e[1][1] * e[2][2] - e[1][2] * e[2][1];
    const double c1 = e[1][2] * e[2][0] - e[1][0] * e[2][2];
    const double c2 = e[1][0] * e[2][1] - e[1][1] * e[2][0];
    const double d = (e[0][0] * c0 + e[0][1] * c1) + e[0][2] * c2;
    return d > 0.0 ? 1 : d < 0.0 ? -1 : 0;
}
__device__ inline int volume_sign2(const double* __restrict__ x, const int32_t (&v)[3]) {
#pragma clang fp contract(off)
    const double a0 = x[(int64_t)v[1] * 2] - x[(int64_t)v[0] * 2], a1 = x[(int64_t)v[1] * 2 + 1] - x[(int64_t)v[0] * 2 + 1];
    const double b0 = x[(int64_t)v[2] * 2] - x[(int64_t)v[0] * 2], b1 = x[(int64_t)v[2] * 2 + 1] - x[(int64_t)v[0] * 2 + 1];
    const double d = a0 * b1 - a1 * b0;
    return d > 0.0 ? 1 : d < 0.0 ? -1 : 0;
}

// ---- S0 ----------------------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(SNT) void k_surface_plane(int64_t nv, const double* __restrict__ x, double o0, double o1, double o2, double n0,
                                                       double n1, double n2, double* __restrict__ s) {
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * SNT + threadIdx.x; i < nv; i += (int64_t)gridDim.x * SNT) {
        double r = (x[i * DIM] - o0) * n0 + (x[i * DIM + 1] - o1) * n1;
        if constexpr (DIM == 3) r = r + (x[i * DIM + 2] - o2) * n2;
        s[i] = r;
    }
}

// ---- S1 ----------------------------------------------------------------------------------------------------------------------------
template <int NPI>
__global__ __launch_bounds__(SNT) void k_surface_count(int64_t n_items, int64_t n_b, int64_t nv, const int32_t* __restrict__ items,
                                                       const int32_t* __restrict__ bfacets, const int32_t* __restrict__ bfacet_item,
                                                       const double* __restrict__ s, double iso, int32_t* __restrict__ counts) {
    for (int64_t i = (int64_t)blockIdx.x * SNT + threadIdx.x; i < n_items + n_b; i += (int64_t)gridDim.x * SNT) {
        int n = 0;
        if (i < n_items) {
            const Cut<NPI> c = classify<NPI>(items, i, nv, s, iso);
            n = c.ok ? n_cut_elements<NPI>(c.n_in) : 0;
        } else {
            const int64_t f = i - n_items;
            const Cut<NPI - 1> c = classify<NPI - 1>(bfacets, f, nv, s, iso);
            const int32_t it = bfacet_item[f];
            n = (c.ok && it >= 0 && (int64_t)it < n_items) ? n_boundary_elements<NPI - 1>(c.n_in) : 0;
        }
        counts[i] = n;
    }
}

// ---- S2 ----------------------------------------------------------------------------------------------------------------------------
template <int NPE>
__device__ inline void store_element(int64_t e, const int64_t (&k)[NPE], bool rev, int32_t item, int32_t tag, uint8_t kind,
                                     int64_t* __restrict__ keys, int32_t* __restrict__ e_item, int32_t* __restrict__ e_tag,
                                     uint8_t* __restrict__ e_kind) {
    keys[e * NPE] = k[0];
    if constexpr (NPE == 3) {
        keys[e * 3 + 1] = rev ? k[2] : k[1];
        keys[e * 3 + 2] = rev ? k[1] : k[2];
    } else {
        if (rev) { keys[e * 2] = k[1]; keys[e * 2 + 1] = k[0]; }
        else keys[e * 2 + 1] = k[1];
    }
    e_item[e] = item; e_tag[e] = tag; e_kind[e] = kind;
}

template <int NPI>
__global__ __launch_bounds__(SNT) void k_surface_emit(int64_t n_items, int64_t n_b, int64_t nv, int dim, const int32_t* __restrict__ items,
                                                      const uint8_t* __restrict__ item_side, const int32_t* __restrict__ item_ref,
                                                      const int32_t* __restrict__ bfacets, const int32_t* __restrict__ bfacet_item,
                                                      const double* __restrict__ s, double iso, const double* __restrict__ x,
                                                      const int64_t* __restrict__ offsets, int64_t n_el, int64_t* __restrict__ keys,
                                                      int32_t* __restrict__ e_item, int32_t* __restrict__ e_tag, uint8_t* __restrict__ e_kind) {
    constexpr int NPE = NPI - 1;
    for (int64_t i = (int64_t)blockIdx.x * SNT + threadIdx.x; i < n_items + n_b; i += (int64_t)gridDim.x * SNT) {
        const int64_t e0 = offsets[i];
        if (i < n_items) {
            const Cut<NPI> c = classify<NPI>(items, i, nv, s, iso);
            const int n = c.ok ? n_cut_elements<NPI>(c.n_in) : 0;
            if (n == 0 || e0 < 0 || e0 + n > n_el) continue;
            const int side = item_side[i] & 1;
            const int32_t tag = item_ref[i];
            int in[NPI], out[NPI], ni = 0, no = 0;          // ascending local indices of the inside / outside vertices
#pragma unroll
            for (int k = 0; k < NPI; ++k) {
                if (c.mask >> k & 1u) in[ni++] = k; else out[no++] = k;
            }
            auto cut = [&](int a, int b) { return vkey(side, c.v[a], c.v[b], nv); };
            if constexpr (NPI == 4) {
                const int sd = volume_sign3(x, c.v);
                if (c.n_in == 1) {
                    const int q[4] = {in[0], out[0], out[1], out[2]};
                    const int64_t k[3] = {cut(in[0], out[0]), cut(in[0], out[1]), cut(in[0], out[2])};
                    store_element<3>(e0, k, sd * parity(q) < 0, (int32_t)i, tag, 0, keys, e_item, e_tag, e_kind);
                } else if (c.n_in == 3) {
                    const int q[4] = {out[0], in[0], in[1], in[2]};
                    const int64_t k[3] = {cut(in[0], out[0]), cut(in[1], out[0]), cut(in[2], out[0])};
                    store_element<3>(e0, k, sd * parity(q) > 0, (int32_t)i, tag, 0, keys, e_item, e_tag, e_kind);
                } else {
                    const int q[4] = {in[0], in[1], out[0], out[1]};
                    const bool rev = sd * parity(q) < 0;
                    const int64_t pr = cut(in[0], out[0]), pt = cut(in[0], out[1]), qt = cut(in[1], out[1]), qr = cut(in[1], out[0]);
                    const int64_t k0[3] = {pr, pt, qt}, k1[3] = {pr, qt, qr};
                    store_element<3>(e0, k0, rev, (int32_t)i, tag, 0, keys, e_item, e_tag, e_kind);
                    store_element<3>(e0 + 1, k1, rev, (int32_t)i, tag, 0, keys, e_item, e_tag, e_kind);
                }
            } else {
                const int sd = dim == 2 ? volume_sign2(x, c.v) : 1;      // a facet of a 3D mesh: its stored order is its orientation
                if (c.n_in == 1) {
                    const int q[3] = {in[0], out[0], out[1]};
                    const int64_t k[2] = {cut(in[0], out[0]), cut(in[0], out[1])};
                    store_element<2>(e0, k, sd * parity(q) < 0, (int32_t)i, tag, 0, keys, e_item, e_tag, e_kind);
                } else {
                    const int q[3] = {out[0], in[0], in[1]};
                    const int64_t k[2] = {cut(in[0], out[0]), cut(in[1], out[0])};
                    store_element<2>(e0, k, sd * parity(q) > 0, (int32_t)i, tag, 0, keys, e_item, e_tag, e_kind);
                }
            }
        } else {
            const int64_t f = i - n_items;
            const Cut<NPE> c = classify<NPE>(bfacets, f, nv, s, iso);
            const int32_t it = bfacet_item[f];
            const int n = (c.ok && it >= 0 && (int64_t)it < n_items) ? n_boundary_elements<NPE>(c.n_in) : 0;
            if (n == 0 || e0 < 0 || e0 + n > n_el) continue;
            const int side = item_side[it] & 1;
            const int32_t tag = item_ref[it];
            auto own = [&](int a) { return vkey(side, c.v[a], c.v[a], nv); };
            auto cut = [&](int a, int b) { return vkey(side, c.v[a], c.v[b], nv); };
            if constexpr (NPE == 3) {
                if (c.n_in == 3) {
                    const int64_t k[3] = {own(0), own(1), own(2)};
                    store_element<3>(e0, k, false, it, tag, 1, keys, e_item, e_tag, e_kind);
                } else if (c.n_in == 1) {
                    const int a = c.mask == 1u ? 0 : c.mask == 2u ? 1 : 2, b = (a + 1) % 3, cc = (a + 2) % 3;
                    const int64_t k[3] = {own(a), cut(a, b), cut(a, cc)};
                    store_element<3>(e0, k, false, it, tag, 1, keys, e_item, e_tag, e_kind);
                } else {
                    const int cc = c.mask == 6u ? 0 : c.mask == 5u ? 1 : 2, a = (cc + 1) % 3, b = (cc + 2) % 3;
                    const int64_t bc = cut(b, cc), ac = cut(a, cc);
                    const int64_t k0[3] = {own(a), own(b), bc}, k1[3] = {own(a), bc, ac};
                    store_element<3>(e0, k0, false, it, tag, 1, keys, e_item, e_tag, e_kind);
                    store_element<3>(e0 + 1, k1, false, it, tag, 1, keys, e_item, e_tag, e_kind);
                }
            } else {
                const int64_t k[2] = {(c.mask & 1u) ? own(0) : cut(1, 0), (c.mask & 2u) ? own(1) : cut(0, 1)};
                store_element<2>(e0, k, false, it, tag, 1, keys, e_item, e_tag, e_kind);
            }
        }
    }
}

// ---- S3 ----------------------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(SNT) void k_surface_vertices(int64_t n_out, int64_t nv, const int64_t* __restrict__ ukeys,
                                                          const double* __restrict__ s, double iso, const double* __restrict__ x,
                                                          int32_t* __restrict__ va, int32_t* __restrict__ vb, double* __restrict__ vw,
                                                          uint8_t* __restrict__ vside, double* __restrict__ xyz) {
#pragma clang fp contract(off)
    for (int64_t i = (int64_t)blockIdx.x * SNT + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * SNT) {
        const int64_t key = ukeys[i];
        const int64_t rem = key & (((int64_t)1 << 62) - 1);
        int64_t a = rem / nv, b = rem - a * nv;
        if (key < 0 || a >= nv) a = b = 0;               // keys that k_surface_emit did not write: stay inside the arrays
        double w = 0.0;
        if (a != b) {
            const double ta = s[a] - iso, tb = s[b] - iso;
            w = ta / (ta - tb);
        }
        va[i] = (int32_t)a; vb[i] = (int32_t)b; vw[i] = w; vside[i] = (uint8_t)((key >> 62) & 1);
#pragma unroll
        for (int c = 0; c < DIM; ++c) xyz[i * DIM + c] = (1.0 - w) * x[a * DIM + c] + w * x[b * DIM + c];
    }
}

// ---- S4 ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SNT) void k_surface_remap(int64_t n_keys, int64_t n_out, const int64_t* __restrict__ keys,
                                                       const int64_t* __restrict__ ukeys, int32_t* __restrict__ elements) {
    for (int64_t i = (int64_t)blockIdx.x * SNT + threadIdx.x; i < n_keys; i += (int64_t)gridDim.x * SNT) {
        const int64_t key = keys[i];
        int64_t lo = 0, hi = n_out;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (ukeys[mid] < key) lo = mid + 1; else hi = mid;
        }
        elements[i] = (int32_t)lo;
    }
}

// ---- S5 ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SNT) void k_surface_gather(int64_t n_out, const int32_t* __restrict__ va, const int32_t* __restrict__ vb,
                                                        const double* __restrict__ vw, const uint8_t* __restrict__ vside, SurfaceFieldPtrs fi,
                                                        SurfaceFieldPtrs fe, double* __restrict__ out) {
#pragma clang fp contract(off)
    const double* __restrict__ Fi = fi.p[blockIdx.y];
    const double* __restrict__ Fe = fe.p[blockIdx.y];
    double* __restrict__ o = out + (int64_t)blockIdx.y * n_out;
    for (int64_t i = (int64_t)blockIdx.x * SNT + threadIdx.x; i < n_out; i += (int64_t)gridDim.x * SNT) {
        const double* __restrict__ F = vside[i] ? Fe : Fi;
        double r = __builtin_nan("");
        if (F) {
            const double w = vw[i];
            r = (1.0 - w) * F[va[i]] + w * F[vb[i]];
        }
        o[i] = r;
    }
}

// ---- S6 ----------------------------------------------------------------------------------------------------------------------------
template <int DIM, int NPE>
__global__ __launch_bounds__(SNT) void k_surface_measure(int64_t n_el, int64_t n_out, const int32_t* __restrict__ elements,
                                                         const double* __restrict__ xyz, double* __restrict__ measure) {
    for (int64_t i = (int64_t)blockIdx.x * SNT + threadIdx.x; i < n_el; i += (int64_t)gridDim.x * SNT) {
        double e[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        const int32_t v0 = elements[i * NPE];
        bool ok = v0 >= 0 && (int64_t)v0 < n_out;
#pragma unroll
        for (int k = 1; k < NPE; ++k) {
            const int32_t vk = elements[i * NPE + k];
            ok = ok && vk >= 0 && (int64_t)vk < n_out;
            if (ok)
#pragma unroll
                for (int c = 0; c < DIM; ++c) e[k - 1][c] = xyz[(int64_t)vk * DIM + c] - xyz[(int64_t)v0 * DIM + c];
        }
        double m;
        if constexpr (NPE == 2) {
            m = sqrt(e[0][0] * e[0][0] + e[0][1] * e[0][1] + e[0][2] * e[0][2]);
        } else {
            const double c0 = e[0][1] * e[1][2] - e[0][2] * e[1][1], c1 = e[0][2] * e[1][0] - e[0][0] * e[1][2],
                         c2 = e[0][0] * e[1][1] - e[0][1] * e[1][0];
            m = 0.5 * sqrt(c0 * c0 + c1 * c1 + c2 * c2);
        }
        measure[i] = ok ? m : __builtin_nan("");
    }
}

static inline bool shape_ok(int32_t dim, int32_t npi) { return (dim == 2 && npi == 3) || (dim == 3 && (npi == 3 || npi == 4)); }

}  // namespace knp_surface

extern "C" {

int knp_surface_plane(int32_t dim, int64_t n_vertices, const double* coords, const double* origin, const double* normal, double* s,
                      void* stream) {
    using namespace knp_surface;
    if ((dim != 2 && dim != 3) || n_vertices < 0 || n_vertices > SMAX || !origin || !normal) return KNP_E_ARG;
    if (n_vertices == 0) return KNP_OK;
    if (!coords || !s) return KNP_E_ARG;
    const double o2 = dim == 3 ? origin[2] : 0.0, n2 = dim == 3 ? normal[2] : 0.0;
    const dim3 grid = grid_for(KNP_SK_PLANE, n_vertices), block(SNT);
    if (dim == 2) hipLaunchKernelGGL(k_surface_plane<2>, grid, block, 0, (hipStream_t)stream, n_vertices, coords, origin[0], origin[1], o2, normal[0], normal[1], n2, s);
    else hipLaunchKernelGGL(k_surface_plane<3>, grid, block, 0, (hipStream_t)stream, n_vertices, coords, origin[0], origin[1], o2, normal[0], normal[1], n2, s);
    return launched();
}

int knp_surface_count(int32_t nodes_per_item, int64_t n_items, int64_t n_vertices, const int32_t* items, int64_t n_bfacets,
                      const int32_t* bfacets, const int32_t* bfacet_item, const double* s, double iso, int32_t* counts, void* stream) {
    using namespace knp_surface;
    if ((nodes_per_item != 3 && nodes_per_item != 4) || n_items < 0 || n_items > SMAX || n_bfacets < 0 || n_bfacets > SMAX ||
        n_items + n_bfacets > SMAX || n_vertices < 1 || n_vertices > SMAX)
        return KNP_E_ARG;
    if (n_items + n_bfacets == 0) return KNP_OK;
    if (!s || !counts || (n_items > 0 && !items) || (n_bfacets > 0 && (!bfacets || !bfacet_item))) return KNP_E_ARG;
    const dim3 grid = grid_for(KNP_SK_COUNT, n_items + n_bfacets), block(SNT);
    if (nodes_per_item == 4)
        hipLaunchKernelGGL(k_surface_count<4>, grid, block, 0, (hipStream_t)stream, n_items, n_bfacets, n_vertices, items, bfacets, bfacet_item, s, iso, counts);
    else
        hipLaunchKernelGGL(k_surface_count<3>, grid, block, 0, (hipStream_t)stream, n_items, n_bfacets, n_vertices, items, bfacets, bfacet_item, s, iso, counts);
    return launched();
}

int knp_surface_emit(int32_t dim, int32_t nodes_per_item, int64_t n_items, int64_t n_vertices, const int32_t* items, const uint8_t* item_side,
                     const int32_t* item_ref, int64_t n_bfacets, const int32_t* bfacets, const int32_t* bfacet_item, const double* s, double iso,
                     const double* coords, const int64_t* offsets, int64_t n_elements, int64_t* element_keys, int32_t* element_item,
                     int32_t* element_tag, uint8_t* element_kind, void* stream) {
    using namespace knp_surface;
    if (!shape_ok(dim, nodes_per_item) || n_items < 0 || n_items > SMAX || n_bfacets < 0 || n_bfacets > SMAX || n_items + n_bfacets > SMAX ||
        n_vertices < 1 || n_vertices > SMAX || n_elements < 0 || n_elements > SMAX)
        return KNP_E_ARG;
    if (n_items + n_bfacets == 0 || n_elements == 0) return KNP_OK;
    const bool needs_x = dim == nodes_per_item - 1;      // cells: the orientation comes from the signed volume
    if (!s || !offsets || !element_keys || !element_item || !element_tag || !element_kind || !item_side || !item_ref || !items ||
        (needs_x && !coords) || (n_bfacets > 0 && (!bfacets || !bfacet_item)))
        return KNP_E_ARG;
    const dim3 grid = grid_for(KNP_SK_EMIT, n_items + n_bfacets), block(SNT);
    if (nodes_per_item == 4)
        hipLaunchKernelGGL(k_surface_emit<4>, grid, block, 0, (hipStream_t)stream, n_items, n_bfacets, n_vertices, (int)dim, items, item_side, item_ref,
                           bfacets, bfacet_item, s, iso, coords, offsets, n_elements, element_keys, element_item, element_tag, element_kind);
    else
        hipLaunchKernelGGL(k_surface_emit<3>, grid, block, 0, (hipStream_t)stream, n_items, n_bfacets, n_vertices, (int)dim, items, item_side, item_ref,
                           bfacets, bfacet_item, s, iso, coords, offsets, n_elements, element_keys, element_item, element_tag, element_kind);
    return launched();
}

int knp_surface_vertices(int32_t dim, int64_t n_vertices, int64_t n_out, const int64_t* unique_keys, const double* s, double iso,
                         const double* coords, int32_t* vertex_a, int32_t* vertex_b, double* vertex_w, uint8_t* vertex_side, double* xyz,
                         void* stream) {
    using namespace knp_surface;
    if ((dim != 2 && dim != 3) || n_vertices < 1 || n_vertices > SMAX || n_out < 0 || n_out > SMAX) return KNP_E_ARG;
    if (n_out == 0) return KNP_OK;
    if (!unique_keys || !s || !coords || !vertex_a || !vertex_b || !vertex_w || !vertex_side || !xyz) return KNP_E_ARG;
    const dim3 grid = grid_for(KNP_SK_VERTICES, n_out), block(SNT);
    if (dim == 2)
        hipLaunchKernelGGL(k_surface_vertices<2>, grid, block, 0, (hipStream_t)stream, n_out, n_vertices, unique_keys, s, iso, coords, vertex_a, vertex_b,
                           vertex_w, vertex_side, xyz);
    else
        hipLaunchKernelGGL(k_surface_vertices<3>, grid, block, 0, (hipStream_t)stream, n_out, n_vertices, unique_keys, s, iso, coords, vertex_a, vertex_b,
                           vertex_w, vertex_side, xyz);
    return launched();
}

int knp_surface_remap(int64_t n_keys, int64_t n_out, const int64_t* element_keys, const int64_t* unique_keys, int32_t* elements, void* stream) {
    using namespace knp_surface;
    if (n_keys < 0 || n_keys > 3 * SMAX || n_out < 0 || n_out > SMAX) return KNP_E_ARG;
    if (n_keys == 0) return KNP_OK;
    if (!element_keys || !elements || (n_out > 0 && !unique_keys)) return KNP_E_ARG;
    const dim3 grid = grid_for(KNP_SK_REMAP, n_keys), block(SNT);
    hipLaunchKernelGGL(k_surface_remap, grid, block, 0, (hipStream_t)stream, n_keys, n_out, element_keys, unique_keys, elements);
    return launched();
}

int knp_surface_gather(int32_t n_fields, int64_t n_out, const int32_t* vertex_a, const int32_t* vertex_b, const double* vertex_w,
                       const uint8_t* vertex_side, const double* const* fields_i, const double* const* fields_e, double* out, void* stream) {
    using namespace knp_surface;
    if (n_fields < 0 || n_fields > KNP_SURFACE_MAX_FIELDS || n_out < 0 || n_out > SMAX || (!fields_i && !fields_e && n_fields > 0)) return KNP_E_ARG;
    if (n_fields == 0 || n_out == 0) return KNP_OK;
    if (!vertex_a || !vertex_b || !vertex_w || !vertex_side || !out) return KNP_E_ARG;
    SurfaceFieldPtrs fi, fe;
    for (int f = 0; f < KNP_SURFACE_MAX_FIELDS; ++f) {
        fi.p[f] = (fields_i && f < n_fields) ? fields_i[f] : nullptr;
        fe.p[f] = (fields_e && f < n_fields) ? fields_e[f] : nullptr;
    }
    const dim3 grid = grid_for(KNP_SK_GATHER, n_out, (unsigned)n_fields), block(SNT);
    hipLaunchKernelGGL(k_surface_gather, grid, block, 0, (hipStream_t)stream, n_out, vertex_a, vertex_b, vertex_w, vertex_side, fi, fe, out);
    return launched();
}

int knp_surface_measure(int32_t dim, int32_t nodes_per_element, int64_t n_elements, int64_t n_out, const int32_t* elements, const double* xyz,
                        double* measure, void* stream) {
    using namespace knp_surface;
    if ((dim != 2 && dim != 3) || (nodes_per_element != 2 && nodes_per_element != 3) || (nodes_per_element == 3 && dim != 3) || n_elements < 0 ||
        n_elements > SMAX || n_out < 0 || n_out > SMAX)
        return KNP_E_ARG;
    if (n_elements == 0) return KNP_OK;
    if (!elements || !xyz || !measure) return KNP_E_ARG;
    const dim3 grid = grid_for(KNP_SK_MEASURE, n_elements), block(SNT);
    hipStream_t st = (hipStream_t)stream;
    if (nodes_per_element == 3) hipLaunchKernelGGL((k_surface_measure<3, 3>), grid, block, 0, st, n_elements, n_out, elements, xyz, measure);
    else if (dim == 3) hipLaunchKernelGGL((k_surface_measure<3, 2>), grid, block, 0, st, n_elements, n_out, elements, xyz, measure);
    else hipLaunchKernelGGL((k_surface_measure<2, 2>), grid, block, 0, st, n_elements, n_out, elements, xyz, measure);
    return launched();
}

int knp_surface_get_info(int32_t* out, int n) {
    using namespace knp_surface;
    if (!out || n <= 0) return KNP_E_ARG;
    for (int k = 0; k < n && k < KNP_SI_COUNT; ++k) out[k] = g_info[k];
    return KNP_OK;
}

}  // extern "C"
