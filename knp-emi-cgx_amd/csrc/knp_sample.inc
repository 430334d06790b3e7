// Field sampling (knp_sample_*): P1 evaluation of nodal fields at arbitrary points -- grids, slices, probe lines -- with the point
// location done on the device, once per set of points (a "plan").
// Included at the end of knp_kernels.hip, after knp_diagnostics.inc (by_dim) and the host helpers (dev_upload, dev_free) it uses.
//
// Containment rule (that of cgx_hip/output.py::_barycentric, stated on the weights alone): cell T contains p iff all DIM+1 barycentric
// weights of p in T are >= -SAMPLE_TOL; among the containing cells the lowest cell index wins; the stored weights are clipped to [0, 1] and
// renormalised to sum 1.  Only owned cells of the requested side are searched.
//
// The host sorts the points into a uniform lattice of bins over their bounding box (the caller does, knp_sample_plan_create verifies).
//   k_sample_locate   one lane per cell: x0 and the inverse edge matrix once in registers, the cell's bounding box against the lattice
//                     (almost every cell of a 3D mesh leaves here when the points are a slice), then the points of the bins the box
//                     overlaps; every hit is a 32-bit integer atomicMin of the cell index on winner[point].  The minimum does not depend
//                     on the order of arrival: the same bits on every run.  Work: cells + tests inside overlapping bins.
//   k_sample_weights  one lane per point: the winner's weights again in closed form, clipped and renormalised; vertices, weights, side.
//   k_sample_gather   one lane per point, per record: out[f n + pt] = sum_a w_a F[f][v_a], a = 0..DIM in that order, F the field of the
//                     winning cell's side; points in no cell get `fill`.  The plan keeps its points in bin order, so neighbouring lanes
//                     read neighbouring vertices; the store goes to the caller's position of the point.
// Every loop is bounded by a mesh or plan size; there are no floating-point atomics and nothing waits inside a kernel.

static constexpr double SAMPLE_TOL = 1e-9;
static constexpr unsigned SAMPLE_NONE = 0xffffffffu;     // winner[] of a point no cell contains (the memset value)
static constexpr int SAMPLE_MAX_FIELDS = 16;             // field pointer pairs per launch of k_sample_gather (kernel arguments)
static constexpr uint8_t SAMPLE_OUTSIDE = 2;             // side[] of a point in no cell

struct SampleBins {
    double origin[3], size[3];
    int shape[3];
};
struct SampleFields {
    const double* fi[SAMPLE_MAX_FIELDS];
    const double* fe[SAMPLE_MAX_FIELDS];
};

// the simplex with vertices x[0..DIM]: lambda_{a+1}(p) = inv[a] . (p - x[0]), lambda_0 = 1 - sum; false when the cell is flat
template <int DIM>
struct SampleCell {
    double x0[DIM], inv[DIM][DIM];
    __device__ bool setup(const double (*x)[DIM]) {
        double e[DIM][DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a)
#pragma unroll
            for (int k = 0; k < DIM; ++k) e[a][k] = x[a + 1][k] - x[0][k];
#pragma unroll
        for (int k = 0; k < DIM; ++k) x0[k] = x[0][k];
        if constexpr (DIM == 2) {
            const double det = e[0][0] * e[1][1] - e[0][1] * e[1][0];
            if (!(det != 0.0)) return false;
            inv[0][0] = e[1][1] / det;  inv[0][1] = -e[1][0] / det;
            inv[1][0] = -e[0][1] / det; inv[1][1] = e[0][0] / det;
        } else {
            double cr[3][3];      // cr[a] = e[a+1] x e[a+2]: grad(lambda_{a+1}) = cr[a] / det
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double *u = e[(a + 1) % 3], *w = e[(a + 2) % 3];
                cr[a][0] = u[1] * w[2] - u[2] * w[1]; cr[a][1] = u[2] * w[0] - u[0] * w[2]; cr[a][2] = u[0] * w[1] - u[1] * w[0];
            }
            const double det = e[0][0] * cr[0][0] + e[0][1] * cr[0][1] + e[0][2] * cr[0][2];
            if (!(det != 0.0)) return false;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int k = 0; k < 3; ++k) inv[a][k] = cr[a][k] / det;
        }
        return true;
    }
    // the DIM+1 weights of p; true when the cell contains p
    __device__ bool weights(const double* p, double* w) const {
        double d[DIM], s = 0.0;
#pragma unroll
        for (int k = 0; k < DIM; ++k) d[k] = p[k] - x0[k];
        bool in = true;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < DIM; ++k) t += inv[a][k] * d[k];
            w[a + 1] = t;
            s += t;
            in = in && t >= -SAMPLE_TOL;
        }
        w[0] = 1.0 - s;
        return in && w[0] >= -SAMPLE_TOL;
    }
};

template <int DIM>
__device__ __forceinline__ void sample_load_cell(int c, const int32_t* __restrict__ cells, const double* __restrict__ coords, int* v,
                                                 double (*x)[DIM]) {
#pragma unroll
    for (int a = 0; a <= DIM; ++a) {
        v[a] = cells[(size_t)c * (DIM + 1) + a];
#pragma unroll
        for (int k = 0; k < DIM; ++k) x[a][k] = coords[(size_t)v[a] * DIM + k];
    }
}

template <int DIM>
__global__ void __launch_bounds__(NT) k_sample_locate(int n_cells, int side, const int32_t* __restrict__ cells,
                                                      const uint8_t* __restrict__ cell_side, const double* __restrict__ coords, SampleBins B,
                                                      const int32_t* __restrict__ bin_ptr, const double* __restrict__ pts,
                                                      unsigned* __restrict__ winner) {
    const int c = blockIdx.x * NT + threadIdx.x;
    if (c >= n_cells) return;
    if (side >= 0 && cell_side[c] != side) return;
    int v[DIM + 1];
    double x[DIM + 1][DIM];
    sample_load_cell<DIM>(c, cells, coords, v, x);
    // the bins the cell's bounding box overlaps.  A point the cell contains lies within DIM * SAMPLE_TOL extents of the box; the margin is
    // wider.  Host and device compute floor((x - origin) / size) with the same two IEEE operations, both monotone in x: a point never
    // falls in a bin below the one of the box's lower end or above the one of its upper end.  Indices are clamped as doubles first.
    int ilo[3] = {0, 0, 0}, ihi[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        double lo = x[0][k], hi = x[0][k];
#pragma unroll
        for (int a = 1; a <= DIM; ++a) {
            lo = fmin(lo, x[a][k]);
            hi = fmax(hi, x[a][k]);
        }
        const double m = 1e-8 * (hi - lo), top = (double)(B.shape[k] - 1);
        const double tlo = floor((lo - m - B.origin[k]) / B.size[k]), thi = floor((hi + m - B.origin[k]) / B.size[k]);
        if (thi < 0.0 || tlo > top + 1.0) return;      // (the last point of an axis may compute index shape: the host clamps it to shape - 1)
        ilo[k] = (int)fmin(fmax(tlo, 0.0), top);
        ihi[k] = (int)fmin(fmax(thi, 0.0), top);
    }
    SampleCell<DIM> T;
    if (!T.setup(x)) return;
    // bins are row-major, last axis fastest: the bins ilo..ihi of the last axis are consecutive, and so are their points
    for (int i0 = ilo[0]; i0 <= ihi[0]; ++i0) {
        for (int i1 = (DIM == 3 ? ilo[1] : 0); i1 <= (DIM == 3 ? ihi[1] : 0); ++i1) {
            const size_t row = DIM == 3 ? ((size_t)i0 * B.shape[1] + i1) * B.shape[2] : (size_t)i0 * B.shape[1];
            const int p0 = bin_ptr[row + ilo[DIM - 1]], p1 = bin_ptr[row + ihi[DIM - 1] + 1];
            for (int p = p0; p < p1; ++p) {
                double q[DIM], w[DIM + 1];
#pragma unroll
                for (int k = 0; k < DIM; ++k) q[k] = pts[(size_t)p * DIM + k];
                if (T.weights(q, w)) atomicMin(&winner[p], (unsigned)c);
            }
        }
    }
}

template <int DIM>
__global__ void __launch_bounds__(NT) k_sample_weights(int n, const unsigned* __restrict__ winner, const int32_t* __restrict__ cells,
                                                       const uint8_t* __restrict__ cell_side, const double* __restrict__ coords,
                                                       const double* __restrict__ pts, int32_t* __restrict__ cell_out,
                                                       int32_t* __restrict__ vert, double* __restrict__ wt, uint8_t* __restrict__ pside) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const unsigned cw = winner[i];
    int v[DIM + 1];
    double w[DIM + 1];
    uint8_t s = SAMPLE_OUTSIDE;
#pragma unroll
    for (int a = 0; a <= DIM; ++a) {
        v[a] = 0;
        w[a] = 0.0;
    }
    if (cw != SAMPLE_NONE) {
        const int c = (int)cw;
        double x[DIM + 1][DIM], q[DIM];
        sample_load_cell<DIM>(c, cells, coords, v, x);
#pragma unroll
        for (int k = 0; k < DIM; ++k) q[k] = pts[(size_t)i * DIM + k];
        SampleCell<DIM> T;
        T.setup(x);               // not flat: it won
        T.weights(q, w);
        double sum = 0.0;
#pragma unroll
        for (int a = 0; a <= DIM; ++a) {
            w[a] = fmin(fmax(w[a], 0.0), 1.0);
            sum += w[a];
        }
#pragma unroll
        for (int a = 0; a <= DIM; ++a) w[a] /= sum;
        s = cell_side[c] != 0 ? 1 : 0;
    }
    cell_out[i] = cw != SAMPLE_NONE ? (int)cw : -1;
    pside[i] = s;
#pragma unroll
    for (int a = 0; a <= DIM; ++a) {
        vert[(size_t)a * n + i] = v[a];
        wt[(size_t)a * n + i] = w[a];
    }
}

template <int DIM>
__global__ void __launch_bounds__(NT) k_sample_gather(int n, int n_f, const int32_t* __restrict__ perm, const int32_t* __restrict__ vert,
                                                      const double* __restrict__ wt, const uint8_t* __restrict__ pside, SampleFields F,
                                                      double fill, double* __restrict__ out) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    const int s = pside[i];
    const size_t o = (size_t)perm[i];
    if (s == SAMPLE_OUTSIDE) {
        for (int f = 0; f < n_f; ++f) out[(size_t)f * n + o] = fill;
        return;
    }
    int v[DIM + 1];
    double w[DIM + 1];
#pragma unroll
    for (int a = 0; a <= DIM; ++a) {
        v[a] = vert[(size_t)a * n + i];
        w[a] = wt[(size_t)a * n + i];
    }
    for (int f = 0; f < n_f; ++f) {
        const double* __restrict__ src = s ? F.fe[f] : F.fi[f];
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a <= DIM; ++a) acc += w[a] * src[v[a]];
        out[(size_t)f * n + o] = acc;
    }
}

static void sample_plan_free(KnpSamplePlan& P) {
    dev_free(P.d_perm); dev_free(P.d_vert); dev_free(P.d_w); dev_free(P.d_side);
    P = KnpSamplePlan();
}
void knp_sample_free(knp_ctx* ctx) {
    for (auto& P : ctx->sample_plans) sample_plan_free(P);
    ctx->sample_plans.clear();
}

static int sample_plan_of(knp_ctx* ctx, int32_t plan) {
    if (plan < 0 || plan >= (int)ctx->sample_plans.size() || !ctx->sample_plans[(size_t)plan].live) {
        ctx->err = "unknown sampling plan " + std::to_string(plan);
        return KNP_E_ARG;
    }
    return KNP_OK;
}

extern "C" {

int knp_sample_plan_create(knp_ctx* ctx, int32_t n_points, const double* pts, int32_t side, int32_t n_bins, const int32_t* bin_ptr,
                           const int32_t* bin_pts, const double* bin_origin, const double* bin_size, const int32_t* bin_shape, int32_t* plan) {
    CHECK_CTX(ctx);
    const KnpHostGraph& g = ctx->g;
    const int dim = g.dim, n = n_points;
    if (n_points <= 0) { ctx->err = "sampling plan: n_points must be positive"; return KNP_E_ARG; }
    if (!pts || !bin_ptr || !bin_pts || !bin_origin || !bin_size || !bin_shape || !plan) { ctx->err = "sampling plan: null array"; return KNP_E_ARG; }
    if (side < -1 || side > 1) { ctx->err = "sampling plan: side must be -1 (any cell), 0 (intracellular) or 1 (extracellular)"; return KNP_E_ARG; }
    int64_t nb = 1;
    SampleBins B;
    for (int k = 0; k < 3; ++k) {
        B.origin[k] = 0.0; B.size[k] = 1.0; B.shape[k] = 1;
        if (k >= dim) continue;
        if (bin_shape[k] < 1 || !(bin_size[k] > 0.0) || !std::isfinite(bin_size[k]) || !std::isfinite(bin_origin[k])) {
            ctx->err = "sampling plan: the bin lattice needs a finite origin, positive bin sizes and at least one bin per axis";
            return KNP_E_ARG;
        }
        B.origin[k] = bin_origin[k]; B.size[k] = bin_size[k]; B.shape[k] = bin_shape[k];
        nb *= bin_shape[k];
        if (nb > INT32_MAX - 1) { ctx->err = "sampling plan: too many bins"; return KNP_E_ARG; }
    }
    if (n_bins <= 0 || nb != n_bins) { ctx->err = "sampling plan: n_bins must be the product of bin_shape"; return KNP_E_ARG; }
    if (bin_ptr[0] != 0 || bin_ptr[n_bins] != n) { ctx->err = "sampling plan: bin_ptr must run from 0 to n_points"; return KNP_E_ARG; }
    for (int b = 0; b < n_bins; ++b)
        if (bin_ptr[b + 1] < bin_ptr[b]) { ctx->err = "sampling plan: bin_ptr must be non-decreasing"; return KNP_E_ARG; }
    // the points in bin order; every point once, finite, and in the bin its coordinates give
    std::vector<double> sorted((size_t)n * dim);
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int b = 0; b < n_bins; ++b)
        for (int i = bin_ptr[b]; i < bin_ptr[b + 1]; ++i) {
            const int p = bin_pts[i];
            if (p < 0 || p >= n || seen[(size_t)p]) { ctx->err = "sampling plan: bin_pts must list every point once"; return KNP_E_ARG; }
            seen[(size_t)p] = 1;
            int64_t lin = 0;
            for (int k = 0; k < dim; ++k) {
                const double x = pts[(size_t)p * dim + k];
                if (!std::isfinite(x)) { ctx->err = "sampling plan: point " + std::to_string(p) + " is not finite"; return KNP_E_ARG; }
                const double t = std::floor((x - B.origin[k]) / B.size[k]);
                lin = lin * B.shape[k] + (int64_t)std::min(std::max(t, 0.0), (double)(B.shape[k] - 1));
                sorted[(size_t)i * dim + k] = x;
            }
            if (lin != b) { ctx->err = "sampling plan: point " + std::to_string(p) + " is not in the bin its coordinates give"; return KNP_E_ARG; }
        }
    size_t slot = 0;
    while (slot < ctx->sample_plans.size() && ctx->sample_plans[slot].live) ++slot;
    if (slot == ctx->sample_plans.size()) ctx->sample_plans.emplace_back();
    KnpSamplePlan& P = ctx->sample_plans[slot];
    const int nv1 = dim + 1;
    double* d_pts = nullptr;
    int32_t *d_bin_ptr = nullptr, *d_cell = nullptr;
    unsigned* d_winner = nullptr;
    std::vector<int32_t> cell_b((size_t)n);
    std::vector<double> w_b((size_t)n * nv1);
    std::vector<uint8_t> side_b((size_t)n);
    const int rc = [&]() -> int {
        KCHK(dev_upload(ctx, &d_pts, sorted));
        KCHK(dev_upload_raw(ctx, &d_bin_ptr, bin_ptr, (size_t)n_bins + 1));
        KCHK(dev_upload_raw(ctx, &P.d_perm, bin_pts, (size_t)n));
        HIPCHK(hipMalloc((void**)&d_winner, (size_t)n * sizeof(unsigned)));
        HIPCHK(hipMalloc((void**)&d_cell, (size_t)n * sizeof(int32_t)));
        HIPCHK(hipMalloc((void**)&P.d_vert, (size_t)n * nv1 * sizeof(int32_t)));
        HIPCHK(hipMalloc((void**)&P.d_w, (size_t)n * nv1 * sizeof(double)));
        HIPCHK(hipMalloc((void**)&P.d_side, (size_t)n));
        HIPCHK(hipMemsetAsync(d_winner, 0xff, (size_t)n * sizeof(unsigned), ctx->stream));
        if (g.n_c_owned > 0) {
            by_dim(dim, [&](auto D) {
                hipLaunchKernelGGL(k_sample_locate<D()>, dim3((unsigned)((g.n_c_owned + NT - 1) / NT)), dim3(NT), 0, ctx->stream, g.n_c_owned,
                                   (int)side, ctx->d_cells, ctx->d_cell_side, ctx->d_coords, B, d_bin_ptr, d_pts, d_winner);
            });
            HIPCHK(hipGetLastError());
        }
        by_dim(dim, [&](auto D) {
            hipLaunchKernelGGL(k_sample_weights<D()>, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, ctx->stream, n, d_winner, ctx->d_cells,
                               ctx->d_cell_side, ctx->d_coords, d_pts, d_cell, P.d_vert, P.d_w, P.d_side);
        });
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipMemcpy(cell_b.data(), d_cell, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(w_b.data(), P.d_w, (size_t)n * nv1 * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(side_b.data(), P.d_side, (size_t)n, hipMemcpyDeviceToHost));
        return KNP_OK;
    }();
    dev_free(d_pts); dev_free(d_bin_ptr); dev_free(d_cell); dev_free(d_winner);
    if (rc != KNP_OK) {
        sample_plan_free(P);
        return rc;
    }
    // host copies in the caller's order (knp_sample_plan_get), and how many located points read each side's fields
    P.h_cell.assign((size_t)n, -1);
    P.h_w.assign((size_t)n * nv1, 0.0);
    P.n_side[0] = P.n_side[1] = 0;
    for (int i = 0; i < n; ++i) {
        const size_t p = (size_t)bin_pts[i];
        P.h_cell[p] = cell_b[(size_t)i];
        for (int a = 0; a < nv1; ++a) P.h_w[p * nv1 + a] = w_b[(size_t)a * n + i];
        if (side_b[(size_t)i] < 2) ++P.n_side[side_b[(size_t)i]];
    }
    P.n = n;
    P.live = true;
    *plan = (int32_t)slot;
    return KNP_OK;
}

int knp_sample_plan_get(knp_ctx* ctx, int32_t plan, int32_t* cell, double* w) {
    CHECK_CTX(ctx);
    KCHK(sample_plan_of(ctx, plan));
    if (!cell || !w) { ctx->err = "sampling plan: null output array"; return KNP_E_ARG; }
    const KnpSamplePlan& P = ctx->sample_plans[(size_t)plan];
    std::memcpy(cell, P.h_cell.data(), P.h_cell.size() * sizeof(int32_t));
    std::memcpy(w, P.h_w.data(), P.h_w.size() * sizeof(double));
    return KNP_OK;
}

int knp_sample(knp_ctx* ctx, int32_t plan, int32_t n_fields, const double* const* f_i, const double* const* f_e, double fill, double* out) {
    CHECK_CTX(ctx);
    KCHK(sample_plan_of(ctx, plan));
    const KnpSamplePlan& P = ctx->sample_plans[(size_t)plan];
    if (n_fields <= 0) { ctx->err = "knp_sample: n_fields must be positive"; return KNP_E_ARG; }
    if (!out) { ctx->err = "knp_sample: null output buffer"; return KNP_E_ARG; }
    for (int s = 0; s < 2; ++s) {
        if (P.n_side[s] == 0) continue;
        const double* const* fs = s ? f_e : f_i;
        for (int f = 0; f < n_fields; ++f)
            if (!fs || !fs[f]) {
                ctx->err = std::string("knp_sample: null ") + (s ? "extracellular" : "intracellular") + " field " + std::to_string(f) +
                           " although the plan has points in cells of that side";
                return KNP_E_ARG;
            }
    }
    const unsigned nblk = (unsigned)((P.n + NT - 1) / NT);
    for (int f0 = 0; f0 < n_fields; f0 += SAMPLE_MAX_FIELDS) {
        const int nf = std::min(SAMPLE_MAX_FIELDS, n_fields - f0);
        SampleFields F;
        for (int f = 0; f < SAMPLE_MAX_FIELDS; ++f) {
            F.fi[f] = (f < nf && f_i) ? f_i[f0 + f] : nullptr;
            F.fe[f] = (f < nf && f_e) ? f_e[f0 + f] : nullptr;
        }
        double* o = out + (size_t)f0 * P.n;
        by_dim(ctx->g.dim, [&](auto D) {
            hipLaunchKernelGGL(k_sample_gather<D()>, dim3(nblk), dim3(NT), 0, ctx->stream, P.n, nf, P.d_perm, P.d_vert, P.d_w, P.d_side, F, fill, o);
        });
        HIPCHK(hipGetLastError());
    }
    return KNP_OK;
}

int knp_sample_plan_destroy(knp_ctx* ctx, int32_t plan) {
    CHECK_CTX(ctx);
    KCHK(sample_plan_of(ctx, plan));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // a record in flight may still read the plan
    sample_plan_free(ctx->sample_plans[(size_t)plan]);
    return KNP_OK;
}

}  // extern "C"
