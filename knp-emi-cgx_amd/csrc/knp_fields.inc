// Derived fields: the value of a functional's program on every cell or facet (knp_functional_eval_items,
// knp_membrane_functional_eval_items) and the measure-weighted average of such per-item values onto the vertices (knp_project_*).
// Linear forms: the load vector of a functional's program on every cell or facet (knp_functional_eval_load,
// knp_membrane_functional_eval_load), the sum of those onto the vertices (knp_scatter_*) and its addition to the right-hand side of a
// step (knp_rhs_add_load).
// Included at the end of knp_kernels.hip, after knp_functional.inc and knp_membrane_functional.inc, whose plans, kernels and fn_eval
// the per-item evaluation uses, and after knp_dispatch.hpp (with_lanes).
//
// Per-item evaluation.  k_functional / k_membrane_functional instantiated with ITEMS: the body is the functionals' own (fn_lane,
// fn_load_fields, the derivative slots, the quadrature loop of fn_integrate), the end is one store per live lane of the item's mean
// sum_q q_w[q] OUT_j at out[i n_out + j], i the item's place in the plan's list.  The measure is not applied and the tag keys are not
// read.  The LDS of a block is the interpreter's register file [n_regs][FN_BT] and the constants, as for a functional, without the
// segmented scan's arrays.
//
// Projection.  A plan holds the inverted index of an item -> vertices table: per vertex the items that contain it, ascending, with
// each entry's measure next to it, and 1 / (sum of the list's measures).  The work is cut into units: a list of at most PROJ_SPLIT
// entries is one unit (an empty list too: it writes `fill`), a longer list is cut into chunks of PROJ_SPLIT entries, one unit each.
//   k_project<L, NOUT>        one unit per group of L lanes, NT / L units per block.  Lane l adds the entries l, l + L, .. of the unit
//                             in that order, then the lanes are combined by the fixed tree __shfl_down by L/2, .., 1.  Lane 0 writes
//                             out[j][v] = sum * inv[v] (or fill), or, for a chunk, the sum into the chunk's slot of the partials.
//   k_project_combine<NOUT>   one lane per split list: adds the list's partials in chunk order, writes out[j][v] = sum * inv[v].
// No atomics and no order that depends on the launch: the same inputs give the same bits on every run.
// L is chosen at create from the mean length of the non-empty lists: the smallest power of two that is not below it, within 2 .. 32
// (with_lanes<2, 32>).
//
// Sum-only gather (knp_scatter_*).  The same plan and the same two kernels with SUM: an entry is (item i, local vertex a) and the
// plan's item array holds i nv + a, which is the entry's place in values [n_items][nv][NOUT]; the weight is 1, there is no inv, an
// empty list writes 0.  out[j][v] = sum over v's entries, i ascending, of values[(i nv + a) NOUT + j]: the assembly of the element
// vectors of FN_LOAD into a nodal vector, without atomics.
//   k_rhs_add_load            one lane per owned node: b[4 node + field] += scale load[node_vertex[node]] on the nodes of one side.

static constexpr int PROJ_SPLIT = 512;      // entries per unit at most: longer vertex lists are cut into chunks of this many

template <int L, int NOUT, bool SUM = false>
__global__ void __launch_bounds__(NT) k_project(int n_units, const int32_t* __restrict__ ubeg, const int32_t* __restrict__ uvert,
                                                const int32_t* __restrict__ uslot, const int32_t* __restrict__ item,
                                                const double* __restrict__ meas, const double* __restrict__ inv,
                                                const double* __restrict__ values, double fill, int n_vertices, double* __restrict__ out,
                                                double* __restrict__ partial) {
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
    const int u = (int)(t / L), lane = (int)(t % L);
    const bool live = u < n_units;
    const int uu = live ? u : n_units - 1;      // idle groups of the last block shadow the last unit: the shuffles stay whole
    const int b = ubeg[uu], e = ubeg[uu + 1];
    double acc[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) acc[j] = 0.0;
    for (int p = b + lane; p < e; p += L) {
        const int i = item[p];
        if constexpr (SUM) {
#pragma unroll
            for (int j = 0; j < NOUT; ++j) acc[j] += values[(size_t)i * NOUT + j];
        } else {
            const double m = meas[p];
#pragma unroll
            for (int j = 0; j < NOUT; ++j) acc[j] += m * values[(size_t)i * NOUT + j];
        }
    }
#pragma unroll
    for (int d = L / 2; d > 0; d >>= 1) {
#pragma unroll
        for (int j = 0; j < NOUT; ++j) acc[j] += __shfl_down(acc[j], d, L);
    }
    if (live && lane == 0) {
        const int v = uvert[u], slot = uslot[u];
        if (slot < 0) {
            if constexpr (SUM) {      // an empty list has added nothing: 0
#pragma unroll
                for (int j = 0; j < NOUT; ++j) out[(size_t)j * n_vertices + v] = acc[j];
            } else {
                const double s = inv[v];
#pragma unroll
                for (int j = 0; j < NOUT; ++j) out[(size_t)j * n_vertices + v] = e > b ? acc[j] * s : fill;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NOUT; ++j) partial[(size_t)slot * NOUT + j] = acc[j];
        }
    }
}

template <int NOUT, bool SUM = false>
__global__ void __launch_bounds__(NT) k_project_combine(int n_split, const int32_t* __restrict__ svert, const int32_t* __restrict__ sptr,
                                                        const double* __restrict__ partial, const double* __restrict__ inv, int n_vertices,
                                                        double* __restrict__ out) {
    const int k = blockIdx.x * NT + threadIdx.x;
    if (k >= n_split) return;
    const int v = svert[k];
    double acc[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) acc[j] = 0.0;
    for (int c = sptr[k]; c < sptr[k + 1]; ++c) {
#pragma unroll
        for (int j = 0; j < NOUT; ++j) acc[j] += partial[(size_t)c * NOUT + j];
    }
    if constexpr (SUM) {
#pragma unroll
        for (int j = 0; j < NOUT; ++j) out[(size_t)j * n_vertices + v] = acc[j];
    } else {
        const double s = inv[v];
#pragma unroll
        for (int j = 0; j < NOUT; ++j) out[(size_t)j * n_vertices + v] = acc[j] * s;
    }
}

__global__ void __launch_bounds__(NT) k_rhs_add_load(int n_nodes_owned, const int32_t* __restrict__ node_vertex,
                                                     const uint8_t* __restrict__ node_side, int field, int side, double scale,
                                                     const double* __restrict__ load, double* __restrict__ b) {
    const int n = blockIdx.x * NT + threadIdx.x;
    if (n >= n_nodes_owned || node_side[n] != side) return;
    b[(size_t)4 * n + field] += scale * load[node_vertex[n]];
}

static void project_free_plan(KnpProjection& P) {
    dev_free(P.d_ubeg); dev_free(P.d_uvert); dev_free(P.d_uslot); dev_free(P.d_item); dev_free(P.d_meas); dev_free(P.d_inv);
    dev_free(P.d_svert); dev_free(P.d_sptr); dev_free(P.d_partial);
    P = KnpProjection();
}
void knp_project_free(knp_ctx* ctx) {
    for (auto* plans : {&ctx->projections, &ctx->scatters}) {
        for (auto& P : *plans) project_free_plan(P);
        plans->clear();
    }
}
// A kind of gather is its name in the error texts and its table of the context, like a kind of functional: the ids of the two are
// apart.  A scatter (sum-only) plan has no measures and no inv.
struct ProjKind {
    const char* name;
    std::vector<KnpProjection>& plans;
    bool sum;
};
static ProjKind proj_average(knp_ctx* ctx) { return {"projection", ctx->projections, false}; }
static ProjKind proj_sum(knp_ctx* ctx) { return {"scatter", ctx->scatters, true}; }
static int project_of(knp_ctx* ctx, const ProjKind& kind, int32_t id) {
    if (id < 0 || id >= (int)kind.plans.size() || !kind.plans[(size_t)id].live) {
        ctx->err = "unknown " + std::string(kind.name) + " " + std::to_string(id);
        return KNP_E_ARG;
    }
    return KNP_OK;
}

// Create of either kind: the inverted index of item_vertices.  An averaging plan keeps every entry's item and measure and 1 / (sum of a
// list's measures); a sum-only plan (measure is not read) keeps every entry's place i nv + a in [n_items][nv] and nothing else.
static int project_create(knp_ctx* ctx, const ProjKind& kind, int32_t n_items, int32_t nv, const int32_t* item_vertices, const double* measure,
                          int32_t* id) {
    const int n_v = ctx->g.n_v;
    const std::string pre = std::string(kind.name) + ": ";
    if (!id || n_items < 0 || (n_items > 0 && (!item_vertices || (!kind.sum && !measure)))) { ctx->err = pre + "null argument or negative item count"; return KNP_E_ARG; }
    if (nv < 2 || nv > 4) { ctx->err = pre + "nv must be 2..4"; return KNP_E_ARG; }
    if ((int64_t)n_items * nv > INT32_MAX) { ctx->err = pre + "more than 2^31 - 1 entries"; return KNP_E_ARG; }
    std::vector<int32_t> ptr((size_t)n_v + 1, 0);
    for (int i = 0; i < n_items; ++i) {
        if (!kind.sum && !(std::isfinite(measure[i]) && measure[i] > 0.0)) { ctx->err = pre + "the measure of item " + std::to_string(i) + " is not finite and positive"; return KNP_E_ARG; }
        const int32_t* w = item_vertices + (size_t)i * nv;
        for (int a = 0; a < nv; ++a) {
            if (w[a] < 0 || w[a] >= n_v) { ctx->err = pre + "item " + std::to_string(i) + " lists a vertex outside 0 .. n_vertices-1"; return KNP_E_ARG; }
            for (int b = 0; b < a; ++b)
                if (w[b] == w[a]) { ctx->err = pre + "item " + std::to_string(i) + " lists a vertex twice"; return KNP_E_ARG; }
            ++ptr[(size_t)w[a] + 1];
        }
    }
    for (int v = 0; v < n_v; ++v) ptr[(size_t)v + 1] += ptr[(size_t)v];
    const int n_entries = ptr[(size_t)n_v];
    std::vector<int32_t> item((size_t)n_entries), fillp(ptr.begin(), ptr.end() - 1);
    std::vector<double> meas(kind.sum ? 0 : (size_t)n_entries), inv(kind.sum ? 0 : (size_t)n_v, 0.0);
    for (int i = 0; i < n_items; ++i)      // items ascending: every list comes out in ascending item order
        for (int a = 0; a < nv; ++a) {
            const int p = fillp[(size_t)item_vertices[(size_t)i * nv + a]]++;
            item[(size_t)p] = kind.sum ? i * nv + a : i;
            if (!kind.sum) meas[(size_t)p] = measure[i];
        }
    KnpProjection P;
    std::vector<int32_t> ubeg, uvert, uslot, svert, sptr(1, 0);
    int64_t n_nonempty = 0;
    for (int v = 0; v < n_v; ++v) {
        const int b = ptr[(size_t)v], len = ptr[(size_t)v + 1] - b;
        if (!kind.sum) {
            double s = 0.0;
            for (int p = b; p < b + len; ++p) s += meas[(size_t)p];
            inv[(size_t)v] = len ? 1.0 / s : 0.0;
        }
        n_nonempty += len > 0;
        P.longest = std::max(P.longest, len);
        if (len <= PROJ_SPLIT) {
            ubeg.push_back(b); uvert.push_back(v); uslot.push_back(-1);
        } else {
            for (int c = 0; c < len; c += PROJ_SPLIT) {
                ubeg.push_back(b + c); uvert.push_back(v); uslot.push_back(P.n_slots++);
            }
            svert.push_back(v);
            sptr.push_back(P.n_slots);
        }
    }
    ubeg.push_back(n_entries);
    P.n_items = n_items;
    P.n_units = (int)uvert.size();
    P.n_split = (int)svert.size();
    const double mean = n_nonempty ? (double)n_entries / (double)n_nonempty : 0.0;
    P.lanes = 2;
    while (P.lanes < 32 && (double)P.lanes < mean) P.lanes *= 2;
    const int rc = [&]() -> int {
        KCHK(dev_upload(ctx, &P.d_ubeg, ubeg));
        KCHK(dev_upload(ctx, &P.d_uvert, uvert));
        KCHK(dev_upload(ctx, &P.d_uslot, uslot));
        KCHK(dev_upload(ctx, &P.d_item, item));
        if (!kind.sum) {
            KCHK(dev_upload(ctx, &P.d_meas, meas));
            KCHK(dev_upload(ctx, &P.d_inv, inv));
        }
        KCHK(dev_upload(ctx, &P.d_svert, svert));
        KCHK(dev_upload(ctx, &P.d_sptr, sptr));
        HIPCHK(hipMalloc((void**)&P.d_partial, std::max<size_t>((size_t)P.n_slots * 3, 1) * sizeof(double)));
        return KNP_OK;
    }();
    if (rc != KNP_OK) {
        project_free_plan(P);
        return rc;
    }
    P.live = true;
    size_t slot = 0;
    while (slot < kind.plans.size() && kind.plans[slot].live) ++slot;
    if (slot == kind.plans.size()) kind.plans.emplace_back();
    kind.plans[slot] = P;
    *id = (int32_t)slot;
    return KNP_OK;
}

static int project_apply(knp_ctx* ctx, const ProjKind& kind, int32_t id, const double* values, int32_t n_out, double fill, double* out) {
    KCHK(project_of(ctx, kind, id));
    const KnpProjection& P = kind.plans[(size_t)id];
    const std::string pre = std::string(kind.name) + ": ";
    if (n_out < 1 || n_out > 3) { ctx->err = pre + "n_out must be 1..3"; return KNP_E_ARG; }
    if (!out || (P.n_items > 0 && !values)) { ctx->err = pre + "null values or null output buffer"; return KNP_E_ARG; }
    const int n_v = ctx->g.n_v;
    if (P.n_units == 0) return KNP_OK;      // a mesh without vertices
    auto run = [&](auto NOUT, auto SUM) {
        with_lanes<2, 32>(P.lanes, [&](auto L) {
            hipLaunchKernelGGL((k_project<L(), NOUT(), SUM()>), dim3(nblocks((int64_t)P.n_units * L())), dim3(NT), 0, ctx->stream, P.n_units,
                               P.d_ubeg, P.d_uvert, P.d_uslot, P.d_item, P.d_meas, P.d_inv, values, fill, n_v, out, P.d_partial);
        });
        if (P.n_split > 0)
            hipLaunchKernelGGL((k_project_combine<NOUT(), SUM()>), dim3(nblocks(P.n_split)), dim3(NT), 0, ctx->stream, P.n_split, P.d_svert,
                               P.d_sptr, P.d_partial, P.d_inv, n_v, out);
    };
    auto by_out = [&](auto SUM) {
        if (n_out == 1) run(std::integral_constant<int, 1>(), SUM);
        else if (n_out == 2) run(std::integral_constant<int, 2>(), SUM);
        else run(std::integral_constant<int, 3>(), SUM);
    };
    if (kind.sum) by_out(std::true_type());
    else by_out(std::false_type());
    HIPCHK(hipGetLastError());
    return KNP_OK;
}

static int project_get_info(const std::vector<KnpProjection>& plans, int32_t id, int32_t* out, int n) {
    if (!out || n <= 0) return KNP_E_ARG;
    if (id < 0 || id >= (int)plans.size() || !plans[(size_t)id].live) return KNP_E_ARG;
    const KnpProjection& P = plans[(size_t)id];
    int32_t v[KNP_PI_COUNT];
    v[KNP_PI_LANES] = P.lanes;
    v[KNP_PI_LONGEST] = P.longest;
    v[KNP_PI_N_SPLIT] = P.n_split;
    v[KNP_PI_N_UNITS] = P.n_units;
    v[KNP_PI_SPLIT] = PROJ_SPLIT;
    for (int i = 0; i < n && i < KNP_PI_COUNT; ++i) out[i] = v[i];
    return KNP_OK;
}

static int project_destroy(knp_ctx* ctx, const ProjKind& kind, int32_t id) {
    KCHK(project_of(ctx, kind, id));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // an application in flight may still read the plan
    project_free_plan(kind.plans[(size_t)id]);
    return KNP_OK;
}

extern "C" {

int knp_functional_eval_items(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out) {
    CHECK_CTX(ctx);
    return functional_eval<FN_ITEMS>(ctx, id, fields, out);
}

int knp_membrane_functional_eval_items(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out) {
    CHECK_CTX(ctx);
    return membrane_functional_eval<FN_ITEMS>(ctx, id, fields, out);
}

int knp_project_create(knp_ctx* ctx, int32_t n_items, int32_t nv, const int32_t* item_vertices, const double* measure, int32_t* id) {
    CHECK_CTX(ctx);
    return project_create(ctx, proj_average(ctx), n_items, nv, item_vertices, measure, id);
}

int knp_project_apply(knp_ctx* ctx, int32_t id, const double* values, int32_t n_out, double fill, double* out) {
    CHECK_CTX(ctx);
    return project_apply(ctx, proj_average(ctx), id, values, n_out, fill, out);
}

int knp_project_get_info(const knp_ctx* ctx, int32_t id, int32_t* out, int n) {
    if (!ctx) return KNP_E_ARG;
    return project_get_info(ctx->projections, id, out, n);
}

int knp_project_destroy(knp_ctx* ctx, int32_t id) {
    CHECK_CTX(ctx);
    return project_destroy(ctx, proj_average(ctx), id);
}

int knp_functional_eval_load(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out) {
    CHECK_CTX(ctx);
    return functional_eval<FN_LOAD>(ctx, id, fields, out);
}

int knp_membrane_functional_eval_load(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out) {
    CHECK_CTX(ctx);
    return membrane_functional_eval<FN_LOAD>(ctx, id, fields, out);
}

int knp_scatter_create(knp_ctx* ctx, int32_t n_items, int32_t nv, const int32_t* item_vertices, int32_t* id) {
    CHECK_CTX(ctx);
    return project_create(ctx, proj_sum(ctx), n_items, nv, item_vertices, nullptr, id);
}

int knp_scatter_apply(knp_ctx* ctx, int32_t id, const double* values, int32_t n_out, double* out) {
    CHECK_CTX(ctx);
    return project_apply(ctx, proj_sum(ctx), id, values, n_out, 0.0, out);
}

int knp_scatter_get_info(const knp_ctx* ctx, int32_t id, int32_t* out, int n) {
    if (!ctx) return KNP_E_ARG;
    return project_get_info(ctx->scatters, id, out, n);
}

int knp_scatter_destroy(knp_ctx* ctx, int32_t id) {
    CHECK_CTX(ctx);
    return project_destroy(ctx, proj_sum(ctx), id);
}

int knp_rhs_add_load(knp_ctx* ctx, int32_t field, int32_t side, double scale, const double* load, double* b) {
    CHECK_CTX(ctx);
    const KnpHostGraph& g = ctx->g;
    if (field < 0 || field > 3) { ctx->err = "rhs_add_load: field must be 0..3"; return KNP_E_ARG; }
    if (side < 0 || side > 1) { ctx->err = "rhs_add_load: side must be 0 (intra) or 1 (extra)"; return KNP_E_ARG; }
    if (!load || !b) { ctx->err = "rhs_add_load: null load or null b"; return KNP_E_ARG; }
    if (g.n_nodes > g.n_nodes_owned) { ctx->err = "rhs_add_load: one GPU only (the context has ghost nodes)"; return KNP_E_STATE; }
    side_discard(ctx);      // a preconditioned norm in flight on the side stream reads b
    if (g.n_nodes_owned > 0)
        hipLaunchKernelGGL(k_rhs_add_load, dim3(nblocks(g.n_nodes_owned)), dim3(NT), 0, ctx->stream, g.n_nodes_owned, ctx->d_node_vertex,
                           ctx->d_node_side, field, side, scale, load, b);
    HIPCHK(hipGetLastError());
    return KNP_OK;
}

}  // extern "C"
