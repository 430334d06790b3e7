// The EMI model (reference src/CGx/EMI): two potentials with constant conductivities, one unknown per node of the graph knp_create
// built.  Included at the end of knp_kernels.hip; uses its helpers (block_sum, run_program, amg_vcycle, read_slots, dev_upload...).
//
//   A = [ dt sigma_i K_i + C_M M_Gamma     -C_M M_Gamma              ]        (EMIx_problem.py:152-157)
//       [ -C_M M_Gamma                     dt sigma_e K_e + C_M M_Gamma ]
//
// Storage: val[p] for every same-side node pair p (the order of pair_col) and xval[s] for every membrane vertex pair s, the entry of
// both of its rows towards the other side's node (gx_i / gx_e): 8 B + the 4-byte column that the graph already holds.
//
// One PCG iteration (knp_emi_cg_solve), every scalar on the device:
//   k_emi_spmv<DOT>   q = A p and the per-block partial sums of p . q
//   k_emi_xr          every block sums those partials in the same order -> alpha = (r.z) / (p.q); x += alpha p, r -= alpha q;
//                     with no / Jacobi preconditioning also z = Dinv r and the partial sums of r.z, z.z, r.r, sum z, sum r
//   [V-cycle + k_emi_dots with KNP_PC_AMG]
//   k_emi_p           every block sums the five partial rows -> mean of z (null space), beta, the norm; p = (z - mean) + beta p;
//                     block 0 publishes the norm to pinned host memory
// The next q = A p is enqueued before the host waits for the norm, so the read-back hides behind it.

static constexpr int EMI_SPMV_BLOCKS = 1024;   // blocks of the SpMV = partial sums of p . q
static constexpr int EMI_VEC_BLOCKS = 512;     // blocks of the vector kernels = partial sums per row of the five inner products
static constexpr int EMI_ROW0 = EMI_SPMV_BLOCKS;   // d_partial: [0, 1024) p.q | 1024 + 512 k, k = 0..4: r.z z.z r.r sum z sum r
static constexpr int EMI_BT = 128;             // facets per block of the membrane kernel (LDS register file [n_regs][EMI_BT])
static constexpr int EMI_SLOT = 0;             // reduction slots 0..3: {norm^2, r.z, breakdown flag, reference norm^2}
static_assert(EMI_ROW0 + 5 * EMI_VEC_BLOCKS <= RED_SLOTS * RED_BLOCKS, "partial-sum buffer");

struct EmiAux { const double* a[KNP_MAX_AUX]; };

// sum of nb values in a fixed order, the same in every block that calls it; valid in every thread
__device__ __forceinline__ double emi_sum_all(const double* __restrict__ v, int nb, double* sm) {
    double a = 0.0;
    for (int i = threadIdx.x; i < nb; i += NT) a += v[i];
    a = block_sum(a, sm);
    __syncthreads();
    if (threadIdx.x == 0) sm[0] = a;
    __syncthreads();
    a = sm[0];
    __syncthreads();
    return a;
}

// ---- matrix -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) k_emi_pairs(int64_t n_pairs, const int32_t* __restrict__ pair_row, const uint8_t* __restrict__ node_side,
                                                  const double* __restrict__ pair_K, double a_i, double a_e, double* __restrict__ val) {
    const int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (p < n_pairs) val[p] = (node_side[pair_row[p]] ? a_e : a_i) * pair_K[p];
}
// M_Gamma entry of a membrane vertex pair from its facets (P1 facet mass matrix |F| (1 + delta_ab) / (d (d + 1))); every same-side
// slot belongs to exactly one membrane pair, so the plain += does not race
__global__ void __launch_bounds__(NT) k_emi_gamma(int64_t n_gp, int dim, double C_M, const int32_t* __restrict__ grow,
                                                  const int32_t* __restrict__ gv_node_i, const int32_t* __restrict__ gv_node_e,
                                                  const int32_t* __restrict__ gq_i, const int32_t* __restrict__ gq_e,
                                                  const int32_t* __restrict__ gcptr, const int32_t* __restrict__ gc_facet,
                                                  const int32_t* __restrict__ gc_lab, const double* __restrict__ fmeas,
                                                  const int32_t* __restrict__ pair_ptr, double* __restrict__ val, double* __restrict__ xval) {
    const int64_t s = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (s >= n_gp) return;
    const int A = grow[s];
    const double mref = 1.0 / (dim * (dim + 1.0));
    double m0 = 0.0;
    for (int c = gcptr[s]; c < gcptr[s + 1]; ++c) {
        const int la = gc_lab[c] >> 2, lb = gc_lab[c] & 3;
        m0 += fmeas[gc_facet[c]] * mref * (la == lb ? 2.0 : 1.0);
    }
    m0 *= C_M;
    val[(size_t)pair_ptr[gv_node_i[A]] + gq_i[s]] += m0;
    val[(size_t)pair_ptr[gv_node_e[A]] + gq_e[s]] += m0;
    xval[s] = -m0;
}
__global__ void __launch_bounds__(NT) k_emi_dinv(int n, const int32_t* __restrict__ pair_ptr, const int32_t* __restrict__ pair_col,
                                                 const double* __restrict__ val, const uint8_t* __restrict__ mask, double* __restrict__ dinv) {
    const int node = blockIdx.x * NT + threadIdx.x;
    if (node >= n) return;
    double d = 0.0;
    for (int p = pair_ptr[node]; p < pair_ptr[node + 1]; ++p)
        if (pair_col[p] == node) d = val[p];
    dinv[node] = (mask[node] || d == 0.0) ? 1.0 : 1.0 / d;
}

// ---- SpMV: a G-lane group per node over its pair row plus the entries towards the other side (the lane-group idiom of
// k_spmv_node).  Grid-stride with a fixed grid, so that the partial sums of x . (A x) (DOT) have a fixed order.
//   MODE 0: y = A x    MODE 1: y = b - A x     BC: Dirichlet nodes are identity rows and columns
template <int G, int MODE, bool BC, bool DOT>
__global__ void __launch_bounds__(NT)
k_emi_spmv(int n, const int32_t* __restrict__ pair_ptr, const int32_t* __restrict__ pair_col, const double* __restrict__ val,
           const int32_t* __restrict__ node_gv, const uint8_t* __restrict__ node_side, const int32_t* __restrict__ gptr,
           const int32_t* __restrict__ gx_i, const int32_t* __restrict__ gx_e, const double* __restrict__ xval,
           const uint8_t* __restrict__ mask, const double* __restrict__ x, const double* __restrict__ b, double* __restrict__ y,
           double* __restrict__ partial) {
    __shared__ double sm[NT / 64];
    const int lane = threadIdx.x & (G - 1);
    const int groups = gridDim.x * (NT / G);
    const int trips = (n + groups - 1) / groups;   // the same for every lane: the shuffles below are executed by whole waves
    double acc = 0.0;
    for (int t = 0; t < trips; ++t) {
        const int node = t * groups + (blockIdx.x * NT + threadIdx.x) / G;
        const bool live = node < n;
        const bool bcrow = BC && live && mask[node];
        double s = 0.0;
        if (live && !bcrow) {
            const int p1 = pair_ptr[node + 1];
            for (int p = pair_ptr[node] + lane; p < p1; p += G) {
                const int j = pair_col[p];
                double xv = x[j];
                if (BC && mask[j]) xv = 0.0;
                s += val[p] * xv;
            }
            const int A = node_gv[node];
            if (A >= 0) {
                const int32_t* __restrict__ gx = node_side[node] ? gx_e : gx_i;
                const int q1 = gptr[A + 1];
                for (int q = gptr[A] + lane; q < q1; q += G) {
                    const int j = gx[q];
                    double xv = x[j];
                    if (BC && mask[j]) xv = 0.0;
                    s += xval[q] * xv;
                }
            }
        }
#pragma unroll
        for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, G);
        if (lane == 0 && live) {
            if (bcrow) s = x[node];
            y[node] = MODE ? b[node] - s : s;
            if (DOT) acc += x[node] * s;
        }
    }
    if (DOT) {
        acc = block_sum(acc, sm);
        if (threadIdx.x == 0) partial[blockIdx.x] = acc;
    }
}

// ---- right-hand side ----------------------------------------------------------------------------------------------------------
// (a) one thread per membrane facet: fvec[a * n_g + f] = |F| sum_q w_q lambda_a(q) (C_M phi_m(q) - dt I_ch(q)), I_ch = the sum of
// the outputs of the facet's program at the point.  The interpreter needs wave-uniform instruction words: every program some lane of
// the wave uses is run by the whole wave and each lane keeps the value of its own.
template <int DIM, bool FUNCS = false>
__global__ void __launch_bounds__(EMI_BT)
k_emi_facets(int n_g, int n_q, double C_M, double dt, const int32_t* __restrict__ fv, const double* __restrict__ fmeas,
             const double* __restrict__ qp, const double* __restrict__ qw, const double* __restrict__ phim, EmiAux aux, int n_aux,
             const double* __restrict__ coords, const int32_t* __restrict__ gamma_prog, int n_progs,
             const int32_t* const* __restrict__ prog_code, const int32_t* __restrict__ prog_len,
             const double* const* __restrict__ prog_consts, double* __restrict__ fvec) {
    extern __shared__ double emi_regs[];
    const int i = blockIdx.x * EMI_BT + threadIdx.x;
    const bool live = i < n_g;
    const int f = live ? i : n_g - 1;      // idle lanes shadow the last facet with weight zero: the wave stays uniform
    int v[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) v[a] = fv[(size_t)f * DIM + a];
    const double meas = live ? fmeas[f] : 0.0;
    const int prog = gamma_prog[f];
    double* reg = emi_regs + threadIdx.x;
    double acc[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) acc[a] = 0.0;
    for (int q = 0; q < n_q; ++q) {
        double lam[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) lam[a] = qp[q * DIM + a];
        double kq[1][3] = {{0.0, 0.0, 0.0}}, phq[1] = {0.0}, auxq[1][KNP_MAX_AUX], xq[1][3];
#pragma unroll
        for (int a = 0; a < DIM; ++a) phq[0] += lam[a] * phim[v[a]];
        for (int k = 0; k < n_aux; ++k) {
            double t = 0.0;
#pragma unroll
            for (int a = 0; a < DIM; ++a) t += lam[a] * aux.a[k][v[a]];
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
        double I = 0.0;
        for (int pl = 0; pl < n_progs; ++pl) {
            if (__ballot(prog == pl) == 0) continue;
            double Iout[1][3] = {{0.0, 0.0, 0.0}};
            run_program<1, EMI_BT, FUNCS>(prog_code[pl], prog_len[pl], prog_consts[pl], kq, kq, phq, auxq, xq, Iout, reg);
            if (prog == pl) I = Iout[0][0] + Iout[0][1] + Iout[0][2];
        }
        const double w = qw[q] * meas * (C_M * phq[0] - dt * I);
#pragma unroll
        for (int a = 0; a < DIM; ++a) acc[a] += w * lam[a];
    }
    if (live) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) fvec[(size_t)a * n_g + f] = acc[a];
    }
}
// (b) a G-lane group per node: volume sources over its pair row, the membrane term gathered over the facets of its vertex
// (gdiag / gcptr, as k_rhs does), the Dirichlet lifting b -= A g over the same row
template <int G>
__global__ void __launch_bounds__(NT)
k_emi_rhs(int n, int n_g, double dt, double scale, const int32_t* __restrict__ node_vertex, const uint8_t* __restrict__ node_side,
          const int32_t* __restrict__ pair_ptr, const int32_t* __restrict__ pair_col, const double* __restrict__ pair_M,
          const double* __restrict__ val, const double* __restrict__ f_i, const double* __restrict__ f_e,
          const int32_t* __restrict__ node_gv, const int32_t* __restrict__ gptr, const int32_t* __restrict__ gx_i,
          const int32_t* __restrict__ gx_e, const double* __restrict__ xval, const int32_t* __restrict__ gdiag,
          const int32_t* __restrict__ gcptr, const int32_t* __restrict__ gc_facet, const int32_t* __restrict__ gc_lab,
          const double* __restrict__ fvec, const uint8_t* __restrict__ mask /* null: no Dirichlet nodes */,
          const double* __restrict__ g, double* __restrict__ b) {
    const int node = (blockIdx.x * NT + threadIdx.x) / G;
    const int lane = threadIdx.x & (G - 1);
    const bool live = node < n;
    double s = 0.0;
    if (live) {
        const int side = node_side[node];
        const double* __restrict__ src = side ? f_e : f_i;
        const bool lift = mask && g && !mask[node];
        const int p1 = pair_ptr[node + 1];
        if (src || lift) {
            for (int p = pair_ptr[node] + lane; p < p1; p += G) {
                const int j = pair_col[p];
                if (src) s += dt * pair_M[p] * src[node_vertex[j]];
                if (lift && mask[j]) s -= val[p] * g[j];
            }
        }
        const int A = node_gv[node];
        if (A >= 0) {
            const int sd = gdiag[A];
            const double sg = side ? -scale : scale;
            for (int c = gcptr[sd] + lane; c < gcptr[sd + 1]; c += G)
                s += sg * fvec[(size_t)(gc_lab[c] >> 2) * n_g + gc_facet[c]];
            if (lift) {
                const int32_t* __restrict__ gx = side ? gx_e : gx_i;
                for (int q = gptr[A] + lane; q < gptr[A + 1]; q += G) {
                    const int j = gx[q];
                    if (mask[j]) s -= xval[q] * g[j];
                }
            }
        }
    }
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, G);
    if (lane == 0 && live) b[node] = (mask && mask[node]) ? (g ? g[node] : 0.0) : s;
}

// ---- vector kernels of the solver ---------------------------------------------------------------------------------------------
// partial sums of r.z, z.z, r.r, sum z, sum r per block (rows of EMI_VEC_BLOCKS behind `rows`)
__device__ __forceinline__ void emi_store_rows(double a0, double a1, double a2, double a3, double a4, double* __restrict__ rows, double* sm) {
    const double v[5] = {a0, a1, a2, a3, a4};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double t = block_sum(v[k], sm);
        if (threadIdx.x == 0) rows[k * EMI_VEC_BLOCKS + blockIdx.x] = t;
    }
}
__global__ void __launch_bounds__(NT) k_emi_dots(int n, const double* __restrict__ r, const double* __restrict__ z, double* __restrict__ rows) {
    __shared__ double sm[NT / 64];
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
    for (int e = blockIdx.x * NT + threadIdx.x; e < n; e += gridDim.x * NT) {
        const double rv = r[e], zv = z[e];
        a0 += rv * zv; a1 += zv * zv; a2 += rv * rv; a3 += zv; a4 += rv;
    }
    emi_store_rows(a0, a1, a2, a3, a4, rows, sm);
}
// PCK 0: z = r, 1: z = Dinv r (both with the partial sums), 2: the preconditioner is applied afterwards
template <int PCK>
__global__ void __launch_bounds__(NT)
k_emi_xr(int n, int nb_pq, const double* __restrict__ part_pq, double* __restrict__ st, int cur, const double* __restrict__ p,
         const double* __restrict__ q, const double* __restrict__ dinv, double* __restrict__ x, double* __restrict__ r,
         double* __restrict__ z, double* __restrict__ rows) {
    __shared__ double sm[NT / 64];
    const double pq = emi_sum_all(part_pq, nb_pq, sm);
    const bool ok = pq > 0.0;
    const double alpha = ok ? st[cur] / pq : 0.0;
    if (!ok && blockIdx.x == 0 && threadIdx.x == 0) st[2] = 1.0;     // breakdown: p . A p <= 0 or not a number
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
    for (int e = blockIdx.x * NT + threadIdx.x; e < n; e += gridDim.x * NT) {
        x[e] += alpha * p[e];
        const double rv = r[e] - alpha * q[e];
        r[e] = rv;
        if (PCK < 2) {
            const double zv = PCK == 1 ? dinv[e] * rv : rv;
            z[e] = zv;
            a0 += rv * zv; a1 += zv * zv; a2 += rv * rv; a3 += zv; a4 += rv;
        }
    }
    if (PCK < 2) emi_store_rows(a0, a1, a2, a3, a4, rows, sm);
}
// the three inner products with the mean of z taken out (null space: z' = z - mu, r.z' = r.z - mu sum r, z'.z' = z.z - n mu^2)
// z.z - n mu^2 cancels when z is nearly constant: below EMI_CANCEL of z.z the difference is rounding noise, `cancel` says so and the
// solve ends with the breakdown flag (as p . A p <= 0 does) instead of reporting a norm that the host would clamp to zero
static constexpr double EMI_CANCEL = 1e-8;
struct EmiNorms { double mu, beta, dp2; int cancel; };
__device__ __forceinline__ EmiNorms emi_norms(const double* __restrict__ rows, int nb, int n, int ns, int norm_type, double* sm) {
    double S[5];
    for (int k = 0; k < 5; ++k) S[k] = emi_sum_all(rows + k * EMI_VEC_BLOCKS, nb, sm);
    EmiNorms o;
    o.mu = ns ? S[3] / (double)n : 0.0;
    o.beta = S[0] - o.mu * S[4];
    const double zz = S[1] - (double)n * o.mu * o.mu;
    o.cancel = (ns && norm_type == 0 && zz < EMI_CANCEL * S[1]) ? 1 : 0;
    o.dp2 = norm_type == 0 ? zz : norm_type == 1 ? S[2] : fabs(o.beta);
    return o;
}
__device__ __forceinline__ void emi_publish(double* __restrict__ red, double* mirror, int slot, int count, const double* v,
                                            volatile int64_t* seq, int64_t seq_val) {
    for (int k = 0; k < count; ++k) {
        red[slot + k] = v[k];
        if (mirror) mirror[slot + k] = v[k];
    }
    if (seq) {
        __threadfence_system();
        *seq = seq_val;
    }
}
// p = (z - mu) + (beta / beta_old) p; block 0 keeps beta for the next iteration and publishes {norm^2, beta, breakdown flag}
__global__ void __launch_bounds__(NT)
k_emi_p(int n, int nb, const double* __restrict__ rows, int ns, int norm_type, int first, double* __restrict__ st, int cur,
        const double* __restrict__ z, double* __restrict__ p, double* __restrict__ red, double* mirror, volatile int64_t* seq, int64_t seq_val) {
    __shared__ double sm[NT / 64];
    const EmiNorms N = emi_norms(rows, nb, n, ns, norm_type, sm);
    const double bc = first ? 0.0 : N.beta / st[cur];
    for (int e = blockIdx.x * NT + threadIdx.x; e < n; e += gridDim.x * NT) p[e] = first ? z[e] - N.mu : (z[e] - N.mu) + bc * p[e];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[cur ^ 1] = N.beta;
        if (N.cancel) st[2] = 1.0;
        const double v[3] = {N.dp2, N.beta, st[2]};
        emi_publish(red, mirror, EMI_SLOT, 3, v, seq, seq_val);
    }
}
// one block: the norm of a pair (b, B b) into slot EMI_SLOT + 3 (the reference of the stopping test)
__global__ void __launch_bounds__(NT)
k_emi_ref(int n, int nb, const double* __restrict__ rows, int ns, int norm_type, double* __restrict__ red, double* mirror,
          volatile int64_t* seq, int64_t seq_val) {
    __shared__ double sm[NT / 64];
    const EmiNorms N = emi_norms(rows, nb, n, ns, norm_type, sm);
    const double ref2 = N.cancel ? nan("") : N.dp2;      // no usable reference norm: the host reports KNP_DIVERGED_NANORINF
    if (threadIdx.x == 0) emi_publish(red, mirror, EMI_SLOT + 3, 1, &ref2, seq, seq_val);
}
__global__ void __launch_bounds__(NT) k_emi_scale(int n, const double* __restrict__ d, const double* __restrict__ r, double* __restrict__ z) {
    for (int e = blockIdx.x * NT + threadIdx.x; e < n; e += gridDim.x * NT) z[e] = d ? d[e] * r[e] : r[e];
}
// Dirichlet nodes around the V-cycle: t = r with them zeroed (MODE 0), z = r on them (MODE 1)
template <int MODE>
__global__ void __launch_bounds__(NT) k_emi_mask(int n, const uint8_t* __restrict__ mask, const double* __restrict__ r, double* __restrict__ out) {
    for (int e = blockIdx.x * NT + threadIdx.x; e < n; e += gridDim.x * NT) {
        if (MODE == 0) out[e] = mask[e] ? 0.0 : r[e];
        else if (mask[e]) out[e] = r[e];
    }
}
// per-block partial sums of v alone (the mean of a vector: right-hand side, preconditioner output, first residual)
__global__ void __launch_bounds__(NT) k_emi_sum(int n, const double* __restrict__ v, double* __restrict__ row) {
    __shared__ double sm[NT / 64];
    double a = 0.0;
    for (int e = blockIdx.x * NT + threadIdx.x; e < n; e += gridDim.x * NT) a += v[e];
    a = block_sum(a, sm);
    if (threadIdx.x == 0) row[blockIdx.x] = a;
}
// v -= mean(v), the mean from the partial sums of row `row`
__global__ void __launch_bounds__(NT) k_emi_sub_mean(int n, int nb, const double* __restrict__ row, double* __restrict__ v) {
    __shared__ double sm[NT / 64];
    const double mu = emi_sum_all(row, nb, sm) / (double)n;
    for (int e = blockIdx.x * NT + threadIdx.x; e < n; e += gridDim.x * NT) v[e] -= mu;
}
__global__ void __launch_bounds__(NT)
k_emi_update(int n_v, const int32_t* __restrict__ node_i, const int32_t* __restrict__ node_e, int n, const double* __restrict__ x,
             double* __restrict__ phi_i, double* __restrict__ phi_e, double* __restrict__ phi_m) {
    const int v = blockIdx.x * NT + threadIdx.x;
    if (v >= n_v) return;
    const int ni = node_i[v], ne = node_e[v];
    const double a = (ni >= 0 && ni < n) ? x[ni] : 0.0, c = (ne >= 0 && ne < n) ? x[ne] : 0.0;
    phi_i[v] = a;
    phi_e[v] = c;
    phi_m[v] = a - c;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
void knp_emi_free(knp_ctx* ctx) {
    KnpEmi& E = ctx->emi;
    dev_free(E.d_val); dev_free(E.d_xval); dev_free(E.d_dinv); dev_free(E.d_mask);
    dev_free(E.d_r); dev_free(E.d_z); dev_free(E.d_p); dev_free(E.d_q); dev_free(E.d_t);
    dev_free(E.d_fvec); dev_free(E.d_st);
    E.ready = false;
}

static int emi_check(knp_ctx* ctx) {
    if (ctx->g.n_nodes != ctx->g.n_nodes_owned) { ctx->err = "the EMI model runs on one GPU only (the context has ghost nodes)"; return KNP_E_STATE; }
    if (!ctx->emi.ready) { ctx->err = "knp_emi_setup has not been called"; return KNP_E_STATE; }
    return KNP_OK;
}
static inline int emi_vec_blocks(int n) { return std::min(EMI_VEC_BLOCKS, nblocks(n)); }

template <int MODE, bool DOT>
static void emi_launch_spmv(knp_ctx* ctx, const double* x, const double* b, double* y) {
    const KnpEmi& E = ctx->emi;
    const int n = ctx->g.n_nodes_owned;
    constexpr int G = 8;
    const int nb = std::min(EMI_SPMV_BLOCKS, nblocks((int64_t)n * G));
    with_flag(E.n_bc > 0, [&](auto BC) {
        hipLaunchKernelGGL((k_emi_spmv<G, MODE, BC(), DOT>), dim3(nb), dim3(NT), 0, ctx->stream, n, ctx->d_pair_ptr, ctx->d_pair_col, E.d_val,
                           ctx->d_node_gv, ctx->d_node_side, ctx->d_gptr, ctx->d_gx_i, ctx->d_gx_e, E.d_xval, E.d_mask, x, b, y, ctx->d_partial);
    });
}
static inline int emi_spmv_blocks(const knp_ctx* ctx) { return std::min(EMI_SPMV_BLOCKS, nblocks((int64_t)ctx->g.n_nodes_owned * 8)); }

static int emi_write_dinv(knp_ctx* ctx) {
    KnpEmi& E = ctx->emi;
    const int n = ctx->g.n_nodes_owned;
    hipLaunchKernelGGL(k_emi_dinv, dim3(nblocks(n)), dim3(NT), 0, ctx->stream, n, ctx->d_pair_ptr, ctx->d_pair_col, E.d_val, E.d_mask, E.d_dinv);
    HIPCHK(hipGetLastError());
    return KNP_OK;
}

// z = B r without the null-space projection (the solver folds it into its reductions)
static int emi_pc_raw(knp_ctx* ctx, const double* r, double* z) {
    KnpEmi& E = ctx->emi;
    const int n = ctx->g.n_nodes_owned, nb = emi_vec_blocks(n);
    if (E.pc_kind == KNP_PC_AMG) {
        const double* in = r;
        if (E.n_bc > 0) {
            hipLaunchKernelGGL(k_emi_mask<0>, dim3(nb), dim3(NT), 0, ctx->stream, n, E.d_mask, r, E.d_t);
            in = E.d_t;
        }
        amg_vcycle(ctx, ctx->hier[0], 0, in, z);
        if (E.n_bc > 0) hipLaunchKernelGGL(k_emi_mask<1>, dim3(nb), dim3(NT), 0, ctx->stream, n, E.d_mask, r, z);
    } else {
        hipLaunchKernelGGL(k_emi_scale, dim3(nb), dim3(NT), 0, ctx->stream, n, E.pc_kind == KNP_PC_VBJACOBI ? E.d_dinv : (const double*)nullptr, r, z);
    }
    HIPCHK(hipGetLastError());
    return KNP_OK;
}

// Device table of the membrane programs for k_emi_facets, rebuilt only after knp_set_program (progs_dirty).  What sync_program_table
// does, without its hiprtc build of the KNP-EMI facet kernel: the EMI facet kernel runs the interpreter only, and a context that
// assembles EMI right-hand sides would pay that compile for nothing.  A native kernel of earlier programs is dropped, so a KNP-EMI
// right-hand side on the same context would run the interpreter too (same values).  Also notes, once per table, the highest aux
// field any program reads (aux_need), so the per-step path does not walk the instruction lists.
static int emi_sync_programs(knp_ctx* ctx) {
    KnpEmi& E = ctx->emi;
    if (!ctx->progs_dirty && E.aux_need >= 0) return KNP_OK;
    if ((int)ctx->progs.size() <= ctx->max_prog) { ctx->err = "a membrane facet refers to a program that was not set (knp_set_program)"; return KNP_E_STATE; }
    const size_t np = std::max<size_t>(ctx->progs.size(), 1);
    std::vector<int32_t*> codes(np, nullptr);
    std::vector<double*> consts(np, nullptr);
    std::vector<int32_t> lens(np, 0), ncs(np, 0);
    ctx->prog_regs = ctx->prog_len_cap = ctx->prog_consts_cap = 0;
    ctx->prog_funcs = false;
    int need = 0;
    for (size_t i = 0; i < ctx->progs.size(); ++i) {
        const KnpProgram& pr = ctx->progs[i];
        if ((int)i <= ctx->max_prog && !pr.d_code) { ctx->err = "membrane program " + std::to_string(i) + " not set"; return KNP_E_STATE; }
        codes[i] = pr.d_code; consts[i] = pr.d_consts; lens[i] = pr.n_instr; ncs[i] = pr.n_consts;
        ctx->prog_regs = std::max(ctx->prog_regs, pr.n_regs);
        ctx->prog_len_cap = std::max(ctx->prog_len_cap, pr.n_instr);
        ctx->prog_consts_cap = std::max(ctx->prog_consts_cap, pr.n_consts);
        ctx->prog_funcs = ctx->prog_funcs || pr.funcs;
        for (int k = 0; k < pr.n_instr; ++k)
            if (pr.h_code[4 * k] == KNP_OP_AUX) need = std::max(need, pr.h_code[4 * k + 2] + 1);
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    dev_free(ctx->d_prog_code); dev_free(ctx->d_prog_consts); dev_free(ctx->d_prog_len); dev_free(ctx->d_prog_nconsts);
    KCHK(dev_upload(ctx, &ctx->d_prog_code, codes));
    KCHK(dev_upload(ctx, &ctx->d_prog_consts, consts));
    KCHK(dev_upload(ctx, &ctx->d_prog_len, lens));
    KCHK(dev_upload(ctx, &ctx->d_prog_nconsts, ncs));
    knp_jit_release(ctx);
    ctx->jit_msg = "not built: the context assembles EMI right-hand sides (interpreter)";
    ctx->progs_dirty = false;
    E.aux_need = need;
    return KNP_OK;
}

extern "C" {

int knp_emi_setup(knp_ctx* ctx, double dt, double C_M, double sigma_i, double sigma_e) {
    CHECK_CTX(ctx);
    const KnpHostGraph& g = ctx->g;
    if (g.n_nodes != g.n_nodes_owned) { ctx->err = "the EMI model runs on one GPU only (the context has ghost nodes)"; return KNP_E_STATE; }
    if (!(dt > 0) || !(C_M > 0) || !(sigma_i > 0) || !(sigma_e > 0)) { ctx->err = "knp_emi_setup: dt, C_M, sigma_i, sigma_e must be positive"; return KNP_E_ARG; }
    KnpEmi& E = ctx->emi;
    const size_t n = (size_t)std::max(g.n_nodes_owned, 1);
    if (!E.d_st) {            // d_st is allocated last: anything short of it is a half-made set from a failed call and is dropped
        knp_emi_free(ctx);
        HIPCHK(hipMalloc((void**)&E.d_val, std::max<size_t>((size_t)ctx->n_pairs, 1) * sizeof(double)));
        HIPCHK(hipMalloc((void**)&E.d_xval, std::max<size_t>((size_t)ctx->n_gp, 1) * sizeof(double)));
        HIPCHK(hipMalloc((void**)&E.d_dinv, n * sizeof(double)));
        HIPCHK(hipMalloc((void**)&E.d_mask, n));
        HIPCHK(hipMemsetAsync(E.d_mask, 0, n, ctx->stream));
        double** w[5] = {&E.d_r, &E.d_z, &E.d_p, &E.d_q, &E.d_t};
        for (int k = 0; k < 5; ++k) {
            HIPCHK(hipMalloc((void**)w[k], n * sizeof(double)));
            HIPCHK(hipMemsetAsync(*w[k], 0, n * sizeof(double), ctx->stream));
        }
        HIPCHK(hipMalloc((void**)&E.d_fvec, std::max<size_t>((size_t)g.n_g * g.dim, 1) * sizeof(double)));
        HIPCHK(hipMalloc((void**)&E.d_st, 4 * sizeof(double)));
    }
    E.dt = dt; E.C_M = C_M; E.sigma_i = sigma_i; E.sigma_e = sigma_e;
    if (ctx->n_pairs > 0)
        hipLaunchKernelGGL(k_emi_pairs, dim3(nblocks(ctx->n_pairs)), dim3(NT), 0, ctx->stream, ctx->n_pairs, ctx->d_pair_row, ctx->d_node_side,
                           ctx->d_pair_K, dt * sigma_i, dt * sigma_e, E.d_val);
    if (ctx->n_gp > 0)
        hipLaunchKernelGGL(k_emi_gamma, dim3(nblocks(ctx->n_gp)), dim3(NT), 0, ctx->stream, ctx->n_gp, g.dim, C_M, ctx->d_grow, ctx->d_gv_node_i,
                           ctx->d_gv_node_e, ctx->d_gq_i, ctx->d_gq_e, ctx->d_gcptr, ctx->d_gc_facet, ctx->d_gc_lab, ctx->d_fmeas, ctx->d_pair_ptr,
                           E.d_val, E.d_xval);
    KCHK(emi_write_dinv(ctx));
    E.ready = true;
    return KNP_OK;
}

int knp_emi_get_csr(knp_ctx* ctx, int32_t* rp, int32_t* ci, double* vals) {
    CHECK_CTX(ctx);
    KCHK(emi_check(ctx));
    if (!rp || !ci || !vals) { ctx->err = "knp_emi_get_csr: null argument"; return KNP_E_ARG; }
    const KnpHostGraph& g = ctx->g;
    const KnpEmi& E = ctx->emi;
    std::vector<double> val((size_t)ctx->n_pairs), xval((size_t)ctx->n_gp);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (!val.empty()) HIPCHK(hipMemcpy(val.data(), E.d_val, val.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (!xval.empty()) HIPCHK(hipMemcpy(xval.data(), E.d_xval, xval.size() * sizeof(double), hipMemcpyDeviceToHost));
    int64_t k = 0;
    rp[0] = 0;
    for (int n = 0; n < g.n_nodes_owned; ++n) {
        for (int p = g.pair_ptr[n]; p < g.pair_ptr[n + 1]; ++p) { ci[k] = g.pair_col[p]; vals[k++] = val[p]; }
        const int A = g.node_gv[n];
        if (A >= 0) {
            const std::vector<int32_t>& gx = g.node_side[n] ? g.gx_e : g.gx_i;
            for (int s = g.gptr[A]; s < g.gptr[A + 1]; ++s) { ci[k] = gx[s]; vals[k++] = xval[s]; }
        }
        rp[n + 1] = (int32_t)k;
    }
    return KNP_OK;
}

int knp_emi_set_dirichlet(knp_ctx* ctx, int32_t n, const int32_t* nodes) {
    CHECK_CTX(ctx);
    KCHK(emi_check(ctx));
    if (n < 0 || (n > 0 && !nodes)) { ctx->err = "knp_emi_set_dirichlet: bad arguments"; return KNP_E_ARG; }
    const int no = ctx->g.n_nodes_owned;
    std::vector<uint8_t> mask((size_t)std::max(no, 1), 0);
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
        if (nodes[i] < 0 || nodes[i] >= no) { ctx->err = "knp_emi_set_dirichlet: node out of range"; return KNP_E_ARG; }
        if (!mask[nodes[i]]) { mask[nodes[i]] = 1; ++cnt; }
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(ctx->emi.d_mask, mask.data(), mask.size(), hipMemcpyHostToDevice));
    ctx->emi.n_bc = cnt;
    return emi_write_dinv(ctx);
}

int knp_emi_spmv(knp_ctx* ctx, const double* x, double* y) {
    CHECK_CTX(ctx);
    KCHK(emi_check(ctx));
    if (!x || !y) { ctx->err = "knp_emi_spmv: null argument"; return KNP_E_ARG; }
    if (ctx->g.n_nodes_owned > 0) emi_launch_spmv<0, false>(ctx, x, nullptr, y);
    HIPCHK(hipGetLastError());
    return KNP_OK;
}

int knp_emi_assemble_rhs(knp_ctx* ctx, const knp_fields* fields, const double* f_i, const double* f_e, const double* gvals,
                         double rhs_scale, double* b) {
    CHECK_CTX(ctx);
    KCHK(emi_check(ctx));
    if (!fields || !b) { ctx->err = "knp_emi_assemble_rhs: null argument"; return KNP_E_ARG; }
    const KnpHostGraph& g = ctx->g;
    KnpEmi& E = ctx->emi;
    if (g.n_g > 0 && !fields->phi_m) { ctx->err = "knp_emi_assemble_rhs: null phi_m field"; return KNP_E_ARG; }
    EmiAux aux;
    int n_aux = 0;
    for (int k = 0; k < KNP_MAX_AUX; ++k) {
        aux.a[k] = fields->aux[k];
        if (fields->aux[k]) n_aux = k + 1;
    }
    for (int k = 0; k < n_aux; ++k)
        if (!fields->aux[k]) { ctx->err = "aux fields must be contiguous from index 0"; return KNP_E_ARG; }
    const int n = g.n_nodes_owned;
    if (g.n_g > 0) {
        KCHK(emi_sync_programs(ctx));
        if (E.aux_need > n_aux) { ctx->err = "a membrane program reads aux field " + std::to_string(E.aux_need - 1) + ", which was not given"; return KNP_E_ARG; }
        const size_t lds = (size_t)std::max(ctx->prog_regs, 1) * EMI_BT * sizeof(double);
        if (lds > 64 * 1024) { ctx->err = "membrane programs need more LDS than the EMI facet kernel has"; return KNP_E_STATE; }
        const int n_progs = ctx->max_prog + 1;
        with_either<2, 3>(g.dim == 2, [&](auto D) {
            with_flag(ctx->prog_funcs, [&](auto M) {
                hipLaunchKernelGGL((k_emi_facets<D(), M()>), dim3(nblocks(g.n_g, EMI_BT)), dim3(EMI_BT), lds, ctx->stream, g.n_g, g.n_q, E.C_M, E.dt,
                                   ctx->d_fv, ctx->d_fmeas, ctx->d_qp, ctx->d_qw, fields->phi_m, aux, n_aux, ctx->d_coords, ctx->d_gamma_prog, n_progs,
                                   (const int32_t* const*)ctx->d_prog_code, (const int32_t*)ctx->d_prog_len,
                                   (const double* const*)ctx->d_prog_consts, E.d_fvec);
            });
        });
    }
    if (n > 0) {
        constexpr int G = 8;
        hipLaunchKernelGGL(k_emi_rhs<G>, dim3(nblocks((int64_t)n * G)), dim3(NT), 0, ctx->stream, n, g.n_g, E.dt, rhs_scale, ctx->d_node_vertex,
                           ctx->d_node_side, ctx->d_pair_ptr, ctx->d_pair_col, ctx->d_pair_M, E.d_val, f_i, f_e, ctx->d_node_gv, ctx->d_gptr,
                           ctx->d_gx_i, ctx->d_gx_e, E.d_xval, ctx->d_gdiag, ctx->d_gcptr, ctx->d_gc_facet, ctx->d_gc_lab, E.d_fvec,
                           E.n_bc > 0 ? E.d_mask : (const uint8_t*)nullptr, gvals, b);
        if (ctx->ns_on && E.n_bc == 0) {   // nullspace.remove(b)
            const int nb = emi_vec_blocks(n);
            hipLaunchKernelGGL(k_emi_sum, dim3(nb), dim3(NT), 0, ctx->stream, n, b, ctx->d_partial + EMI_ROW0);
            hipLaunchKernelGGL(k_emi_sub_mean, dim3(nb), dim3(NT), 0, ctx->stream, n, nb, ctx->d_partial + EMI_ROW0, b);
        }
    }
    HIPCHK(hipGetLastError());
    return KNP_OK;
}

int knp_emi_pc_setup(knp_ctx* ctx, int32_t kind) {
    CHECK_CTX(ctx);
    KCHK(emi_check(ctx));
    if (kind != KNP_PC_NONE && kind != KNP_PC_VBJACOBI && kind != KNP_PC_AMG) { ctx->err = "knp_emi_pc_setup: kind must be none, Jacobi or AMG"; return KNP_E_ARG; }
    if (kind == KNP_PC_AMG) {
        KnpAmgHier& H = ctx->hier[0];
        if (H.levels < 1 || H.lv[0].n != ctx->g.n_nodes_owned || H.lv[0].A_nnz == 0) { ctx->err = "EMI AMG hierarchy not supplied (level 0 = the EMI matrix)"; return KNP_E_STATE; }
        if (H.native0 != 0) { ctx->err = "the EMI hierarchy runs on its uploaded level 0 (knp_amg_use_native_level0 must be off)"; return KNP_E_STATE; }
        for (int l = 0; l < H.levels; ++l) {
            const KnpAmgLevel& L = H.lv[l];
            if (L.n <= 0 || L.dist || L.repl_n > 0) { ctx->err = "EMI AMG hierarchy: level missing or distributed"; return KNP_E_STATE; }
            if (l + 1 < H.levels && L.n_coarse != H.lv[l + 1].n) { ctx->err = "AMG level sizes inconsistent"; return KNP_E_STATE; }
        }
        if (H.nc > 0 && H.nc != H.lv[H.levels - 1].n) { ctx->err = "AMG coarse inverse size mismatch"; return KNP_E_STATE; }
        if (H.pre != H.post) { ctx->err = "EMI AMG hierarchy: pre and post sweeps must be equal (symmetric cycle for CG)"; return KNP_E_ARG; }
        // the generic level-by-level cycle only
        H.fused = H.l0_fused = H.blocked = H.cfused = 0;
        for (int l = 0; l < H.levels; ++l) H.lv[l].lfused = 0;
    }
    ctx->emi.pc_kind = kind;
    return KNP_OK;
}

int knp_emi_pc_apply(knp_ctx* ctx, const double* r, double* z) {
    CHECK_CTX(ctx);
    KCHK(emi_check(ctx));
    if (!r || !z) { ctx->err = "knp_emi_pc_apply: null argument"; return KNP_E_ARG; }
    const int n = ctx->g.n_nodes_owned;
    if (n == 0) return KNP_OK;
    KCHK(emi_pc_raw(ctx, r, z));
    if (ctx->ns_on && ctx->emi.n_bc == 0) {
        const int nb = emi_vec_blocks(n);
        hipLaunchKernelGGL(k_emi_sum, dim3(nb), dim3(NT), 0, ctx->stream, n, z, ctx->d_partial + EMI_ROW0);
        hipLaunchKernelGGL(k_emi_sub_mean, dim3(nb), dim3(NT), 0, ctx->stream, n, nb, ctx->d_partial + EMI_ROW0, z);
    }
    HIPCHK(hipGetLastError());
    return KNP_OK;
}

int knp_emi_cg_solve(knp_ctx* ctx, const double* b, double* x, double rtol, double atol, int32_t max_it, int32_t norm_type,
                     int32_t* its, double* rnorm, int32_t* reason) {
    CHECK_CTX(ctx);
    KCHK(emi_check(ctx));
    if (!b || !x || !its || !rnorm || !reason) { ctx->err = "knp_emi_cg_solve: null argument"; return KNP_E_ARG; }
    if (norm_type < 0 || norm_type > 2 || max_it < 0 || !(rtol >= 0) || !(atol >= 0)) { ctx->err = "knp_emi_cg_solve: bad arguments"; return KNP_E_ARG; }
    side_discard(ctx);     // the reduction scratch and slots are shared with the GMRES drivers
    KnpEmi& E = ctx->emi;
    const int n = ctx->g.n_nodes_owned;
    *its = 0; *rnorm = 0.0; *reason = KNP_CONVERGED_ATOL;
    if (n == 0) return KNP_OK;
    const int nb = emi_vec_blocks(n), nbq = emi_spmv_blocks(ctx);
    const int ns = (ctx->ns_on && E.n_bc == 0) ? 1 : 0;
    double* rows = ctx->d_partial + EMI_ROW0;
    double* mirror = ctx->mirror();
    volatile int64_t* seq = mirror ? ctx->h_seq_dev : nullptr;
    hipStream_t st = ctx->stream;
    const bool ext_pc = E.pc_kind == KNP_PC_AMG;
    HIPCHK(hipMemsetAsync(E.d_st, 0, 4 * sizeof(double), st));
    // the reference of the stopping test: the chosen norm of b (KSPConvergedDefault with a non-zero initial guess)
    if (norm_type == 1) {
        hipLaunchKernelGGL(k_emi_dots, dim3(nb), dim3(NT), 0, st, n, b, b, rows);
    } else {
        KCHK(emi_pc_raw(ctx, b, E.d_z));
        hipLaunchKernelGGL(k_emi_dots, dim3(nb), dim3(NT), 0, st, n, b, E.d_z, rows);
    }
    hipLaunchKernelGGL(k_emi_ref, dim3(1), dim3(NT), 0, st, n, nb, rows, ns, norm_type, ctx->d_red, mirror, seq, ++ctx->seq_counter);
    // Dirichlet nodes take their value at once (identity rows: x = b there), so their residual is zero from the start and stays zero
    if (E.n_bc > 0) hipLaunchKernelGGL(k_emi_mask<1>, dim3(nb), dim3(NT), 0, st, n, E.d_mask, b, x);
    // r = b - A x, z = B r, p = z
    emi_launch_spmv<1, false>(ctx, x, b, E.d_r);
    if (ns) {
        // A x has no component along the constant, but its rounding errors (of the size eps |A| |x|, far above rtol |b| when x is
        // nearly constant per side) do, and no search direction could ever remove it from r: take it out once
        hipLaunchKernelGGL(k_emi_sum, dim3(nb), dim3(NT), 0, st, n, E.d_r, rows);
        hipLaunchKernelGGL(k_emi_sub_mean, dim3(nb), dim3(NT), 0, st, n, nb, rows, E.d_r);
    }
    KCHK(emi_pc_raw(ctx, E.d_r, E.d_z));
    hipLaunchKernelGGL(k_emi_dots, dim3(nb), dim3(NT), 0, st, n, E.d_r, E.d_z, rows);
    int cur = 0;
    hipLaunchKernelGGL(k_emi_p, dim3(nb), dim3(NT), 0, st, n, nb, rows, ns, norm_type, 1, E.d_st, cur, E.d_z, E.d_p, ctx->d_red, mirror, seq, ++ctx->seq_counter);
    cur ^= 1;
    emi_launch_spmv<0, true>(ctx, E.d_p, nullptr, E.d_q);       // enqueued before the host waits: the read-back hides behind it
    HIPCHK(hipGetLastError());
    KCHK(read_slots(ctx, EMI_SLOT, 4, ctx->seq_counter));
    const double bref = std::sqrt(std::max(ctx->h_red[EMI_SLOT + 3], 0.0));
    if (!std::isfinite(ctx->h_red[EMI_SLOT + 3])) { *rnorm = ctx->h_red[EMI_SLOT + 3]; *reason = KNP_DIVERGED_NANORINF; return KNP_OK; }
    ctx->last_bnorm = bref;
    const double ttol = std::max(rtol * bref, atol);
    int it = 0;
    for (;;) {
        const double dp2 = ctx->h_red[EMI_SLOT], flag = ctx->h_red[EMI_SLOT + 2];
        const double res = std::sqrt(std::max(dp2, 0.0));
        *rnorm = res;
        if (flag != 0.0 || !std::isfinite(dp2) || !std::isfinite(ctx->h_red[EMI_SLOT + 1])) { *reason = KNP_DIVERGED_NANORINF; break; }
        if (res <= ttol) { *reason = (res <= atol) ? KNP_CONVERGED_ATOL : KNP_CONVERGED_RTOL; break; }
        if (it >= max_it) { *reason = KNP_DIVERGED_ITS; break; }
        if (res > 1e5 * bref) { *reason = KNP_DIVERGED_DTOL; break; }
        // q = A p and the partial sums of p . q are already enqueued
        if (ext_pc) {
            hipLaunchKernelGGL(k_emi_xr<2>, dim3(nb), dim3(NT), 0, st, n, nbq, ctx->d_partial, E.d_st, cur, E.d_p, E.d_q, E.d_dinv, x, E.d_r, E.d_z, rows);
            KCHK(emi_pc_raw(ctx, E.d_r, E.d_z));
            hipLaunchKernelGGL(k_emi_dots, dim3(nb), dim3(NT), 0, st, n, E.d_r, E.d_z, rows);
        } else if (E.pc_kind == KNP_PC_VBJACOBI) {
            hipLaunchKernelGGL(k_emi_xr<1>, dim3(nb), dim3(NT), 0, st, n, nbq, ctx->d_partial, E.d_st, cur, E.d_p, E.d_q, E.d_dinv, x, E.d_r, E.d_z, rows);
        } else {
            hipLaunchKernelGGL(k_emi_xr<0>, dim3(nb), dim3(NT), 0, st, n, nbq, ctx->d_partial, E.d_st, cur, E.d_p, E.d_q, E.d_dinv, x, E.d_r, E.d_z, rows);
        }
        hipLaunchKernelGGL(k_emi_p, dim3(nb), dim3(NT), 0, st, n, nb, rows, ns, norm_type, 0, E.d_st, cur, E.d_z, E.d_p, ctx->d_red, mirror, seq, ++ctx->seq_counter);
        cur ^= 1;
        emi_launch_spmv<0, true>(ctx, E.d_p, nullptr, E.d_q);
        HIPCHK(hipGetLastError());
        ++it;
        KCHK(read_slots(ctx, EMI_SLOT, 3, ctx->seq_counter));
    }
    *its = it;
    return KNP_OK;
}

int knp_emi_update(knp_ctx* ctx, const double* x, double* phi_i, double* phi_e, double* phi_m) {
    CHECK_CTX(ctx);
    KCHK(emi_check(ctx));
    if (!x || !phi_i || !phi_e || !phi_m) { ctx->err = "knp_emi_update: null argument"; return KNP_E_ARG; }
    const KnpHostGraph& g = ctx->g;
    if (g.n_v > 0)
        hipLaunchKernelGGL(k_emi_update, dim3(nblocks(g.n_v)), dim3(NT), 0, ctx->stream, g.n_v, ctx->d_node_i, ctx->d_node_e, g.n_nodes_owned, x,
                           phi_i, phi_e, phi_m);
    HIPCHK(hipGetLastError());
    return KNP_OK;
}

}  // extern "C"
