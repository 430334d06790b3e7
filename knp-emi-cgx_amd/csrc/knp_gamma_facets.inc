// Membrane facet quadrature kernel (K2).  This file is compiled twice:
//   * ahead of time, included from knp_kernels.hip: the mechanism currents are evaluated by the bytecode INTERPRETER;
//   * at run time through hiprtc (knp_jit.cpp) with KNP_GAMMA_JIT defined, after the generated straight-line functions
//     knp_prog_<id>() and the dispatcher knp_jit_eval(): the mechanism currents are NATIVE code (what FFCx's JIT gives
//     the reference).  The JIT build only instantiates the VEC (right-hand side) variants.
// Needs before inclusion: KNP_MAX_AUX, DevParams, FieldPtrs, and (interpreter build) the KNP_OP_* opcodes.

__device__ __forceinline__ double powi_d(double x, int e) {
    bool neg = e < 0;
    unsigned u = neg ? (unsigned)(-e) : (unsigned)e;
    double r = 1.0;
    while (u) {
        if (u & 1u) r *= x;
        x *= x;
        u >>= 1;
    }
    return neg ? 1.0 / r : r;
}

#ifndef KNP_GAMMA_JIT
#define KNP_JIT_XMASK 7
// The register file lives in LDS (a private array indexed by the instruction stream would be spilled to scratch
// memory): register r of evaluation s of thread t sits at reg[(r*QV + s)*BT + t] -- one column per thread, conflict-free.
// Each interpreted instruction is executed for QV quadrature points at once: the decode, the branch and the LDS
// latency are paid once per instruction and the QV independent evaluations overlap.  `code` / `consts` point to LDS
// when the whole block runs the same program (the usual case), to global memory otherwise.
// The caller guarantees that every active lane of the wave runs the same program, so the instruction words are
// wave-uniform: readfirstlane moves them to scalar registers (scalar branch, scalar address arithmetic), and the next
// instruction is fetched while the current one executes.
// FUNCS: the instantiation that also knows the function block KNP_OP_SIN / COS / TANH.  A kernel launches it only for a program that
// holds such an opcode (program_uses_funcs): inlined, the three fp64 functions (Payne-Hanek range reduction) cost every kernel around
// the interpreter some 19 registers and eleven of them a wave of occupancy, for programs that never call them.  Behind a call the
// FUNCS kernels keep the registers of their twins, and the kernels without the flag are the ones of before, instruction by instruction.
__device__ __noinline__ double prog_sin(double x) { return sin(x); }
__device__ __noinline__ double prog_cos(double x) { return cos(x); }
__device__ __noinline__ double prog_tanh(double x) { return tanh(x); }

template <int QV, int BT, bool FUNCS = false>
__device__ __forceinline__ void run_program(const int32_t* code, int n_instr, const double* consts,
                                            const double (*ki)[3], const double (*ke)[3], const double* phim,
                                            const double (*aux)[KNP_MAX_AUX], const double (*xq)[3], double (*Iout)[3], double* reg) {
#define RG(i, s) reg[((i) * QV + (s)) * BT]
#define EACH for (int s_ = 0; s_ < QV; ++s_)
#define UN(expr)                                                       \
    _Pragma("unroll") EACH { const double x = RG(a, s_); RG(d, s_) = (expr); } \
    break
#define BIN(expr)                                                                             \
    _Pragma("unroll") EACH { const double x = RG(a, s_), y = RG(b, s_); RG(d, s_) = (expr); } \
    break
    int4 nxt = n_instr > 0 ? *reinterpret_cast<const int4*>(code) : make_int4(0, 0, 0, 0);
    for (int i = 0; i < n_instr; ++i) {
        const int4 ins = nxt;
        if (i + 1 < n_instr) nxt = *reinterpret_cast<const int4*>(code + 4 * (i + 1));
        const int op = __builtin_amdgcn_readfirstlane(ins.x), d = __builtin_amdgcn_readfirstlane(ins.y),
                  a = __builtin_amdgcn_readfirstlane(ins.z), b = __builtin_amdgcn_readfirstlane(ins.w);
        switch (op) {
            case KNP_OP_CONST: { const double c = consts[a];
#pragma unroll
                EACH RG(d, s_) = c; } break;
            case KNP_OP_KI:
#pragma unroll
                EACH RG(d, s_) = ki[s_][a]; break;
            case KNP_OP_KE:
#pragma unroll
                EACH RG(d, s_) = ke[s_][a]; break;
            case KNP_OP_PHIM:
#pragma unroll
                EACH RG(d, s_) = phim[s_]; break;
            case KNP_OP_AUX:
#pragma unroll
                EACH RG(d, s_) = aux[s_][a]; break;
            case KNP_OP_X:
#pragma unroll
                EACH RG(d, s_) = xq[s_][a]; break;
            case KNP_OP_ADD: BIN(x + y);
            case KNP_OP_SUB: BIN(x - y);
            case KNP_OP_MUL: BIN(x * y);
            case KNP_OP_DIV: BIN(x / y);
            case KNP_OP_NEG: UN(-x);
            case KNP_OP_POW: BIN(pow(x, y));
            case KNP_OP_LN: UN(log(x));
            case KNP_OP_EXP: UN(exp(x));
            case KNP_OP_SQRT: UN(sqrt(x));
            case KNP_OP_MAX: BIN(fmax(x, y));
            case KNP_OP_MIN: BIN(fmin(x, y));
            case KNP_OP_ABS: UN(fabs(x));
            case KNP_OP_LT: BIN(x < y ? 1.0 : 0.0);
            case KNP_OP_GT: BIN(x > y ? 1.0 : 0.0);
            case KNP_OP_LE: BIN(x <= y ? 1.0 : 0.0);
            case KNP_OP_GE: BIN(x >= y ? 1.0 : 0.0);
            case KNP_OP_EQ: BIN(x == y ? 1.0 : 0.0);
            case KNP_OP_AND: BIN((x != 0.0 && y != 0.0) ? 1.0 : 0.0);
            case KNP_OP_OR: BIN((x != 0.0 || y != 0.0) ? 1.0 : 0.0);
            case KNP_OP_NOT: UN(x != 0.0 ? 0.0 : 1.0);
            case KNP_OP_SEL:
#pragma unroll
                EACH { if (RG(a, s_) != 0.0) RG(d, s_) = RG(b, s_); } break;
            case KNP_OP_OUT:
#pragma unroll
                EACH Iout[s_][a] += RG(b, s_); break;
            case KNP_OP_MOV: UN(x);
            case KNP_OP_POWI: UN(powi_d(x, b));
            default:
                if constexpr (FUNCS) {
                    if (op == KNP_OP_SIN) { EACH RG(d, s_) = prog_sin(RG(a, s_)); }
                    else if (op == KNP_OP_COS) { EACH RG(d, s_) = prog_cos(RG(a, s_)); }
                    else if (op == KNP_OP_TANH) { EACH RG(d, s_) = prog_tanh(RG(a, s_)); }
                }
                break;
        }
    }
#undef BIN
#undef UN
#undef EACH
#undef RG
}

#endif  // !KNP_GAMMA_JIT

// ------------------------------------------------------------------------------------------
// K2: membrane facet quadrature.  LF lanes per facet; a lane takes the quadrature points q = lane + LF*s, QV of them
//     at a time; partial sums are combined with a fixed shuffle tree (deterministic).
//   fmat[(g*NPK + ab)*6 + k], k = 0..2 intra ions, 3..5 extra ions : M_Gamma[alpha^k C_M/(F z_k)]
//   fvec[(k*DIM + a)*n_g + g],  k = 0..2 intra, 3..5 extra, 6 potential
// ------------------------------------------------------------------------------------------
template <int DIM, bool MAT, bool VEC, int LF, int QV, int BT, bool FUNCS = false>
__device__ __forceinline__ void
gamma_facets_body(int n_g, int n_q, DevParams P, const int32_t* __restrict__ fv, const double* __restrict__ fmeas,
               const double* __restrict__ qp, const double* __restrict__ qw, FieldPtrs f, int n_aux,
               const double* __restrict__ coords, const int32_t* __restrict__ gamma_prog,
               const int32_t* const* __restrict__ prog_code, const int32_t* __restrict__ prog_len,
               const double* const* __restrict__ prog_consts, const int32_t* __restrict__ prog_nconsts, int n_regs,
               int consts_cap, double* __restrict__ fmat, double* __restrict__ fvec) {
    constexpr int NPK = DIM * (DIM + 1) / 2;
#ifndef KNP_GAMMA_JIT
    extern __shared__ double smem[];   // VEC only: [n_regs][QV][BT] register file | [consts_cap] constants | program code
#endif
    const int g_raw = (blockIdx.x * BT + threadIdx.x) / LF;
    const int qlane = threadIdx.x & (LF - 1);
    const bool live = g_raw < n_g;
    const int g = live ? g_raw : n_g - 1;      // idle lanes shadow the last facet so that shuffles stay uniform
    int v[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) v[a] = fv[(size_t)g * DIM + a];
    double ki[3][DIM], ke[3][DIM], pm[DIM];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            ki[j][a] = f.ki[j][v[a]];
            ke[j][a] = f.ke[j][v[a]];
        }
#pragma unroll
    for (int a = 0; a < DIM; ++a) pm[a] = f.phim[v[a]];
    const double meas = fmeas[g];
    double am[MAT ? 6 : 1][MAT ? NPK : 1];
    double av[VEC ? 7 : 1][VEC ? DIM : 1];
    if (MAT) {
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int i = 0; i < NPK; ++i) am[k][i] = 0.0;
    }
    if (VEC) {
#pragma unroll
        for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int a = 0; a < DIM; ++a) av[k][a] = 0.0;
    }
    const int prog = VEC ? gamma_prog[g] : 0;
    // P.dz2i/dz2e/rFz/cmFz/rF: loop invariants prepared on the host.  A division in double precision is ~11 instructions with a
    // quarter-rate reciprocal inside, and the compiler may not turn x / c into x * (1 / c) by itself -- 13 of the 25 divisions per
    // quadrature point were by these constants or by the two conductivity sums
#ifdef KNP_GAMMA_JIT
    double U[KNP_JIT_UNIFORMS];      // sub-expressions of the program that only depend on its constants: once per thread, not per point
    if (VEC) knp_jit_pre(prog, prog_consts[prog], U);
#endif
#ifndef KNP_GAMMA_JIT
    const int32_t* code = nullptr;
    const double* consts = nullptr;
    int n_instr = 0;
    if (VEC) {
        __shared__ int s_p0;
        if (threadIdx.x == 0) s_p0 = prog;
        __syncthreads();
        const int p0 = s_p0;
        n_instr = prog_len[prog];
        if (__syncthreads_and(prog == p0)) {      // one program for the whole block: run it out of LDS
            double* sconst = smem + (size_t)n_regs * QV * BT;
            int32_t* scode = reinterpret_cast<int32_t*>(sconst + consts_cap);
            const int32_t* gc = prog_code[p0];
            const double* gk = prog_consts[p0];
            for (int i = threadIdx.x; i < 4 * n_instr; i += BT) scode[i] = gc[i];
            for (int i = threadIdx.x; i < prog_nconsts[p0]; i += BT) sconst[i] = gk[i];
            __syncthreads();
            code = scode;
            consts = sconst;
        }   // else: code stays null and every wave walks through its distinct programs one at a time (below)
    }
#endif
    for (int q0 = qlane; q0 < n_q; q0 += LF * QV) {
        double lam[QV][DIM], w[QV], kiq[QV][3], keq[QV][3], phq[QV], ali[QV][3], ale[QV][3];
#pragma unroll
        for (int s = 0; s < QV; ++s) {
            const int qq = q0 + s * LF;
            const bool on = qq < n_q;
            const int q = on ? qq : q0;               // surplus slots repeat a valid point with weight zero
#pragma unroll
            for (int a = 0; a < DIM; ++a) lam[s][a] = qp[q * DIM + a];
            w[s] = on ? qw[q] * meas : 0.0;
            phq[s] = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double si = 0.0, se = 0.0;
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                    si += lam[s][a] * ki[j][a];
                    se += lam[s][a] * ke[j][a];
                }
                kiq[s][j] = si;
                keq[s][j] = se;
            }
#pragma unroll
            for (int a = 0; a < DIM; ++a) phq[s] += lam[s][a] * pm[a];
            double deni = 0.0, dene = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                deni += P.dz2i[j] * kiq[s][j];
                dene += P.dz2e[j] * keq[s][j];
            }
            const double rdi = 1.0 / deni, rde = 1.0 / dene;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                ali[s][j] = P.dz2i[j] * kiq[s][j] * rdi;
                ale[s][j] = P.dz2e[j] * keq[s][j] * rde;
            }
            if (MAT) {
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double wi = w[s] * ali[s][j] * P.cmFz[j];
                    const double we = w[s] * ale[s][j] * P.cmFz[j];
                    int idx = 0;
#pragma unroll
                    for (int a = 0; a < DIM; ++a)
#pragma unroll
                        for (int b = a; b < DIM; ++b) {
                            const double ll = lam[s][a] * lam[s][b];
                            am[j][idx] += wi * ll;
                            am[3 + j][idx] += we * ll;
                            ++idx;
                        }
                }
            }
        }
        if (VEC) {
            double auxq[QV][KNP_MAX_AUX], xq[QV][3], Iout[QV][3];
#pragma unroll
            for (int s = 0; s < QV; ++s) {
#ifdef KNP_GAMMA_JIT
                // the generated programs state how many auxiliary fields they read: a compile-time bound keeps auxq in registers (a run-time
                // bound makes it a dynamically indexed array, i.e. scratch memory: 576 bytes per lane with 9 points in flight)
#pragma unroll
                for (int k = 0; k < KNP_JIT_NAUX; ++k) {
#else
                for (int k = 0; k < n_aux; ++k) {
#endif
                    double t = 0.0;
#pragma unroll
                    for (int a = 0; a < DIM; ++a) t += lam[s][a] * f.aux[k][v[a]];
                    auxq[s][k] = t;
                }
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    double t = 0.0;
                    if (d < DIM && ((KNP_JIT_XMASK >> d) & 1)) {   // only the coordinates a program reads
#pragma unroll
                        for (int a = 0; a < DIM; ++a) t += lam[s][a] * coords[(size_t)v[a] * DIM + d];
                    }
                    xq[s][d] = t;
                    Iout[s][d] = 0.0;
                }
            }
#ifdef KNP_GAMMA_JIT
#pragma unroll
            for (int s = 0; s < QV; ++s) knp_jit_eval(prog, prog_consts[prog], U, kiq[s], keq[s], phq[s], auxq[s], xq[s], Iout[s]);
#else
            double* reg = smem + threadIdx.x;
            if (code) {
                run_program<QV, BT, FUNCS>(code, n_instr, consts, kiq, keq, phq, auxq, xq, Iout, reg);
            } else {   // mixed block: serialise over the programs present in this wave (the interpreter needs uniform code)
                bool pending = true;
                while (true) {
                    const unsigned long long m = __ballot(pending);
                    if (!m) break;
                    const int pl = __shfl(prog, __ffsll((long long)m) - 1);
                    if (pending && prog == pl) {
                        run_program<QV, BT, FUNCS>(prog_code[pl], prog_len[pl], prog_consts[pl], kiq, keq, phq, auxq, xq, Iout, reg);
                        pending = false;
                    }
                }
            }
#endif
#pragma unroll
            for (int s = 0; s < QV; ++s) {
                const double Itot = Iout[s][0] + Iout[s][1] + Iout[s][2];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double gi = w[s] * (P.dt * Iout[s][j] - ali[s][j] * P.C_M * phq[s]) * P.rFz[j];
                    const double ge = w[s] * (P.dt * Iout[s][j] - ale[s][j] * P.C_M * phq[s]) * P.rFz[j];
#pragma unroll
                    for (int a = 0; a < DIM; ++a) {
                        av[j][a] += gi * lam[s][a];
                        av[3 + j][a] += ge * lam[s][a];
                    }
                }
                const double gp = w[s] * (P.dt * Itot - P.C_M * phq[s]) * P.rF;
#pragma unroll
                for (int a = 0; a < DIM; ++a) av[6][a] += gp * lam[s][a];
            }
        }
    }
    if (MAT) {
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int i = 0; i < NPK; ++i) {
                double t = am[k][i];
#pragma unroll
                for (int o = LF >> 1; o > 0; o >>= 1) t += __shfl_xor(t, o, LF);
                // facet-major records {M_i^1..3, M_e^1..3} per local vertex pair: k_gamma_pairs gathers the 48 bytes of a contribution from
                // one place (six planes indexed by facet cost it six cache lines); every lane holds the sum, the lanes share the stores
                if (live && qlane == ((i * 6 + k) & (LF - 1))) fmat[((size_t)g * NPK + i) * 6 + k] = t;
            }
    }
    if (VEC) {
#pragma unroll
        for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                double t = av[k][a];
#pragma unroll
                for (int o = LF >> 1; o > 0; o >>= 1) t += __shfl_xor(t, o, LF);
                if (live && qlane == 0) fvec[((size_t)k * DIM + a) * n_g + g] = t;
            }
    }
}

#define KNP_GAMMA_ARGS                                                                                                        \
    int n_g, int n_q, DevParams P, const int32_t *__restrict__ fv, const double *__restrict__ fmeas,                           \
        const double *__restrict__ qp, const double *__restrict__ qw, FieldPtrs f, int n_aux, const double *__restrict__ coords, \
        const int32_t *__restrict__ gamma_prog, const int32_t *const *__restrict__ prog_code, const int32_t *__restrict__ prog_len, \
        const double *const *__restrict__ prog_consts, const int32_t *__restrict__ prog_nconsts, int n_regs, int consts_cap,   \
        double *__restrict__ fmat, double *__restrict__ fvec
#define KNP_GAMMA_PASS                                                                                                         \
    n_g, n_q, P, fv, fmeas, qp, qw, f, n_aux, coords, gamma_prog, prog_code, prog_len, prog_consts, prog_nconsts, n_regs, consts_cap, fmat, fvec

#ifdef KNP_GAMMA_JIT
// the two right-hand-side variants the library launches (same tuning as the interpreter build)
extern "C" __global__ void __launch_bounds__(64, 2) knp_gamma_vec_2d(KNP_GAMMA_ARGS) { gamma_facets_body<2, false, true, 8, 1, 64>(KNP_GAMMA_PASS); }
extern "C" __global__ void __launch_bounds__(64, 2) knp_gamma_vec_3d(KNP_GAMMA_ARGS) { gamma_facets_body<3, false, true, 16, 3, 64>(KNP_GAMMA_PASS); }
// 4 lanes x 9 points = the 36 points of the degree-10 rule exactly, no surplus slots (16 lanes x 3 points evaluate 48 slots: a
// quarter of the transcendental work is thrown away), fewer shuffles per facet; the default in 3D (gamma_many in knp_kernels.hip)
extern "C" __global__ void __launch_bounds__(64, 1) knp_gamma_vec_3d_many(KNP_GAMMA_ARGS) { gamma_facets_body<3, false, true, 4, 9, 64>(KNP_GAMMA_PASS); }
// The same 4 lanes per facet with ONE point in flight per lane (nine trips): the default in 3D.  Measured on MI355X, 1.5 M facets, the
// HH + pump + cotransporter program: 9 points in flight 3.06 ms (450 registers incl. 194 accumulation registers used as spill space, one
// wave per SIMD, ~1000 instructions per point), 3 points 2.31 ms, 1 point 1.73 ms (236 registers, two waves per SIMD, 635 instructions
// per point); forcing three or four waves per SIMD spills to scratch memory: 3.06 / 3.70 ms.  KNP_GAMMA_QV=9 keeps the nine-point kernel.
extern "C" __global__ void __launch_bounds__(64, 2) knp_gamma_vec_3d_q1(KNP_GAMMA_ARGS) { gamma_facets_body<3, false, true, 4, 1, 64>(KNP_GAMMA_PASS); }
#else
template <int DIM, bool MAT, bool VEC, int LF, int QV, int BT, int OCC, bool FUNCS = false>
__global__ void __launch_bounds__(BT, OCC) k_gamma_facets(KNP_GAMMA_ARGS) {
    gamma_facets_body<DIM, MAT, VEC, LF, QV, BT, FUNCS>(KNP_GAMMA_PASS);
}
#endif

