/*
 * knpemi_hip.h -- C ABI of libknpemi_hip.so: the MI355X-native (gfx950) replacement for the
 * third-party native code that the reference (hherlyng/knp-emi-cgx) calls on its per-timestep
 * KNP-EMI assemble-and-solve path.  Plain pointers and sizes only; no torch / DOLFINx / PETSc types.
 *
 * What each entry point replaces (file:line relative to the reference repository):
 *
 *   knp_create / knp_get_layout / knp_get_csr_pattern
 *        multiphenicsx.fem.DofMapRestriction + create_matrix_block / create_vector_block
 *        (src/CGx/KNPEMI/KNPEMIx_problem.py:75-94, src/CGx/KNPEMI/KNPEMIx_solver.py:157-161)
 *   knp_set_params                   constants of the forms (KNPEMIx_problem.py:459-462, 909-981)
 *   knp_set_program / knp_set_program_constants
 *        the FFCx-JIT-compiled membrane integrands built from IonicModel._eval
 *        (KNPEMIx_problem.py:504-555, 609-610, 641-642; KNPEMIx_ionic_model.py:_eval methods)
 *   knp_assemble_matrix              assemble_matrix_block(A, a)      (KNPEMIx_solver.py:110-115)
 *   knp_assemble_matrix_async        the same, next to the right-hand side chain (own stream)
 *   knp_assemble_rhs                 assemble_vector_block(b, L, a)   (KNPEMIx_solver.py:116)
 *   knp_assemble_precond             assemble_matrix_block(P)         (KNPEMIx_solver.py:118-127,
 *                                    form KNPEMIx_problem.py:657-744)
 *   knp_set_nullspace / knp_project_nullspace
 *        MatNullSpace create/test/remove                              (KNPEMIx_solver.py:297-335)
 *   knp_set_deflation                (multi-GPU only) restores what BoomerAMG's global coarse levels give the reference
 *   knp_pc_setup / knp_amg_*         PC setup: ksp.setUp() with pc_type hypre (KNPEMIx_solver.py:211-214,
 *                                    269-273, 386-389) -> vertex-block Jacobi / aggregation AMG
 *   knp_gmres_solve                  ksp.solve(b, x): GMRES(30), left PC, CGS, preconditioned norm
 *                                    (KNPEMIx_solver.py:435; options :276-280)
 *   knp_pack / knp_unpack            BlockVecSubVectorWrapper copies + phi_m = phi_i - phi_e
 *                                    (KNPEMIx_solver.py:177-209, 452-468)
 *   knp_hh_update                    HodgkinHuxley.update_gating_variables
 *                                    (KNPEMIx_ionic_model.py:605-671)
 *   knp_state_reset / knp_state_set_program / knp_state_set_constants / knp_state_update
 *        the same update for the states of any mechanism: the gating ODEs of KNPEMIx_ionic_model.py:605-671 with the rate
 *        functions given as bytecode programs instead of the six hard-coded ones
 *   knp_l2_norms                     assemble_scalar(inner(phi,phi)*dx(tag)) (src/CGx/KNPEMI/main.py:70-84)
 *   knp_diag_set_cell_tags / knp_diag_volume_integrals
 *        assemble_scalar(k*dx(tag)) per ion and cell tag of print_conservation (KNPEMIx_problem.py:821-840)
 *   knp_diag_set_facet_tags / knp_diag_set_program / knp_diag_set_program_constants / knp_diag_membrane_integral
 *        assemble_scalar(stim_ufl_expr*dS(stimulus_tags)) of the stimulus trace (KNPEMIx_solver.py:580-582, 605-607)
 *   knp_diag_set_flux_facets / knp_diag_membrane_fluxes
 *        assemble_scalar of the six forms of create_flux_forms (utils/calc_fluxes.py:70-90), per membrane tag
 *   knp_diag_set_phim_facets / knp_diag_membrane_potential
 *        integral, minimum and maximum of phi_m per membrane tag: what utils/plot_membrane_potentials.py:48-128 reads per cell from
 *        the reference's per-step checkpoints
 *   knp_activation_arm / knp_activation_step / knp_activation_velocity / knp_diag_set_activation_facets / knp_diag_activation
 *        activation and repolarisation time, peak and upstroke per membrane vertex, conduction velocity per membrane facet: what
 *        utils/plot_membrane_potentials*.py would need the reference's checkpoints of every field at every step for
 *   knp_sample_plan_create / knp_sample
 *        scifem.evaluate_function at many points: the slices the reference cuts out of its checkpoints with pyvista
 *        (utils/plot_slices.py, plot_slice_membrane.py, plot_slices_geometries.py)
 *   knp_functional_create / knp_functional_eval
 *        dfx.fem.assemble_scalar(dfx.fem.form(<UFL expression> * dx(tag))) for any expression of the nodal fields, their gradients
 *        and the coordinates: the norms of main.py:70-84 and tests/KNPEMI/electric_potential_norms_*.py, print_conservation, ...
 *   knp_membrane_functional_create / knp_membrane_functional_eval
 *        dfx.fem.assemble_scalar(dfx.fem.form(<UFL expression> * dS(tag))) with '+' / '-' restrictions, FacetNormal and normal
 *        derivatives: the stimulus current of KNPEMIx_solver.py:580-585, the flux forms of utils/calc_fluxes.py:88
 *   knp_functional_eval_items / knp_membrane_functional_eval_items / knp_project_apply
 *        a UFL expression projected or interpolated into a piecewise-constant or P1 space: its value on every cell or facet, and
 *        the measure-weighted average of those onto the vertices (current density, ion fluxes, channel currents as fields)
 *   knp_functional_eval_load / knp_membrane_functional_eval_load / knp_scatter_apply / knp_rhs_add_load
 *        dfx.fem.assemble_vector(dfx.fem.form(<UFL expression> * v * dx(tag) | dS(tag))) with a P1 test function v, and its
 *        addition to the step's right-hand side: L += dt * inner(ion['f_i'], vki) * dxi (KNPEMIx_problem.py:613-614)
 *   knp_emi_*                        the EMI model (src/CGx/EMI): assemble_matrix_block / assemble_vector_block of the forms
 *                                    EMIx_problem.py:152-157, 215-217 and ksp.solve with KSPCG (EMIx_solver.py)
 *   knp_set_comm                     the MPI calls hidden in PETSc/DOLFINx (ghost updates
 *                                    KNPEMIx_solver.py:439,459,468; Allreduce inside KSPSolve)
 *
 * Conventions
 *   - every function returns 0 on success, a negative KNP_E_* otherwise; knp_last_error() gives text.
 *     Nothing throws or exits across the ABI.  Non-convergence is a *reason code*, not an error.
 *   - a ctx is bound to the HIP device current at knp_create and to one stream (knp_set_stream);
 *     it is not thread-safe; one ctx per GPU.
 *   - the one-off host-side passes (graph build in knp_create, hierarchy hand-over in knp_amg_set_level*) are OpenMP loops sized to
 *     the CPU share of the process: cgroup quota or affinity mask, divided by LOCAL_WORLD_SIZE, at most 32; KNP_HOST_THREADS=<n>
 *     overrides.  Nothing on the per-step path uses host threads.
 *   - "host" pointers are read/written by the CPU during the call; "device" pointers are HBM
 *     addresses owned by the caller (e.g. torch tensors) unless stated otherwise.
 *   - unknown numbering: node = (vertex, side); DoF = 4*node + f, f = 0..2 ions, f = 3 potential.
 *     Nodes follow vertex order; a membrane vertex contributes its intra node then its extra node.
 *     Owned vertices come first (multi-GPU): rows exist for owned nodes only, columns may refer
 *     to ghost nodes; vectors have n_dof_local entries (owned part first).
 */
#ifndef KNPEMI_HIP_H
#define KNPEMI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KNP_MAX_IONS 3
#define KNP_MAX_AUX 8
#define KNP_DIAG_MAX_CONSTS 64   /* constants of a diagnostic program (knp_diag_set_program) */
#define KNP_MAX_PROG_REGS 48
#define KNP_STATE_MAX_INSTR 768  /* instructions of all state programs together (knp_state_set_program) */
#define KNP_STATE_MAX_CONSTS 128 /* constants of all state programs together */
#define KNP_MAX_AMG_LEVELS 16
#define KNP_FUNCTIONAL_MAX_Q 125 /* quadrature points per cell of a volume functional (knp_functional_create) and per facet of a membrane functional */

#define KNP_OK 0
#define KNP_E_ARG (-1)
#define KNP_E_HIP (-2)
#define KNP_E_STATE (-3)
#define KNP_E_ALLOC (-4)
#define KNP_E_MESH (-5)

/* converged reasons (mirroring PETSc's KSPConvergedReason values) */
#define KNP_CONVERGED_RTOL 2
#define KNP_CONVERGED_ATOL 3
#define KNP_DIVERGED_ITS (-3)
#define KNP_DIVERGED_DTOL (-4)
#define KNP_DIVERGED_NANORINF (-9)

/* preconditioner kinds */
#define KNP_PC_NONE 0
#define KNP_PC_VBJACOBI 1 /* per-vertex 4x4 / 8x8 blocks of A, refreshed with A */
#define KNP_PC_AMG 2      /* multilevel V-cycle on P, hierarchy 0 = all fields (the reference's block-Jacobi form) */
#define KNP_PC_AMG_BT 3   /* block lower-triangular: hierarchy 0 = ion fields, then the potential (hierarchy 1) on
                             r_phi - A_{phi,k} z_k with a Cahouet-Chabard Schur term psi/(sum z^2 k)/M_lumped added */
#define KNP_PC_AMG_LT 4   /* the reference's P with use_block_jacobi=False (KNPEMIx_problem.py:720-722): P keeps the (phi,k) blocks
                             dt z_j D_j K (= those of A); applied as the block forward substitution z_k = V_k r_k,
                             z_phi = V_phi (r_phi - P_{phi,k} z_k) with the same two hierarchies, no Schur term */

/* membrane-program opcodes: instruction = {op, dst, a, b}, registers are doubles */
enum {
    KNP_OP_CONST = 0, /* dst = consts[a] */
    KNP_OP_KI = 1,    /* dst = k_i^a at the quadrature point */
    KNP_OP_KE = 2,    /* dst = k_e^a */
    KNP_OP_PHIM = 3,  /* dst = phi_m */
    KNP_OP_AUX = 4,   /* dst = aux field a (gating variables, ...) */
    KNP_OP_X = 5,     /* dst = coordinate a */
    KNP_OP_ADD = 6, KNP_OP_SUB = 7, KNP_OP_MUL = 8, KNP_OP_DIV = 9, KNP_OP_NEG = 10,
    KNP_OP_POW = 11, KNP_OP_LN = 12, KNP_OP_EXP = 13, KNP_OP_SQRT = 14,
    KNP_OP_MAX = 15, KNP_OP_MIN = 16, KNP_OP_ABS = 17,
    KNP_OP_LT = 18, KNP_OP_GT = 19, KNP_OP_LE = 20, KNP_OP_GE = 21, KNP_OP_EQ = 22,
    KNP_OP_AND = 23, KNP_OP_OR = 24, KNP_OP_NOT = 25,
    KNP_OP_SEL = 26,   /* dst = (reg[a] != 0) ? reg[b] : reg[dst]   (dst preloaded with the else-value) */
    KNP_OP_OUT = 27,   /* I_ch^a += reg[b] */
    KNP_OP_MOV = 28,
    KNP_OP_POWI = 29,  /* dst = reg[a]^b with integer literal b */
    KNP_OP_SIN = 30, KNP_OP_COS = 31, KNP_OP_TANH = 32   /* unary functions: dst = f(reg[a]) */
};

typedef struct knp_ctx knp_ctx;

typedef struct {
    int32_t dim;              /* 2 (triangles) or 3 (tetrahedra) */
    int32_t n_vertices;       /* local vertices, owned first */
    int32_t n_vertices_owned; /* == n_vertices on one GPU */
    int32_t n_cells;
    int32_t n_cells_owned;    /* owned cells come first.  The library bounds by it knp_l2_norms, the cell tag map of
                                 knp_diag_set_cell_tags, the cell maps of the volume functionals and the cells the sampler's point
                                 locator searches; the host side selects derived fields and output by the same count.  A value
                                 <= 0 or > n_cells reads as n_cells in all of these (callers that describe a whole mesh may leave it
                                 0): a rank that owns vertices but no cell cannot say so and must not use those entry points */
    const int32_t* cells;     /* host [n_cells*(dim+1)] local vertex ids */
    const double* coords;     /* host [n_vertices*dim], metres */
    const uint8_t* cell_side; /* host [n_cells] 0 = intracellular, 1 = extracellular */
    int32_t n_gamma;
    const int32_t* gamma;     /* host [n_gamma*4] (cell+, lf+, cell-, lf-), '+' = intracellular */
    const int32_t* gamma_prog;/* host [n_gamma] membrane-program id of the facet */
    int32_t n_q;              /* facet quadrature */
    const double* q_pts;      /* host [n_q*dim] barycentric coordinates on the facet */
    const double* q_w;        /* host [n_q] weights, sum 1 */
} knp_mesh_desc;

/* nodal fields (device pointers, each n_vertices doubles) */
typedef struct {
    const double* k_i[KNP_MAX_IONS];
    const double* k_e[KNP_MAX_IONS];
    const double* phi_m;
    const double* aux[KNP_MAX_AUX];
} knp_fields;

typedef struct {
    double* k_i[KNP_MAX_IONS];
    double* k_e[KNP_MAX_IONS];
    double* phi_i;
    double* phi_e;
    double* phi_m;
} knp_fields_out;

/* indices into the array filled by knp_get_sizes */
enum {
    KNP_SZ_N_NODES = 0, KNP_SZ_N_NODES_OWNED = 1, KNP_SZ_N_DOF_LOCAL = 2, KNP_SZ_N_DOF_OWNED = 3,
    KNP_SZ_NNZ = 4, KNP_SZ_N_PAIRS = 5, KNP_SZ_N_CONTRIB = 6, KNP_SZ_N_GAMMA_VERTS = 7,
    KNP_SZ_N_GAMMA_PAIRS = 8, KNP_SZ_NNZ_P = 9, KNP_SZ_N_PHI_OWNED = 10,
    KNP_SZ_NNZ_P_PHI = 11 /* entries of knp_get_precond_phi_csr */, KNP_SZ_EMI_NNZ = 12 /* entries of knp_emi_get_csr, 0 before knp_emi_setup */,
    KNP_SZ_COUNT = 16
};

/* communication hooks (multi-GPU); both receive DEVICE pointers */
typedef int (*knp_halo_fn)(void* user, double* x_local);              /* fill ghost part of x */
typedef int (*knp_allreduce_fn)(void* user, double* buf, int32_t n);  /* in-place SUM over ranks */
/* per-level exchange of a distributed AMG hierarchy; op 0: forward halo (fill the ghost entries of a level vector),
 * op 1: reverse halo (add ghost entries to their owners), op 2: all-reduce SUM of a replicated coarse vector */
typedef int (*knp_level_comm_fn)(void* user, int32_t hier, int32_t level, int32_t op, double* vec);

/* ---- lifetime ---- */
int knp_create(knp_ctx** out, const knp_mesh_desc* mesh);
int knp_destroy(knp_ctx* ctx);
const char* knp_last_error(const knp_ctx* ctx);
int knp_set_stream(knp_ctx* ctx, void* hip_stream);
int knp_set_comm(knp_ctx* ctx, knp_halo_fn halo, knp_allreduce_fn allreduce, void* user);
int knp_set_level_comm(knp_ctx* ctx, knp_level_comm_fn fn);

/* ---- native peer-to-peer exchange (multi-GPU, optional; replaces the hooks above once attached) ----
 * One kernel per exchange: it writes this rank's ghost values / reduction partials straight into the neighbours' mailboxes
 * (uncached device memory mapped over hipIpc: xGMI stores between GPUs), announces them with a sequence flag, waits for the
 * neighbours' flags (bounded) and consumes its own mailbox.  No host round trip, no library call per exchange.  The rendezvous (who are my peers, their IPC handles, where
 * my data lands in their mailbox) is done by the caller with whatever it has (torch.distributed, MPI):
 *   knp_p2p_init            once per ctx
 *   knp_p2p_plan_create     allocates this rank's mailbox of one plan, returns its 64-byte IPC handle
 *   knp_p2p_plan_connect    maps the peers' mailboxes; halo plans also get the index lists and the peers' offsets
 *   knp_p2p_attach          binds a connected plan to the fine halo, a level halo, a level's replicated all-reduce
 *                           or the reduction slots
 * All four are collective in the sense that every rank must make the same sequence of calls.  A wait that exceeds
 * the timeout sets an error that the next knp_gmres_solve / knp_p2p_test_* reports (KNP_E_STATE). */
#define KNP_P2P_HALO 0
#define KNP_P2P_ALLREDUCE 1
#define KNP_P2P_ATTACH_FINE_HALO 0
#define KNP_P2P_ATTACH_LEVEL_HALO 1
#define KNP_P2P_ATTACH_LEVEL_REPL 2
#define KNP_P2P_ATTACH_SLOTS 3
int knp_p2p_init(knp_ctx* ctx, int32_t rank, int32_t size, double timeout_seconds);
int knp_p2p_shutdown(knp_ctx* ctx);   /* drop every plan and return to the hooks (all ranks together) */
int knp_p2p_plan_create(knp_ctx* ctx, int32_t kind, int64_t n_fwd /* halo: ghost count | all-reduce: max length */,
                        int64_t n_rev /* halo: total send count */, int32_t* plan_out, void* ipc_handle_out /* host [64] */);
int knp_p2p_plan_connect(knp_ctx* ctx, int32_t plan, const void* handles /* host [size*64], one per rank */,
                         int32_t n_peers, const int32_t* peer_rank /* host, ascending */,
                         const int64_t* send_ptr /* host [n_peers+1] */, const int32_t* send_idx /* host: owned entries each peer needs */,
                         const int64_t* remote_fwd_off /* host [2*n_peers]: element offset of my values in the peer's mailbox data
                                                          area, for sequence parity 0 and 1 (the mailboxes are double buffered) */,
                         const int64_t* recv_ptr /* host [n_peers+1] */, const int32_t* recv_idx /* host: my ghost entries per peer */,
                         const int64_t* remote_rev_off /* host [2*n_peers]: the same for the reverse (ghost -> owner) direction */);
int knp_p2p_attach(knp_ctx* ctx, int32_t what, int32_t hier, int32_t level, int32_t plan /* -1 detaches */);
int knp_p2p_test_halo(knp_ctx* ctx, int32_t plan, double* x /* device */, int32_t reverse);
int knp_p2p_test_allreduce(knp_ctx* ctx, int32_t plan, double* v /* device */, int32_t n);

/* ---- description ---- */
int knp_get_sizes(const knp_ctx* ctx, int64_t* sizes /* host [KNP_SZ_COUNT] */);
int knp_get_layout(const knp_ctx* ctx, int32_t* node_i, int32_t* node_e /* host [n_vertices] each */);
int knp_get_csr_pattern(const knp_ctx* ctx, int32_t* rowptr, int32_t* colind /* host */);
/* A is held pair-major on the device; these two export it as standard CSR for checkers: rows = owned DoFs,
 * row (n,j<3) = [(nb,j),(nb,phi) for nb in the node's pairs] ++ [(cross,phi)], row (n,phi) = [(nb,0..3) ...] ++ [(cross,phi)] */
int knp_get_csr_values(const knp_ctx* ctx, double* vals /* host [nnz] */);
int knp_get_precond_csr(const knp_ctx* ctx, int32_t* rowptr, int32_t* colind, double* vals /* host */);
/* max |A_ij| over the locally stored entries (what the reference's null-space check scales by; device reduction) */
int knp_matrix_max_abs(knp_ctx* ctx, double* out /* host */);

/* ---- problem data ---- */
int knp_set_params(knp_ctx* ctx, double dt, double F, double C_M, double psi, int32_t n_ions,
                   const double* z, const double* Di, const double* De);
int knp_set_program(knp_ctx* ctx, int32_t prog_id, int32_t n_instr, const int32_t* code /* host [n_instr*4] */,
                    int32_t n_consts, const double* consts /* host */);
/* "native" when the membrane programs were compiled with hiprtc for this device (knp_jit.cpp), otherwise the reason why the
 * bytecode interpreter runs (KNP_JIT=0, no libhiprtc, compile log).  Both run on the GPU and give the same values. */
const char* knp_jit_status(knp_ctx* ctx);
/* test hook, needs neither a device nor a context: generate the HIP source for one program and compile it with hiprtc
 * for `arch` (e.g. "gfx950"); 0 on success, `log` receives the compiler log or a one-line summary */
int knp_jit_compile_check(const int32_t* code, int32_t n_instr, const char* arch, char* log, int32_t log_cap);
/* test hook, needs neither a device nor a context: the number of host threads the one-off OpenMP passes of the library use in this
 * process (KNP_HOST_THREADS, else cgroup CPU quota / affinity mask divided by LOCAL_WORLD_SIZE, at most 32; evaluated once) */
int knp_host_thread_count(void);
int knp_set_program_constants(knp_ctx* ctx, int32_t prog_id, int32_t n_consts, const double* consts);
/* Dirichlet conditions (reference: dfx.fem.dirichletbc + bcs= of assemble_*_block, KNPEMIx_problem.py:106-134,
 * KNPEMIx_solver.py:114-116): rows of the listed owned DoFs become identity rows in A and P at every assembly;
 * the caller sets b[dof] = g.  (DOLFINx also eliminates the columns; same solution.) n = 0 clears. host array. */
int knp_set_dirichlet(knp_ctx* ctx, int32_t n, const int32_t* dofs);
/* volumetric source terms dt*f (KNPEMIx_problem.py:613-614); NULL pointers mean zero. nodal, device. */
int knp_set_sources(knp_ctx* ctx, const double* const* f_i, const double* const* f_e);

/* ---- per-timestep assembly ---- */
int knp_assemble_matrix(knp_ctx* ctx, const knp_fields* fields);
/* the same assembly (assemble_matrix_block(A, a), KNPEMIx_solver.py:110-115) on the library's own stream: A depends on the previous
 * solution only, so the right-hand side chain of the step (gating update, knp_assemble_rhs, knp_gmres_prepare) can be enqueued
 * while it runs.  The fields must not be modified until the next call that needs A (knp_gmres_solve, knp_spmv, exports), which
 * joins it.  In line (== knp_assemble_matrix) on the first assembly, with vertex-block Jacobi or when kernel classes are timed. */
int knp_assemble_matrix_async(knp_ctx* ctx, const knp_fields* fields);
/* writes the owned entries [0, n_dof_owned) of b -- membrane facets this rank sees but does not own contribute to its owned rows --
 * and leaves the ghost entries [n_dof_owned, n_dof_local) as they are */
int knp_assemble_rhs(knp_ctx* ctx, const knp_fields* fields, double* b /* device [n_dof_local] */);
int knp_assemble_precond(knp_ctx* ctx, const knp_fields* fields);
/* form of the potential block of P: 0 the reference's (- (C_M/F) M_Gamma per side, sides uncoupled, KNPEMIx_problem.py:735-738),
 * 1 the potential block of A at assembly time (+ (C_M/F) M_Gamma and the phi_i-phi_e coupling, :637-638).  Before knp_assemble_precond. */
int knp_pc_set_coupled_potential(knp_ctx* ctx, int32_t on);
/* the potential block of P on node-indexed rows / columns: CSR [n_nodes_owned + 1], [KNP_SZ_NNZ_P_PHI] x 2, columns unsorted */
int knp_get_precond_phi_csr(const knp_ctx* ctx, int32_t* rowptr, int32_t* colind, double* vals);

/* ---- linear algebra ---- */
int knp_spmv(knp_ctx* ctx, const double* x, double* y); /* y(owned) = A x ; calls the halo hook first */
int knp_set_nullspace(knp_ctx* ctx, int32_t on);
int knp_project_nullspace(knp_ctx* ctx, double* v);
int knp_nullspace_test(knp_ctx* ctx, double* out_norm /* host: ||A ns||_2 */);
int knp_pc_setup(knp_ctx* ctx, int32_t kind);
int knp_pc_apply(knp_ctx* ctx, const double* r, double* z); /* r, z: [n_dof_local]; distributed contexts overwrite the ghost entries of r (see knp_gmres_solve) */
/* Additive coarse correction for near-null modes the per-GPU preconditioner blocks cannot see (constants of a
 * potential block on a connected component that the partition cuts): z += Z Einv Z^T r with Z the indicator
 * vectors of the potential DoFs of each mode. node_mode: host [n_nodes_owned], -1 = not deflated.
 * Einv: host [n_modes^2], row-major (pseudo-)inverse of Z^T A Z, identical on every rank: the potential entry of a node of
 * mode a gains sum_c Einv[a * n_modes + c] * s_c, s_c = the sum of the potential entries of r over the nodes of mode c.
 * n_modes = 0 disables.  A rejected call (KNP_E_ARG: more than 32 modes, a null array, a mode id outside -1 .. n_modes - 1)
 * changes nothing: the modes of the last accepted call stay in force.
 * Dirichlet rows: the correction is added after the copy z = r on the rows of knp_set_dirichlet, so a pinned potential row
 * that is listed in a mode receives it like any other row of that mode (and its entry of r enters s_c).  B stays non-singular
 * and the limit of the solve is unchanged, but B is no longer the identity on that row.  Callers that want the identity there
 * pass -1 for the node (cgx_hip.backend does).  The gauge projection of knp_set_nullspace, when on, follows and shifts every
 * potential row, pinned or not. */
int knp_set_deflation(knp_ctx* ctx, int32_t n_modes, const int32_t* node_mode, const double* einv);
/* AMG hierarchies (hier 0 or 1) supplied level by level (level 0 = finest = P itself, possibly restricted to a
 * field class by zero rows). All arrays HOST; copied. */
int knp_amg_reset(knp_ctx* ctx, int32_t hier, int32_t n_levels, int32_t pre_sweeps, int32_t post_sweeps, int32_t cheby_degree);
/* Optional, between knp_amg_reset and the levels: the hierarchy has nf (3 or 4) decoupled fields per node that share one
 * sparsity pattern on every level (node-synchronised aggregation: level-0 unknowns 4*node + field, coarse unknowns
 * nf*aggregate + field, rows sorted by column).  With fp32 storage the library then keeps node-blocked copies of the
 * restrictors, the coarse level operators and S (one column index per node entry, nf values behind it) and the fused cycle
 * runs on them.  The pattern is verified level by level; a level that does not have it keeps the whole hierarchy on the
 * scalar kernels (KNP_ST_BLOCKED tells).  What PCGAMG/hypre reach with a block size of the matrix (MatSetBlockSize) for the
 * reference's preconditioner matrix (KNPEMI/KNPEMIx_solver.py:78-101). */
int knp_amg_set_node_fields(knp_ctx* ctx, int32_t hier, int32_t nf);
int knp_amg_set_level(knp_ctx* ctx, int32_t hier, int32_t level, int32_t n_rows, int32_t n_cols_halo,
                      const int32_t* A_rowptr, const int32_t* A_colind, const double* A_vals,
                      const double* inv_diag, double lambda_max,
                      int32_t n_coarse,
                      const int32_t* P_rowptr, const int32_t* P_colind, const double* P_vals,
                      const int32_t* R_rowptr, const int32_t* R_colind, const double* R_vals);
/* distributed levels: replace the prolongator by one that also has rows for the ghost entries (n_rows_P = local size).  The
 * ghost part of the iterate then stays current through the coarse correction and the halo before the first post-smoothing
 * step is skipped. */
int knp_amg_set_level_prolongator(knp_ctx* ctx, int32_t hier, int32_t level, int32_t n_rows_P, const int32_t* P_rp,
                                  const int32_t* P_ci, const double* P_v);
/* distributed hierarchy: `distributed` != 0 -> the level operator has ghost columns (n_cols_halo local columns);
 * repl_n > 0 -> the next level is replicated on all ranks with repl_n unknowns */
int knp_amg_set_level_mode(knp_ctx* ctx, int32_t hier, int32_t level, int32_t distributed, int32_t repl_n);
int knp_amg_set_coarse(knp_ctx* ctx, int32_t hier, int32_t n, const double* dense_inverse /* host [n*n] row-major */);
/* optional, per level with a coarser level below it: S = (I - c2 Dinv A) Pprol with c2 = 1 / (0.6 lambda_max), CSR with n_rows rows
 * (HOST arrays, copied).  With S on every level, V(1,1) / Chebyshev degree 1 and level 0 on the library's own P
 * (knp_amg_use_native_level0) the cycle runs in its fused form: pre-smoothing + residual as one gather, prolongation +
 * post-smoothing as one gather per level (same operator as the unfused cycle; KNP_FUSED=0 selects the latter). */
int knp_amg_set_level_smoothed(knp_ctx* ctx, int32_t hier, int32_t level, int32_t n_rows, const int32_t* S_rowptr, const int32_t* S_colind,
                        const double* S_vals);
/* optional, intermediate levels (1 .. n_levels-2) of a single-GPU hierarchy whose cycle runs fused: both legs as plain products,
 * Rt = R (I - c A Dinv) [n_coarse x n] and U = [c Dinv (2I - c A Dinv) | S] [n x (n + n_coarse)] (cgx_hip/amg.py
 * coarse_fused_operators); replaces restriction + residual and the three-vector up-leg of those levels */
int knp_amg_set_level_coarse_fused(knp_ctx* ctx, int32_t hier, int32_t level, int32_t Rt_rows, const int32_t* Rt_rowptr, const int32_t* Rt_colind,
                                   const double* Rt_vals, int32_t U_rows, const int32_t* U_rowptr, const int32_t* U_colind, const double* U_vals);
/* level 0 == the library's own P (owned block): use its pair-major storage and node kernels instead of the uploaded
 * CSR. mode: 0 off, 1 all four fields, 2 ion fields only, 3 potential only, 4 potential only on node-indexed vectors with the
 * UPLOADED level-0 operator (one GPU; the operator may couple the two sides of the membrane, knp_pc_set_coupled_potential) */
int knp_amg_use_native_level0(knp_ctx* ctx, int32_t hier, int32_t mode);
/* mixed-precision preconditioner: level operators, transfer operators and P on level 0 are STORED in fp32
 * (converted on load); every vector, the dense coarse inverse, the system matrix and the Krylov process stay fp64.
 * Call before uploading a hierarchy. */
int knp_amg_set_precision(knp_ctx* ctx, int32_t fp32_storage);
/* optional: start ||B b|| of the next knp_gmres_solve(ctx, b, ...) on a side stream now (b complete, not to be modified until
 * the solve); it then overlaps whatever the caller enqueues next, typically knp_assemble_matrix.  No-op before the first solve
 * and on distributed contexts whose exchanges go through the hooks (with the native peer-to-peer plans attached everywhere it
 * runs: the exchange kernels are then ordered on the side stream on every rank).  Any other call that touches the
 * preconditioner or b joins / discards it. */
int knp_gmres_prepare(knp_ctx* ctx, const double* b);
/* GMRES(restart), 1 <= restart <= 55 (the per-iteration reduction carries restart + 2 values in the library's 57 Gram-Schmidt
 * slots; anything larger is KNP_E_ARG).  b and x are [n_dof_local] device vectors.  On distributed contexts the GHOST entries
 * [n_dof_owned, n_dof_local) of b -- and of r in knp_pc_apply, b in knp_gmres_prepare -- are OVERWRITTEN by the halo exchange of
 * the preconditioner's fused level-0 leg although the arguments are const-qualified (the owned entries are never written);
 * on one GPU n_dof_local == n_dof_owned and nothing is written.
 * On one GPU without hooks, Dirichlet rows or deflation the first iteration of every cycle is enqueued before the host reads the
 * cycle's initial residual norm (one wait per cycle start less; same kernels, order and results; KNP_GMRES_AHEAD=0, read at
 * knp_pc_setup, restores the in-order form).  KNP_ST_READBACK and KNP_ST_ALLREDUCE count what ran, a discarded iteration included.
 * The kernel that builds v_{j+1} returns at once on an iteration whose residual estimate already meets the tolerance (nobody reads
 * that vector; the host takes its decisions from the same values as before; KNP_UPDATE_EARLY=0, read at knp_pc_setup: off). */
int knp_gmres_solve(knp_ctx* ctx, const double* b, double* x, double rtol, double atol, int32_t max_it,
                    int32_t restart, int32_t* its, double* rnorm, int32_t* reason);
/* Flexible GMRES(restart): what the reference gets from PETSc with ksp_type fgmres, or gmres with norm_type unpreconditioned
 * (right preconditioning), both passed through from the YAML (KNPEMIx_solver.py:80-87, 212, 279).  Classical Gram-Schmidt; per
 * iteration z_j = B v_j is kept in a second basis Z (so B may change between applications), w = A z_j, and the cycle ends with
 * x += Z y.  Same arguments, limits, divergence test (1e5 ||b||) and reason codes as knp_gmres_solve, but
 *   norm:  the TRUE residual: stops when ||b - A x||_2 <= max(rtol ||b||_2, atol) (PETSc KSPConvergedDefault, with or without a
 *          non-zero initial guess); *rnorm is that norm (the Givens estimate of the last iteration).
 *   gauge: with the null space on (knp_set_nullspace) each cycle's correction Z y is added without its component along the constant
 *          potential, so the null-space component of x is that of the initial guess -- what knp_gmres_solve leaves too, whose
 *          Krylov vectors are projected.  B's output is not projected (A ns = 0: w = A z_j does not see it).
 *   ghosts: as knp_gmres_solve -- on distributed contexts the ghost entries of b, and of the basis vectors passed to the
 *          preconditioner, are overwritten by halo exchanges; the owned entries of b are never written.
 * Z costs restart * n_dof_local doubles of device memory, allocated on the first flexible solve (none with KNP_PC_NONE: Z is V).
 * On one GPU without Dirichlet rows the first stage of each reduction runs inside the SpMV (cycles up to 8 vectors; KNP_SPMV_DOTS=0
 * turns it off), and the restart residual b - A x comes with its norm from the same launch.
 * knp_fgmres_prepare: optional, the counterpart of knp_gmres_prepare -- ||b|| of the next knp_fgmres_solve(ctx, b, ...) on a side
 * stream now (b complete and not modified until the solve), overlapping whatever the caller enqueues next.  One GPU only; a no-op
 * on distributed contexts, whose solve computes it in line. */
int knp_fgmres_prepare(knp_ctx* ctx, const double* b);
int knp_fgmres_solve(knp_ctx* ctx, const double* b, double* x, double rtol, double atol, int32_t max_it,
                     int32_t restart, int32_t* its, double* rnorm, int32_t* reason);

/* ---- state transfer ---- */
int knp_pack(knp_ctx* ctx, const knp_fields_out* fields, double* x);
int knp_unpack(knp_ctx* ctx, const double* x, const knp_fields_out* fields);
/* Fused tail of a solve (optional; without these two calls every launch is as before).
 * knp_set_unpack_target: where knp_unpack will put the solution (all nine pointers set; NULL clears the registration).  With a
 * target registered, knp_gmres_solve ends in ONE kernel that adds the last correction to x, unpacks x into the target (exactly what
 * knp_unpack writes) and keeps the node-indexed concentration copy the next matrix assembly reads -- when the update belongs to the
 * cycle after which the solve returns and has at most 8 columns, on one GPU without hooks, peer-to-peer plans, deflation, Dirichlet
 * rows or kernel-class timing beyond the SpMV's (KNP_FUSED_TAIL=0, read at knp_pc_setup: never).  x is bit for bit what the
 * separate kernels give.  knp_unpack(ctx, x, fields) of that x into that target then returns at once.  The library forgets that the
 * target is current at every entry that writes x or the fields (any later solve, knp_project_nullspace, knp_pack,
 * knp_set_dirichlet, knp_pc_setup, knp_assemble_precond, this call); it cannot see the CALLER write x or the target between the solve
 * and knp_unpack: register again (or clear) after doing so.
 * knp_fields_unchanged: the caller's promise that nobody has written the concentration fields of the target since the last
 * knp_unpack.  One shot: the next knp_assemble_matrix(_async) -- given the same six concentration pointers -- then skips its
 * node-indexed copy pass if the solve's tail has already written it, and the promise is consumed either way.
 * KNP_ST_FUSED_TAILS / KNP_ST_KNOD_SKIPS count both.
 * Assembly ahead (KNP_ASM_AHEAD, read at knp_pc_setup: 0 never, 1 (default) where the SpMV's streams and the second buffer below fit
 * the 256 MiB Infinity Cache together, 84 B per node pair + 128 B per membrane vertex pair, 2 whatever the size).  A matrix assembly that skipped the copy pass ARMS the context: the
 * caller has just shown the pattern "unpack, fields untouched, assemble".  While armed, a knp_gmres_solve that ends in the fused tail
 * enqueues the next step's matrix assembly itself, on the library's assembly stream behind its last kernel, reading the concentration
 * fields and phi_m of the registered target -- when only the solution-dependent entries are due (same dt as the last assembly, not
 * KNP_ASM_FULL), with an AMG preconditioner, no Dirichlet rows, one GPU without hooks or peer-to-peer plans and no kernel-class timing
 * beyond the SpMV's.  It writes a second buffer (same size as the solution-dependent entries, allocated at the first such assembly; if
 * that fails the context goes on without the feature), so the matrix of the step just solved stays what knp_spmv, knp_get_csr_values
 * and every other reader see.  The next knp_assemble_matrix(_async) ADOPTS the result -- swaps the buffers and launches nothing;
 * counted in KNP_ST_KNOD_SKIPS there -- iff the promise above was given, the six concentration pointers and phi_m are the target's
 * and dt and the conditions still hold.  Otherwise the result is DISCARDED, the context disarmed, and the assembly runs as without
 * the feature: a caller that writes the fields every step pays one wasted assembly each time the pattern breaks, plus one after the
 * last step of a run.  Every entry listed above as forgetting the target, and knp_set_params, discards a pending result as well.
 * Between the solve and the promise the library's kernels may READ the fields while the caller writes them: harmless, since no index
 * depends on a value and a caller that wrote withholds the promise, so what was read is never used.
 * KNP_ST_AHEAD_ADOPTED / KNP_ST_AHEAD_DISCARDED count both outcomes. */
int knp_set_unpack_target(knp_ctx* ctx, const knp_fields_out* fields /* or NULL */);
int knp_fields_unchanged(knp_ctx* ctx);
/* test hook: the node-indexed concentration copy {k0, k1, k2, 0} per local node, host [4 * n_nodes] (synchronises; KNP_E_STATE on
 * contexts whose assembly reads per-cell means instead) */
int knp_get_nodal_conc(knp_ctx* ctx, double* out);
int knp_hh_update(knp_ctx* ctx, const double* phi_m, double* n, double* m, double* h, int32_t count,
                  double dt, double phi_rest, int32_t rush_larsen, int32_t substeps);
/* Membrane state variables: nodal fields that a mechanism declares and the library advances after every solve.  Every state is one
 * bytecode program (the opcodes and limits of knp_set_program) that reads phi_m, the concentrations, the coordinates, constants and the
 * aux fields -- among them the states themselves, each under the aux slot given for it.  This is HodgkinHuxley.update_gating_variables
 * (KNPEMIx_ionic_model.py:605-671) with the rates handed in: alpha_n .. beta_h there (:617-622) are the OUT 0 / OUT 1 of three gates.
 * knp_state_reset: forget all state programs and make room for n_states of them, 0 .. KNP_MAX_AUX (the reference's Function(V) per
 *   gate in HodgkinHuxley._init, :470-480).  Synchronous.
 * knp_state_set_program: the program of state `slot`.  kind 0, a gate dy/dt = alpha (1 - y) - beta y: KNP_OP_OUT 0 = alpha,
 *   KNP_OP_OUT 1 = beta (the rate expressions of :617-622).  kind 1, a general state: KNP_OP_OUT 0 = dy/dt.  aux_index: the aux slot
 *   under which programs read this state (one state per slot).  All programs together hold at most KNP_STATE_MAX_INSTR instructions and
 *   KNP_STATE_MAX_CONSTS constants.  Host only; the code is uploaded by the next knp_state_update.
 * knp_state_set_constants: new constants for the program of `slot`, same count (the per-step refresh of a time-dependent
 *   dfx.fem.Constant).  They travel as kernel arguments of the next update: no copy, no synchronisation.
 * knp_state_update: one PDE step of all states at the vertices 0 .. count-1 (count <= the local vertices, ghosts included, as
 *   knp_hh_update; no communication), enqueued.  state[s] is the device buffer of slot s; fields->phi_m is read, fields->k_i / k_e only
 *   when a program reads a concentration (null there is then KNP_E_ARG), fields->aux[k] for the slots that are not states (null reads as
 *   0).  Gates: alpha, beta evaluated once from the values at the start of the step, then y <- y_inf + (y - y_inf) exp(-dt (alpha + beta))
 *   (rush_larsen; the sub-steps collapse, :640-655; a vertex where alpha + beta == 0 keeps its y) or `substeps` forward-Euler steps y += dto alpha (1 - y) - dto beta y (:656-671).
 *   General states: `substeps` forward-Euler steps, the program evaluated again in each; within a sub-step every program reads the
 *   states as they stood at its beginning.  With rush_larsen the gates keep their start-of-step value until the end of the step.
 *   The same inputs give the same bits on every run.
 * Errors: KNP_E_ARG for a slot outside 0 .. n_states-1, a kind other than 0 / 1, an aux_index outside 0 .. KNP_MAX_AUX-1 or taken by
 *   another state, an invalid or too long program, a constant count mismatch, a null pointer, count < 0 or beyond the local vertices,
 *   dt <= 0, substeps < 1; KNP_E_STATE for an update with no states or a slot without a program.  Nothing is launched then. */
int knp_state_reset(knp_ctx* ctx, int32_t n_states);
int knp_state_set_program(knp_ctx* ctx, int32_t slot, int32_t kind /* 0 gate, 1 general */, int32_t aux_index, int32_t n_instr,
                          const int32_t* code /* host [n_instr*4] */, int32_t n_consts, const double* consts /* host */);
int knp_state_set_constants(knp_ctx* ctx, int32_t slot, int32_t n_consts, const double* consts /* host */);
int knp_state_update(knp_ctx* ctx, const knp_fields* fields, double* const* state /* host [n_states] device pointers */, int32_t count,
                     double dt, int32_t rush_larsen, int32_t substeps);
int knp_l2_norms(knp_ctx* ctx, const double* phi_i, const double* phi_e, double* out /* host [2]: squared, owned cells */);
/* Per-tag diagnostics.  A tag map lists items sorted by a dense tag index: seg_ptr[t] .. seg_ptr[t+1]-1 are the positions of tag t in
 * `cells` / `facets`; seg_ptr[0] == 0, non-decreasing; every item at most once.  The maps are uploaded once (synchronous); the
 * integrals are enqueued on the library's stream, write the caller's device buffer and never wait for the device.  No atomics: the
 * same inputs give the same bits on every run.  Each rank integrates what it lists; the caller sums over ranks.
 * knp_diag_set_cell_tags: owned cells only (ids < n_cells_owned).
 * knp_diag_volume_integrals: out[3t + j] = sum over the cells c of tag t of |c|/(d+1) * sum over the vertices of c of k_j on the
 *   cell's side (fields->k_i for intracellular cells, k_e for extracellular ones): the exact P1 integral, i.e. assemble_scalar of
 *   k_j*dx(tag) in print_conservation (KNPEMIx_problem.py:821-840). */
int knp_diag_set_cell_tags(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr /* host [n_tags+1] */,
                           const int32_t* cells /* host [seg_ptr[n_tags]] */);
int knp_diag_volume_integrals(knp_ctx* ctx, const knp_fields* fields, double* out /* device [n_tags*3] */);
/* knp_diag_set_facet_tags: membrane facets by their index in knp_mesh_desc.gamma; the caller selects them (one owner per facet, e.g.
 *   the rank owning the facet's first vertex) and may give several membrane tags the same index.
 * knp_diag_set_program: one bytecode program (the opcodes of knp_set_program, at most KNP_DIAG_MAX_CONSTS constants), kept apart from
 *   the assembly's program table; knp_diag_set_program_constants replaces its constants on the host (they travel as kernel arguments
 *   of the next knp_diag_membrane_integral: no copy, no synchronisation).
 * knp_diag_membrane_integral: out[t] = sum over the facets F of tag t and the quadrature points q of q_w |F| times the sum of the
 *   program's outputs at q (bytecode interpreter): assemble_scalar(stim_ufl_expr*dS(stimulus_tags)) of the stimulus trace
 *   (KNPEMIx_solver.py:580-582, 605-607). */
int knp_diag_set_facet_tags(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr /* host [n_tags+1] */,
                            const int32_t* facets /* host [seg_ptr[n_tags]] */);
int knp_diag_set_program(knp_ctx* ctx, int32_t n_instr, const int32_t* code /* host [n_instr*4] */, int32_t n_consts,
                         const double* consts /* host */);
int knp_diag_set_program_constants(knp_ctx* ctx, int32_t n_consts, const double* consts /* host */);
int knp_diag_membrane_integral(knp_ctx* ctx, const knp_fields* fields, double* out /* device [n_tags] */);
/* knp_diag_set_flux_facets: a tag map of membrane facets like knp_diag_set_facet_tags, kept apart from it (both may be live), and an
 *   optional axis-aligned box mask: box_lo / box_hi are host [3] (axes >= dim ignored, -inf / +inf leave an axis open) or both NULL.
 *   Builds on the host (OpenMP) and uploads one time-invariant record per listed facet: the vertices of its intracellular cell T+
 *   (gamma column 0) and extracellular cell T- (column 2), g_a = grad(lambda_a) . n per side (n_0 the unit normal out of T+,
 *   n_1 = -n_0), W0 = |F| sum_q q_w m(x_q) and W_b = |F| sum_q q_w m(x_q) lambda_b(q) with m = 1 where lo < x < hi on every axis (strict),
 *   else 0, at the points of the mesh's facet rule.  128 bytes per facet in 3D, 112 in 2D.  Synchronous.  KNP_E_MESH when a listed
 *   facet's T- does not contain the facet or a cell is flat; the map is then unset.
 * knp_diag_membrane_fluxes: the molar flux of ion k out of side s (0 intra, 1 extra) through the facets of tag t [mol/s],
 *   out[6t + 3s + k] = sum_F -D[k] (W0 sum_a g_a c(v_a) + z_over_psi[k] (sum_b W_b c(f_b)) (sum_a g_a phi(v_a)))
 *   with c = fields->k_i[k], phi = phi_i on T+ for s = 0 and c = fields->k_e[k], phi = phi_e on T- for s = 1: the integral over the
 *   facets of mask * (-D_k (grad c_k + (z_k/psi) c_k grad phi)) . n_s of create_flux_forms (utils/calc_fluxes.py:85-88); positive = ions
 *   leave that side's domain.  D and z_over_psi are host [3] and travel as kernel arguments.  fields->phi_m and aux are not read. */
int knp_diag_set_flux_facets(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr /* host [n_tags+1] */,
                             const int32_t* facets /* host [seg_ptr[n_tags]] */, const double* box_lo /* host [3] or NULL */,
                             const double* box_hi /* host [3] or NULL */);
int knp_diag_membrane_fluxes(knp_ctx* ctx, const knp_fields* fields, const double* phi_i /* device [n_vertices] */,
                             const double* phi_e /* device [n_vertices] */, const double* D /* host [3] */,
                             const double* z_over_psi /* host [3] */, double* out /* device [n_tags*6] */);
/* knp_diag_set_phim_facets: a tag map of membrane facets like knp_diag_set_facet_tags, kept apart from it and from the flux map (all
 *   three may be live); validated and replaced by the same rules.  Synchronous.
 * knp_diag_membrane_potential: with phi = fields->phi_m (nodal; the other fields are not read) and d the number of facet vertices,
 *   out[3t] = sum over the facets F of tag t of |F|/d * sum_a phi(v_a(F)) (the exact P1 integral, V m^(d-1)), out[3t + 1] / out[3t + 2] =
 *   the minimum / maximum of phi over all vertices of the tag's facets.  A tag without facets gives (0, +inf, -inf): the caller reduces
 *   over ranks by sum / min / max and divides by the tag's area for the mean.  A NaN at a vertex of a tag's facets makes that
 *   tag's integral NaN but not its minimum and maximum (fmin / fmax drop it): test out[3t] to detect a diverged field.  Partials are combined in a fixed order (one wave per tag
 *   of at most 64 chunks of 128 facets, one workgroup per longer tag): the same bits on every run.  KNP_E_STATE before a map is set,
 *   KNP_E_ARG for a null argument; n_tags == 0 is a successful no-op. */
int knp_diag_set_phim_facets(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr /* host [n_tags+1] */,
                             const int32_t* facets /* host [seg_ptr[n_tags]] */);
int knp_diag_membrane_potential(knp_ctx* ctx, const knp_fields* fields, double* out /* device [n_tags*3] */);
/* Activation map: per membrane vertex when phi_m first (and last) rose through a threshold, when it fell back, its peak and its
 * steepest upstroke; per membrane facet the conduction velocity; per tag a summary.  The detector's state belongs to the caller
 * (device arrays passed by pointer; the library keeps none): v_last [n], state [7][n] (row r of vertex j at state[r*n + j]; rows
 * t_first, t_last_up, t_repol, v_peak, t_peak, dvdt_max, t_dvdt) and count [n].  vertex [n]: local vertex ids (device int32), e.g. the
 * unique vertices of the selected tags' owned membrane facets in ascending order; phi_m: the nodal field, device [n_vertices].
 * knp_activation_arm: v_last = v_peak = phi_m(vertex), t_peak = t, dvdt_max = -inf, t_first = t_last_up = t_repol = t_dvdt = NaN,
 *   count = 0.
 * knp_activation_step: one interval [t0, t1] with v0 = v_last, v1 = phi_m(vertex), h = t1 - t0, in this order:
 *   1. upward crossing iff v0 < thr_up && v1 >= thr_up: tx = t0 + (thr_up - v0)/(v1 - v0) h, count += 1, t_first = tx at the first
 *      one, t_last_up = tx always;
 *   2. repolarisation iff count > 0 (after 1), t_repol still NaN and v0 >= thr_down && v1 < thr_down:
 *      t_repol = t0 + (v0 - thr_down)/(v0 - v1) h (1 needs v1 > v0 and 2 needs v1 < v0: never both in one interval);
 *   3. peak: v1 > v_peak (strict: the first of equal maxima stays) sets v_peak = v1, t_peak = t1;
 *   4. steepest upstroke: s = (v1 - v0)/h > dvdt_max sets dvdt_max = s, t_dvdt = t0 + h/2;
 *   5. v_last = v1.
 *   All comparisons are plain IEEE: a NaN phi_m records nothing in the interval that ends at it and, being the next v_last, nothing in
 *   the one after it, and leaves no false crossing.  A listed vertex outside [0, n_vertices) reads as NaN.
 * Both run one kernel on the context's stream, one lane per listed vertex, with no host copy and no synchronisation.  KNP_E_ARG (with
 * knp_last_error text, the buffers untouched) for a null pointer, n < 0, t1 <= t0 or a non-finite threshold; n == 0 is a successful no-op.
 * knp_activation_velocity: T is a nodal activation time, device [n_vertices], NaN where a vertex did not fire or is not listed;
 *   facets [n_facets]: indices into the Gamma list of knp_create (device int32).  Per listed facet out[(1+dim) i] = speed [m/s] and
 *   out[(1+dim) i + 1 ...] = the unit direction of propagation [dim], from the surface gradient g of T's P1 interpolant: speed = 1/|g|,
 *   direction = g/|g|.  2D (segments): e = x1 - x0, L = |e|, d = T1 - T0, speed = L/|d|, direction = sign(d) e/L.  3D (triangles):
 *   e1 = x1 - x0, e2 = x2 - x0, a = e1.e1, b = e1.e2, c = e2.e2, det = a c - b^2, d1 = T1 - T0, d2 = T2 - T0,
 *   g = [(c d1 - b d2) e1 + (a d2 - b d1) e2]/det, |g|^2 = (c d1^2 - 2 b d1 d2 + a d2^2)/det.  A facet is valid iff all its T are
 *   finite, its measure is not zero and |g| > 0 (2D: d != 0); an invalid facet, and a listed index outside the Gamma list, writes NaN in all 1 + dim slots.
 *   KNP_E_ARG for a null pointer or n_facets < 0; n_facets == 0 is a successful no-op.
 * knp_diag_set_activation_facets: a tag map of membrane facets like knp_diag_set_phim_facets (same validation, same combine rule),
 *   kept apart from the other maps.  Synchronous.
 * knp_diag_activation: out[5t ..] = over the facets F of tag t (sum |F| [F valid], sum |F| speed(F) [F valid], min and max of T over
 *   the vertices of the facets (fmin / fmax: NaN dropped), sum |F|/d * number of F's vertices with a finite T).  A tag without facets
 *   gives (0, 0, +inf, -inf, 0).  No atomics, partials combined in a fixed order: the same bits on every run.  KNP_E_STATE before a map
 *   is set, KNP_E_ARG for a null argument; n_tags == 0 is a successful no-op. */
int knp_activation_arm(knp_ctx* ctx, int32_t n, const int32_t* vertex /* device [n] */, const double* phi_m /* device [n_vertices] */,
                       double t, double* v_last /* device [n] */, double* state /* device [7*n] */, int32_t* count /* device [n] */);
int knp_activation_step(knp_ctx* ctx, int32_t n, const int32_t* vertex /* device [n] */, const double* phi_m /* device [n_vertices] */,
                        double t0, double t1, double thr_up, double thr_down, double* v_last /* device [n] */,
                        double* state /* device [7*n] */, int32_t* count /* device [n] */);
int knp_activation_velocity(knp_ctx* ctx, int32_t n_facets, const int32_t* facets /* device [n_facets] */,
                            const double* T /* device [n_vertices] */, double* out /* device [n_facets*(1+dim)] */);
int knp_diag_set_activation_facets(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr /* host [n_tags+1] */,
                                   const int32_t* facets /* host [seg_ptr[n_tags]] */);
int knp_diag_activation(knp_ctx* ctx, const double* T /* device [n_vertices] */, double* out /* device [n_tags*5] */);
/* Field sampling: P1 evaluation of nodal fields at arbitrary points (grids, slices), located on the device once per point set.
 * Rule: cell T contains p iff all dim+1 barycentric weights of p in T are >= -1e-9; among the containing cells the lowest local cell
 *   index wins; the stored weights are clipped to [0, 1] and renormalised to sum 1.  Only owned cells are searched, and with side 0 / 1
 *   only the intracellular / extracellular ones (-1: any).  This is the rule of cgx_hip/output.py::_barycentric.
 * knp_sample_plan_create: the caller sorts the points into a uniform lattice of bins: bin index along axis k =
 *   min(max(floor((p_k - bin_origin[k]) / bin_size[k]), 0), bin_shape[k] - 1), bins numbered row-major (last axis fastest),
 *   bin_pts[bin_ptr[b] .. bin_ptr[b+1]-1] the points of bin b.  One cell-major kernel tests every cell against the points of the bins its
 *   bounding box overlaps (32-bit integer atomicMin of the cell index per hit: the same bits on every run), one point-major kernel
 *   stores vertices, weights and side per point.  Work: cells + points + tests inside overlapping bins.  Synchronous; the plan keeps
 *   12 (dim+1) + 5 bytes of device memory per point.  *plan receives an id >= 0 that belongs to the context.
 * knp_sample_plan_get: the winning cell (-1: none) and the weights of every point, in the caller's order.
 * knp_sample: out[f*n_points + pt] = sum_a w_a F[f][v_a] in the order a = 0 .. dim, F[f] = f_i[f] where the winning cell is
 *   intracellular, f_e[f] where it is extracellular; `fill` where the point is in no cell.  Enqueued on the library's stream, no
 *   host copy, no synchronisation.  f_i / f_e (or an entry) may be null when no located point of the plan needs that side.
 * knp_sample_plan_destroy: frees the plan (waits for the stream first); knp_destroy frees the plans that are left.
 * Errors, all KNP_E_ARG with nothing launched: n_points <= 0, a null array, side outside -1 .. 1, a lattice whose shape does not
 *   multiply to n_bins or whose sizes are not positive, bin_ptr not running from 0 to n_points or decreasing, bin_pts not a permutation,
 *   a point that is not finite or not in the bin its coordinates give, an unknown plan, n_fields <= 0, a null field that a located point
 *   needs. */
int knp_sample_plan_create(knp_ctx* ctx, int32_t n_points, const double* pts /* host [n_points*dim], metres */,
                           int32_t side /* -1 any cell, 0 intracellular only, 1 extracellular only */, int32_t n_bins,
                           const int32_t* bin_ptr /* host [n_bins+1] */, const int32_t* bin_pts /* host [n_points] */,
                           const double* bin_origin, const double* bin_size, const int32_t* bin_shape /* host [dim] each */,
                           int32_t* plan /* host */);
int knp_sample_plan_get(knp_ctx* ctx, int32_t plan, int32_t* cell /* host [n_points] */, double* w /* host [n_points*(dim+1)] */);
int knp_sample(knp_ctx* ctx, int32_t plan, int32_t n_fields, const double* const* f_i, const double* const* f_e /* host [n_fields]
               device pointers, [n_vertices] doubles each */, double fill, double* out /* device [n_fields*n_points] */);
int knp_sample_plan_destroy(knp_ctx* ctx, int32_t plan);
/* Volume functionals: per-tag integrals over cells of one bytecode program (the opcodes of knp_set_program) evaluated at the points
 * of a simplex quadrature rule.  A functional is a plan that belongs to the context, like a sampling plan; several may be live.
 * knp_functional_create: a tag map of owned cells like knp_diag_set_cell_tags (cells of either side, each at most once), the rule
 *   (q_bary: dim+1 barycentric coordinates per point in the order of the cell's vertices; q_w sums to 1), the program with at most
 *   KNP_DIAG_MAX_CONSTS constants, and per aux slot what it holds: aux_deriv[k] == -1 the field fields->aux[k] itself, a in 0 .. dim-1
 *   its derivative d/dx_a.  Synchronous.  *id receives an id >= 0.
 * knp_functional_set_constants: replaces the constants on the host; they travel as kernel arguments of the next evaluation (no
 *   copy, no synchronisation).
 * knp_functional_eval: out[t*n_out + j] = sum over the cells T of tag t of |T| sum_q q_w[q] OUT_j(program at point q of T).  There
 *   KNP_OP_KI a / KNP_OP_KE a / KNP_OP_PHIM read the P1 interpolant of fields->k_i[a] / k_e[a] / phi_m at T's vertices, KNP_OP_X a
 *   the point's coordinate, KNP_OP_AUX k the interpolant of fields->aux[k] or, where aux_deriv[k] == a, the derivative
 *   sum_b grad(lambda_b)_a (f(v_b) - f(v_0)) of that field on T (constant per cell; the gradients come from the cell's coordinates
 *   inside the kernel, and the differences are taken first, so a field's constant offset does not cost digits).  Only the pointers of slots the code reads are used: the others may be null.  One cell per lane, 128 cells per block,
 *   the interpreter's register file in LDS (1 KiB per register the program uses, at most 48 KiB); partials are combined in a fixed
 *   order (one wave per tag of at most 64 chunks of 128 cells, one workgroup per longer tag): the same bits on every run.
 *   Enqueued on the library's stream; never waits for the device.
 * knp_functional_destroy: frees the plan (waits for the stream first); knp_destroy frees the plans that are left.
 * Errors leave nothing launched and no plan: KNP_E_ARG for a null argument, n_q outside 1 .. KNP_FUNCTIONAL_MAX_Q, n_out outside
 *   1 .. 3, n_aux outside 0 .. KNP_MAX_AUX, an aux_deriv outside -1 .. dim-1, an invalid or empty program, one that reads an aux slot
 *   >= n_aux or writes an output >= n_out, more than KNP_DIAG_MAX_CONSTS constants or another count in set_constants, an unknown id,
 *   a cell that is not owned or listed twice, a seg_ptr that does not start at 0 or decreases, in eval a null pointer of a slot the
 *   code reads; KNP_E_MESH when a derivative is bound and a listed cell is flat (zero determinant, or gradients that are not
 *   finite; checked on the host at create).  n_tags == 0 is a successful no-op. */
int knp_functional_create(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr /* host [n_tags+1] */,
                          const int32_t* cells /* host [seg_ptr[n_tags]] */, int32_t n_q, const double* q_bary /* host [n_q*(dim+1)] */,
                          const double* q_w /* host [n_q] */, int32_t n_instr, const int32_t* code /* host [n_instr*4] */,
                          int32_t n_consts, const double* consts /* host */, int32_t n_aux, const int32_t* aux_deriv /* host [n_aux] */,
                          int32_t n_out /* 1..3 */, int32_t* id /* host */);
int knp_functional_set_constants(knp_ctx* ctx, int32_t id, int32_t n_consts, const double* consts /* host */);
int knp_functional_eval(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out /* device [n_tags*n_out] */);
int knp_functional_destroy(knp_ctx* ctx, int32_t id);
/* Membrane functionals: per-tag integrals over membrane facets of one bytecode program evaluated at the points of a facet rule, with
 * one-sided gradients, the facet normal and normal derivatives.  A plan that belongs to the context, like a volume functional (ids
 * of their own; a destroyed id is reused); several may be live.
 * knp_membrane_functional_create: a facet map like knp_diag_set_facet_tags (indices into the Gamma list of knp_create, each at most
 *   once), the rule (q_pts: dim barycentric coordinates per point in the order of the facet's vertices, the vertices of the '+' cell
 *   without the opposite one; q_w sums to 1), the program with at most KNP_DIAG_MAX_CONSTS constants, and per aux slot its mode:
 *     -1       the field fields->aux[k] itself, interpolated on the facet
 *     a        d/dx_a of that field on the intracellular ('+') cell of the facet, a in 0 .. dim-1
 *     3 + a    d/dx_a on the extracellular ('-') cell
 *     6 / 7    d/dn on the intracellular / extracellular cell, each along the normal that points out of that cell
 *     8 + a    component a of the unit normal n_i that points out of the intracellular cell; the slot needs no field pointer
 *   n_i = -grad(lambda_opp) / |grad(lambda_opp)| with lambda_opp the barycentric coordinate of the intracellular cell's vertex off the
 *   facet, and n_e = -n_i: the rule and the signs of knp_diag_membrane_fluxes.  Synchronous: builds one record of 32 bytes per listed
 *   facet (its vertices and the opposite vertex of either cell).  *id receives an id >= 0.
 * knp_membrane_functional_set_constants: replaces the constants on the host; they travel as kernel arguments of the next evaluation.
 * knp_membrane_functional_eval: out[t*n_out + j] = sum over the facets F of tag t of |F| sum_q q_w[q] OUT_j(program at point q of F);
 *   the outputs are not summed together.  KNP_OP_KI a / KNP_OP_KE a / KNP_OP_PHIM read the P1 interpolant of fields->k_i[a] / k_e[a] /
 *   phi_m at F's vertices (every field is an array over all vertices), KNP_OP_X a the point's coordinate, KNP_OP_AUX k what the slot's
 *   mode says.  A derivative is sum_{b>=1} g_b (f(v_b) - f(v_0)) over the cell's vertices with v_0 the facet's first vertex and
 *   g_b = grad(lambda_b)_a or grad(lambda_b) . n, constant on the facet: the gradients come from the coordinates inside the kernel, and
 *   the differences are taken first, so a field's constant offset costs no digits.  Only the pointers of slots the code reads are
 *   used.  One facet per lane, 128 per block, the interpreter's register file in LDS (1 KiB per register the program uses, at most
 *   48 KiB); partials are combined in a fixed order (one wave per tag of at most 64 chunks of 128 facets, one workgroup per longer
 *   tag): the same bits on every run.  Enqueued on the library's stream; never waits for the device.
 * knp_membrane_functional_destroy: frees the plan (waits for the stream first); knp_destroy frees the plans that are left.
 * Errors leave nothing launched and no plan: KNP_E_ARG for a null argument, n_q outside 1 .. KNP_FUNCTIONAL_MAX_Q, n_out outside
 *   1 .. 3, n_aux outside 0 .. KNP_MAX_AUX, a mode outside -1 .. 10 or with an axis >= dim, an invalid or empty program, one that
 *   reads an aux slot >= n_aux or writes an output >= n_out, more than KNP_DIAG_MAX_CONSTS constants or another count in
 *   set_constants, an unknown id, a facet out of range or listed twice, a seg_ptr that does not start at 0 or decreases, in eval a
 *   null pointer of a slot the code reads; KNP_E_MESH (checked on the host at create, for the slots the code reads) when a mode of
 *   the extracellular cell (3 .. 5, 7) is bound and a listed facet's extracellular cell does not hold it, or when a geometric mode
 *   (>= 0) is bound and a cell it reads is flat (zero determinant, or gradients that are not finite; mode 7 and the normal read the
 *   intracellular cell).  n_tags == 0 is a successful no-op. */
int knp_membrane_functional_create(knp_ctx* ctx, int32_t n_tags, const int32_t* seg_ptr /* host [n_tags+1] */,
                                   const int32_t* facets /* host [seg_ptr[n_tags]] */, int32_t n_q, const double* q_pts /* host [n_q*dim] */,
                                   const double* q_w /* host [n_q] */, int32_t n_instr, const int32_t* code /* host [n_instr*4] */,
                                   int32_t n_consts, const double* consts /* host */, int32_t n_aux, const int32_t* aux_mode /* host [n_aux] */,
                                   int32_t n_out /* 1..3 */, int32_t* id /* host */);
int knp_membrane_functional_set_constants(knp_ctx* ctx, int32_t id, int32_t n_consts, const double* consts /* host */);
int knp_membrane_functional_eval(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out /* device [n_tags*n_out] */);
int knp_membrane_functional_destroy(knp_ctx* ctx, int32_t id);
/* Derived fields: the value of a functional's program on every listed cell or facet, and its average onto the vertices.
 * knp_functional_eval_items / knp_membrane_functional_eval_items: for a plan of knp_functional_create /
 *   knp_membrane_functional_create, out[i*n_out + j] = sum_q q_w[q] OUT_j(program at point q of item i), i the item's place in the
 *   list given at create (cells / facets, whatever order the tags put them in).  That is the item's mean: q_w sums to 1 and the measure
 *   is not applied.  The kernel is the functional's own with another end: the same loads, geometry, derivative slots and order of
 *   the sums, one store per item instead of the per-tag reduction, so |T_i| out[i] summed per tag is the functional's value up to the
 *   order of that sum.  One item per lane, 128 per block, the interpreter's register file in LDS (1 KiB per register the program
 *   uses, at most 48 KiB).  Enqueued on the library's stream; never waits for the device; the constants of the plan travel as kernel
 *   arguments.  Only the pointers of slots the code reads are used.  A plan without items is a successful no-op.  KNP_E_ARG with
 *   nothing launched: an unknown id, null fields or out, a null pointer of a slot the code reads.
 * Projections: a plan that belongs to the context like a functional (ids of their own; a destroyed id is reused; knp_destroy frees
 * the plans that are left).
 * knp_project_create: from the vertices of n_items items (nv each: dim+1 of a cell, dim of a facet) and their measures it builds the
 *   inverted index on the host -- per vertex the items that hold it, ascending -- and 1 / (sum of the list's measures), 0 for an
 *   empty list.  Synchronous; 12 bytes per entry and 20 per vertex of device memory.  KNP_E_ARG and no plan: a null argument, nv
 *   outside 2 .. 4, a vertex outside 0 .. n_vertices-1, a measure that is not finite and positive, an item that lists a vertex twice.
 * knp_project_apply: out[j*n_vertices + v] = (sum over the items i of v's list, ascending, of measure_i values[i*n_out + j]) /
 *   (sum of their measures); `fill` where the list is empty.  No atomics: one list per group of L lanes, lane l adds the entries
 *   l, l + L, .. in order and a fixed shuffle tree adds the lanes; L is the smallest power of two in 2 .. 32 that is not below the mean
 *   length of the non-empty lists.  A list of more than KNP_PI_SPLIT's value of entries (512) is cut into chunks of that many, each
 *   summed by a group of its own, and a second kernel adds a list's chunks in order: the same bits on every run.  Enqueued on the
 *   library's stream; never waits for the device.  KNP_E_ARG with nothing launched: an unknown id, n_out outside 1 .. 3, null values
 *   or out.
 * knp_project_get_info: what an application of the plan runs (plan fields only, nothing is launched): the first min(n, KNP_PI_COUNT)
 *   slots are written.  KNP_E_ARG for a null argument, n <= 0 or an unknown id.
 * knp_project_destroy: frees the plan (waits for the stream first). */
int knp_functional_eval_items(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out /* device [n_items*n_out] */);
int knp_membrane_functional_eval_items(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out /* device [n_items*n_out] */);
enum { KNP_PI_LANES = 0 /* lanes per list, L */, KNP_PI_LONGEST = 1 /* entries of the longest list */,
       KNP_PI_N_SPLIT = 2 /* lists cut into chunks */, KNP_PI_N_UNITS = 3 /* groups of L lanes launched */,
       KNP_PI_SPLIT = 4 /* the most entries a list may have without being cut; also the chunk length */, KNP_PI_COUNT = 5 };
int knp_project_create(knp_ctx* ctx, int32_t n_items, int32_t nv, const int32_t* item_vertices /* host [n_items*nv] */,
                       const double* measure /* host [n_items] */, int32_t* id /* host */);
int knp_project_apply(knp_ctx* ctx, int32_t id, const double* values /* device [n_items*n_out] */, int32_t n_out /* 1..3 */, double fill,
                      double* out /* device [n_out*n_vertices] */);
int knp_project_get_info(const knp_ctx* ctx, int32_t id, int32_t* out /* host [n] */, int n);
int knp_project_destroy(knp_ctx* ctx, int32_t id);
/* Linear forms: int f v dx(tag) and int g v dS(tag) against the P1 test functions, one number per vertex, for any program of a
 * functional; and their addition to the right-hand side of a step.
 * knp_functional_eval_load / knp_membrane_functional_eval_load: for a plan of knp_functional_create /
 *   knp_membrane_functional_create, with nv = dim+1 vertices of a cell or dim of a facet,
 *     out[(i*nv + a)*n_out + j] = sum_q (measure_i q_w[q] lambda_a(q)) OUT_j(program at point q of item i),
 *   q ascending: the item's element vector, i the item's place in the list given at create, a the local vertex in the order of the
 *   mesh's cell (the facet's vertices of the Gamma list), lambda_a(q) the a-th barycentric coordinate of point q.  Item-major, so
 *   that knp_scatter_apply finds the n_out numbers of an entry side by side.  The kernel is the functional's own with a third end:
 *   the same loads, geometry, derivative slots and normal modes, the interpreter's register file in LDS; the tag keys are not read
 *   and the segmented scan's LDS is not needed.  Enqueued on the library's stream; never waits for the device; the constants of the
 *   plan travel as kernel arguments.  A plan without items is a successful no-op.  KNP_E_ARG with nothing launched: an unknown id,
 *   null fields or out, a null pointer of a slot the code reads.
 * Scatter plans: sum-only gathers that belong to the context like projections (ids of their own; a destroyed id is reused;
 * knp_destroy frees the plans that are left).
 * knp_scatter_create: from the vertices of n_items items (nv each) it builds the inverted index on the host: per vertex the entries
 *   (i, a) with item_vertices[i*nv + a] == v, ascending in i.  Synchronous; 4 bytes per entry and 12 per vertex of device memory.
 *   KNP_E_ARG and no plan: a null argument, nv outside 2 .. 4, a vertex outside 0 .. n_vertices-1, an item that lists a vertex twice.
 * knp_scatter_apply: out[j*n_vertices + v] = sum over v's entries, in that order, of values[(i*nv + a)*n_out + j]; 0 where the list
 *   is empty.  The kernels, the lane rule and the split rule are knp_project_apply's with weight 1 and no division: no atomics, the
 *   same bits on every run.  Enqueued on the library's stream; never waits for the device.  KNP_E_ARG with nothing launched: an
 *   unknown id, n_out outside 1 .. 3, null values or out.
 * knp_scatter_get_info: the slots of knp_project_get_info (KNP_PI_*), for a scatter plan.
 * knp_scatter_destroy: frees the plan (waits for the stream first).
 * knp_rhs_add_load: b[4*node + field] += scale * load[vertex of node] on the owned nodes of `side`; every other entry of b is left
 *   alone.  One lane per owned node, on the library's stream behind knp_assemble_rhs; never waits for the device.  KNP_E_ARG with
 *   nothing launched: a field outside 0 .. 3, a side outside 0 .. 1, a null pointer.  One GPU only: KNP_E_STATE on a context with
 *   ghost nodes. */
int knp_functional_eval_load(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out /* device [n_items*nv*n_out] */);
int knp_membrane_functional_eval_load(knp_ctx* ctx, int32_t id, const knp_fields* fields, double* out /* device [n_items*nv*n_out] */);
int knp_scatter_create(knp_ctx* ctx, int32_t n_items, int32_t nv, const int32_t* item_vertices /* host [n_items*nv] */, int32_t* id /* host */);
int knp_scatter_apply(knp_ctx* ctx, int32_t id, const double* values /* device [n_items*nv*n_out] */, int32_t n_out /* 1..3 */,
                      double* out /* device [n_out*n_vertices] */);
int knp_scatter_get_info(const knp_ctx* ctx, int32_t id, int32_t* out /* host [n] */, int n);
int knp_scatter_destroy(knp_ctx* ctx, int32_t id);
int knp_rhs_add_load(knp_ctx* ctx, int32_t field /* 0..2 ion, 3 potential */, int32_t side /* 0 intra, 1 extra */, double scale,
                     const double* load /* device [n_vertices] */, double* b /* device [n_dof_local] */);

/* ---- the EMI model: two potentials with constant conductivities, ONE unknown per node (reference src/CGx/EMI) ----
 * Unknown n is node n of knp_get_layout; every vector is a device array of n_nodes_owned doubles.  One GPU only: every call
 * returns KNP_E_STATE on a context with ghost nodes, and -- knp_emi_setup apart -- before knp_emi_setup; KNP_E_ARG for a null argument.
 *   A = [ dt sigma_i K_i + C_M M_Gamma     -C_M M_Gamma              ]   (EMIx_problem.py:152-157)
 *       [ -C_M M_Gamma                     dt sigma_e K_e + C_M M_Gamma ]
 * symmetric positive semi-definite, constant in time.  Pure Neumann: A 1 = 0 over ALL nodes (knp_set_nullspace(ctx, 1) declares it).
 * knp_emi_setup: a kernel writes one value per same-side node pair and one per membrane vertex pair (the entry towards the other
 *   side's node) from the graph of knp_create, and the inverse diagonal.  Calling it again rewrites the values (another dt); an
 *   uploaded hierarchy is then stale.  After it, knp_amg_set_level takes n_nodes_owned rows on level 0 (and refuses n_dof_owned).
 * knp_emi_get_csr: A as CSR, rows / columns = nodes: row n = its same-side pairs in the order of the node graph (columns ascending),
 *   then, for a membrane vertex, the entries towards the other side.  KNP_SZ_EMI_NNZ entries.  Dirichlet nodes are NOT applied.
 * knp_emi_set_dirichlet: the listed nodes become identity rows AND columns of the operator knp_emi_spmv, knp_emi_pc_apply and
 *   knp_emi_cg_solve work with (symmetric elimination); n = 0 clears.  Host array, copied.
 * knp_emi_spmv: y = A x (with the Dirichlet elimination).
 * knp_emi_assemble_rhs: b_i = dt M_i f_i + s int_Gamma (C_M phi_m - dt I_ch) v dS, b_e = dt M_e f_e - s (the same), s = rhs_scale.
 *   phi_m = fields->phi_m and the gating variables fields->aux are nodal [n_vertices] and interpolated to the n_q points of the
 *   facet rule; I_ch is the sum of the outputs of the facet's membrane program (knp_set_program, bytecode interpreter; KNP_OP_KI /
 *   KNP_OP_KE read 0; no run-time compiled kernel is built on a context that assembles EMI right-hand sides).  fields->k_i / k_e are not read.  f_i, f_e: nodal [n_vertices], NULL = 0.  g: [n_nodes_owned] or NULL; with
 *   Dirichlet nodes b -= A g on the other rows and b = g on the Dirichlet ones.  With the null space on, b is projected at the end.
 *   Gathers per node, no atomics.
 * knp_emi_pc_setup / knp_emi_pc_apply: KNP_PC_NONE, KNP_PC_VBJACOBI (point Jacobi here) or KNP_PC_AMG: the generic level-by-level
 *   V-cycle on hierarchy 0, uploaded with knp_amg_reset / knp_amg_set_level / knp_amg_set_coarse after knp_emi_setup, level 0 = A
 *   (with the Dirichlet elimination).  pre == post sweeps keep it symmetric.  knp_emi_pc_apply projects z when the null space is on.
 * knp_emi_cg_solve: preconditioned conjugate gradients with PETSc's KSPCG semantics.  x on entry is the initial guess.  norm_type
 *   0 preconditioned ||B r||_2 (KSPCG's default), 1 unpreconditioned ||r||_2, 2 natural sqrt(r . B r).  Stops when the norm is
 *   <= max(rtol * (the same norm of b), atol); reason codes and the divergence test (1e5 times that reference) as knp_gmres_solve;
 *   p . A p <= 0, a non-finite value or a preconditioned norm lost to
 *   cancellation (null space on, B r constant to 8 digits) ends it with KNP_DIVERGED_NANORINF.  alpha and beta stay on the device, the reductions are
 *   two-stage in a fixed order (the same bits on every run), one pinned read-back per iteration.  With the null space on B's output
 *   is projected, so the component of x along the constant is that of the initial guess.  Dirichlet nodes: x = b there on return,
 *   exactly (set before the first residual).
 * knp_emi_update: phi_i / phi_e [n_vertices] = x at the vertex's intra / extra node, 0 where it has none; phi_m = phi_i - phi_e. */
int knp_emi_setup(knp_ctx* ctx, double dt, double C_M, double sigma_i, double sigma_e);
int knp_emi_get_csr(knp_ctx* ctx, int32_t* rowptr /* host [n_nodes_owned + 1] */, int32_t* colind, double* vals /* host [KNP_SZ_EMI_NNZ] */);
int knp_emi_set_dirichlet(knp_ctx* ctx, int32_t n, const int32_t* nodes /* host */);
int knp_emi_spmv(knp_ctx* ctx, const double* x, double* y);
int knp_emi_assemble_rhs(knp_ctx* ctx, const knp_fields* fields, const double* f_i, const double* f_e, const double* g,
                         double rhs_scale, double* b);
int knp_emi_pc_setup(knp_ctx* ctx, int32_t kind);
int knp_emi_pc_apply(knp_ctx* ctx, const double* r, double* z);
int knp_emi_cg_solve(knp_ctx* ctx, const double* b, double* x, double rtol, double atol, int32_t max_it, int32_t norm_type,
                     int32_t* its, double* rnorm, int32_t* reason);
int knp_emi_update(knp_ctx* ctx, const double* x, double* phi_i, double* phi_e, double* phi_m);

/* ---- instrumentation ---- */
/* elapsed ms and launch count of a kernel class since the last reset (HIP events on the ctx stream).
 * classes: 0 spmv, 1 orthogonalisation, 2 pc, 3 assembly, 4 other */
/* step timers of the host loop (reference: perf_counter + allreduce(MAX) around assembly and solve, KNPEMIx_solver.py:402-413,
 * 434-449): knp_timer_mark records one event on the stream (join_assembly != 0: after joining knp_assemble_matrix_async);
 * knp_timer_read synchronises once and returns the seconds between consecutive marks (n marks -> n - 1 intervals), then
 * forgets them; knp_timer_pending = marks recorded and not yet read. */
int knp_timer_mark(knp_ctx* ctx, int32_t join_assembly);
int knp_timer_read(knp_ctx* ctx, int32_t capacity, double* seconds /* host [capacity] */, int32_t* n_intervals);
int knp_timer_pending(const knp_ctx* ctx);
int knp_profile_enable(knp_ctx* ctx, int32_t class_mask); /* bit k enables class k; 0 disables */
int knp_profile_get(knp_ctx* ctx, int32_t cls, double* ms, int64_t* launches);
int knp_profile_reset(knp_ctx* ctx);
/* counters of the linear solves since the last knp_profile_reset: what PETSc's -log_view reports for the KSPSolve stage
 * (VecMDot/VecNorm reductions, VecScatter halos) behind KNPEMIx_solver.py:435 */
enum { KNP_ST_BNORM = 0 /* ||B b|| of the last solve */, KNP_ST_ALLREDUCE = 1 /* reductions over ranks */,
       KNP_ST_HALO = 2 /* fine-level halo exchanges */, KNP_ST_READBACK = 3 /* host waits on a reduced value */,
       KNP_ST_FUSED = 4 /* bit h set: hierarchy h runs the fused V(1,1) cycle; bit 2+h: its level 0 runs fused inside the
                           level-by-level cycle (distributed hierarchies) */,
       KNP_ST_NORM_FALLBACK = 5 /* GMRES iterations whose norm needed a second reduction (cancellation guard) */,
       KNP_ST_BLOCKED = 6 /* bit h set: the fused cycle of hierarchy h runs on node-blocked operators */,
       KNP_ST_FUSED_LEVELS = 7 /* levels >= 1 that run in fused form inside the level-by-level cycle, all hierarchies */,
       KNP_ST_FUSED_DOTS = 8 /* reductions whose first stage ran in the preconditioner's last leg (KNP_FUSED_DOTS) */,
       KNP_ST_SPMV_DOTS = 9 /* reductions whose first stage ran in the SpMV on A (knp_fgmres_solve, KNP_SPMV_DOTS) */,
       KNP_ST_FUSED_TAILS = 10 /* solves whose last update also unpacked x (knp_set_unpack_target, KNP_FUSED_TAIL) */,
       KNP_ST_KNOD_SKIPS = 11 /* matrix assemblies that skipped the node-indexed concentration copy (knp_fields_unchanged) */,
       KNP_ST_AHEAD_ADOPTED = 12 /* matrix assemblies taken from the one enqueued at the end of the last solve (KNP_ASM_AHEAD) */,
       KNP_ST_AHEAD_DISCARDED = 13 /* such assemblies that ran for nothing */,
       KNP_ST_COUNT = 14 };
int knp_get_stats(const knp_ctx* ctx, double* out /* host [KNP_ST_COUNT] */);
/* bytes the kernels of one application must move, from the sizes of the arrays they read and write (per-class roofline): [0] SpMV on A,
 * [1] one preconditioner application, [2] matrix assembly of one step, [3] right-hand side assembly, [4] one owned vector */
int knp_get_traffic_model(const knp_ctx* ctx, double* out /* host [5] */);
/* which kernels the context launches, from the choices made at creation (context fields only; nothing is launched): the first
 * min(n, KNP_LI_COUNT) slots are written.  KNP_E_ARG for a null argument or n <= 0.  The knp_emi_* kernels run 8 lanes per node whatever
 * the groups say; of these fields the graph sizes (MAX_NODE_CELLS, MAX_NODE_PAIRS) are what bears on them. */
enum { KNP_LI_ASM_VARIANT = 0 /* volume assembly: 0 plain gather, 1 staged with pair-major lists, 2 staged with transposed lists */,
       KNP_LI_ASM_STAGE = 1 /* LDS slots for cell means per node (0: not staged) */,
       KNP_LI_ASM_DMAX = 2 /* > 0: cell means fused into the assembly, LDS slots for this many neighbours per node */,
       KNP_LI_ASM_GROUP = 3, KNP_LI_SPMV_GROUP = 4, KNP_LI_PC_GROUP = 5 /* lanes per node: assembly, SpMV, level-0 preconditioner */,
       KNP_LI_MAX_NODE_CELLS = 6 /* most same-side cells around an owned node */,
       KNP_LI_MAX_NODE_PAIRS = 7 /* most node pairs of an owned node (its row of the node graph, self pair included) */,
       KNP_LI_SPMV_UNROLL = 8 /* pairs in flight per lane of the SpMV on A (KNP_SPMV_UNROLL, read once per process) */,
       KNP_LI_SPMV_MK = 9 /* 1: the SpMV on A reads {M, K} per pair, 0: the stored time-invariant entries (Dirichlet rows, KNP_SPMV_MF=0) */,
       KNP_LI_COUNT = 10 };
int knp_get_launch_info(const knp_ctx* ctx, int32_t* out /* host [n] */, int n);
/* what one level of an uploaded hierarchy runs on, and the cycle form knp_pc_setup chose for the hierarchy (context fields only;
 * nothing is launched): the first min(n, KNP_AI_COUNT) slots are written.  Lanes per row of the generic CSR kernels for the operators
 * the level carries, lanes per node row of their node-blocked copies (0: no such copy).  KNP_E_ARG for a null argument, n <= 0, or a
 * hierarchy / level that does not exist.  cgx_hip/backend.py (Backend.AMG_LEVEL_INFO) names the slots in this order: a slot added here is
 * added there (tests/test_synthetic_hierarchies_host.py compares the two). */
enum { KNP_AI_A_LANES = 0, KNP_AI_P_LANES = 1, KNP_AI_R_LANES = 2, KNP_AI_S_LANES = 3, KNP_AI_RT_LANES = 4, KNP_AI_U_LANES = 5,
       KNP_AI_BA_LANES = 6, KNP_AI_BR_LANES = 7, KNP_AI_BS_LANES = 8, KNP_AI_BRT_LANES = 9, KNP_AI_BU_LANES = 10,
       KNP_AI_P_N_ACT = 11, KNP_AI_S_N_ACT = 12 /* > 0: the kernel walks a compact list of this many non-empty rows */,
       KNP_AI_LFUSED = 13 /* the level runs in fused form inside the level-by-level cycle */,
       KNP_AI_N = 14, KNP_AI_N_COARSE = 15, KNP_AI_FP32 = 16 /* operator values are stored in fp32 */,
       KNP_AI_H_FUSED = 17, KNP_AI_H_BLOCKED = 18, KNP_AI_H_CFUSED = 19, KNP_AI_H_L0_FUSED = 20 /* of the hierarchy, as of the last knp_pc_setup */,
       KNP_AI_H_NC = 21 /* size of the dense coarse inverse (0: the last level smooths) */,
       KNP_AI_H_CINV_F32 = 22 /* the dense coarse inverse is applied from an fp32 copy */,
       KNP_AI_COUNT = 23 };
int knp_amg_get_level_info(const knp_ctx* ctx, int32_t hier, int32_t level, int32_t* out /* host [n] */, int n);

/* ---- mesh refinement (csrc/knp_refine.inc; cgx_hip/refine.py) ----------------------------------------------------------------
 * Uniform red refinement of P1 triangles / tetrahedra and the transfer of nodal fields to the refined mesh.  The mesh is refined
 * before a context exists: these entry points take no knp_ctx.  Every pointer is DEVICE memory, every launch goes to `stream`
 * (a hipStream_t; NULL = the default stream), nothing is read back and nothing is synchronised.  KNP_E_ARG for a null pointer, a
 * dimension other than 2 / 3 or a count outside [0, 2^31 - 1] (a fine count included; n_vertices >= 1: the keys then stay below 2^62);
 * KNP_E_HIP when a launch fails.
 *
 * Numbering.  Coarse vertices keep 0 .. nv-1.  The unique edge (a, b), a < b, has the 64-bit key a*nv + b and gets the vertex
 * nv + (rank of its key among the sorted unique keys) at (x[a] + x[b]) * 0.5 per component.  The caller sorts and deduplicates the
 * keys between knp_refine_edge_keys and the other calls; the kernels find an edge by binary search in that array.
 * Local edges of a cell in key order: 2D 01 02 12; 3D 01 02 03 12 13 23.  Below, 0..dim are the cell's vertices and m.. the midpoints.
 *
 * Children.  Cell c becomes the cells 2^dim c .. 2^dim c + 2^dim - 1, each with the orientation of c (fixed tables, no determinant):
 *   2D  (0 m01 m02) (m01 1 m12) (m02 m12 2) (m01 m12 m02)
 *   3D  (0 m01 m02 m03) (m01 1 m12 m13) (m02 m12 2 m23) (m03 m13 m23 3), then four around the diagonal k of the inner octahedron:
 *       k = 0, m01-m23: (m01 m23 m02 m03) (m01 m23 m03 m13) (m01 m23 m13 m12) (m01 m23 m12 m02)
 *       k = 1, m02-m13: (m02 m13 m03 m01) (m02 m13 m23 m03) (m02 m13 m12 m23) (m02 m13 m01 m12)
 *       k = 2, m03-m12: (m03 m12 m01 m02) (m03 m12 m02 m23) (m03 m12 m23 m13) (m03 m12 m13 m01)
 * Diagonal rule.  For k = 0, 1, 2 with (p q r t) = (0 1 2 3), (0 2 1 3), (0 3 1 2): d = ((x_p + x_q) - x_r) - x_t per component,
 * s_k = (d0*d0 + d1*d1) + d2*d2, every operation rounded on its own (no fused multiply-add).  k replaces the best so far only if
 * s_k < (1 - 2^-30) * s_best: near-ties go to the earliest candidate.
 * Tagged facets.  (a b) -> (a mab) (mab b); (a b c) -> (a mab mac) (mab b mbc) (mac mbc c) (mab mbc mac), children 2^(dim-1) f + j. */

/* keys [n_items * n_edges] of the items' edges, n_edges = 1, 3, 6 for nodes_per_item = 2, 3, 4 (facets of 2D / cells of 2D or facets
 * of 3D / cells of 3D).  An item with a vertex outside [0, nv) or with a vertex twice gets the keys 0 and sets *flag to 1 (flag is
 * never cleared here). */
int knp_refine_edge_keys(int32_t nodes_per_item, int64_t n_items, int64_t n_vertices, const int32_t* items, int64_t* keys, int32_t* flag,
                         void* stream);
/* fine_coords [(nv + n_edges) * dim]: the coarse coordinates, then the midpoints; edge_vertices [n_edges * 2] = (a, b) of every key */
int knp_refine_vertices(int32_t dim, int64_t n_vertices, int64_t n_edges, const int64_t* unique_keys, const double* coords,
                        double* fine_coords, int32_t* edge_vertices, void* stream);
/* fine_cells [n_cells * 2^dim * (dim+1)], fine_tags [n_cells * 2^dim] (the parent's tag), diagonal [n_cells] (dim 3; may be NULL in
 * 2D).  Cells must have passed knp_refine_edge_keys; a cell with a vertex out of range writes nothing. */
int knp_refine_cells(int32_t dim, int64_t n_cells, int64_t n_vertices, int64_t n_edges, const int64_t* unique_keys, const int32_t* cells,
                     const int32_t* cell_tags, const double* coords, int32_t* fine_cells, int32_t* fine_tags, uint8_t* diagonal, void* stream);
/* fine_facets [n_facets * 2^(dim-1) * dim], fine_values [n_facets * 2^(dim-1)].  A facet with a vertex out of range, a vertex twice
 * or an edge whose key is not among unique_keys adds 1 to *n_missing and writes nothing. */
int knp_refine_facets(int32_t dim, int64_t n_facets, int64_t n_vertices, int64_t n_edges, const int64_t* unique_keys, const int32_t* facets,
                      const int32_t* values, int32_t* fine_facets, int32_t* fine_values, int32_t* n_missing, void* stream);
/* n_fields nodal arrays at once, field f at in + f*ld_in (nv values) and out + f*ld_out (nv + n_edges values):
 * out[:nv] = in, out[nv + e] = 0.5 * (in[a_e] + in[b_e]).  in and out must not overlap. */
int knp_refine_prolong(int32_t n_fields, int64_t n_vertices, int64_t n_edges, const int32_t* edge_vertices, const double* in, int64_t ld_in,
                       double* out, int64_t ld_out, void* stream);

/* ---- level-set surfaces (csrc/knp_surface.inc; cgx_hip/surfaces.py) -----------------------------------------------------------
 * The cut of a set of simplices by the level s = iso of a nodal function: the clipped boundary of a set of cells, the slice / iso-
 * surface through them, contour lines on membrane facets.  Context-free like the refinement: every pointer is DEVICE memory (the
 * origin / normal of knp_surface_plane and the pointer tables of knp_surface_gather apart: host), every launch goes to `stream`,
 * nothing is read back and nothing is synchronised.  KNP_E_ARG, with nothing launched, for a null pointer, a bad nodes_per_item /
 * dim or a count outside [0, 2^31 - 1] (n_vertices >= 1); KNP_E_HIP when a launch fails.  A zero count is a successful no-op.
 *
 * Definitions.
 *   An ITEM is a simplex of npi = 3 or 4 local vertex ids with a side byte (0 intracellular, 1 extracellular) and a reference id (its
 *   tag): a triangle is a cell of a 2D mesh (dim 2) or a membrane facet of a 3D mesh (dim 3), a tetrahedron a cell of a 3D mesh.
 *   A BOUNDARY FACET has npi - 1 vertex ids, stored in an order whose normal points out of its item (3D: (v1 - v0) x (v2 - v0); 2D:
 *   the item lies to the left of v0 -> v1), and the index of that item, whose side and tag it takes.
 *   t_v = s_v - iso, one fp64 subtraction.  Vertex v is INSIDE iff t_v >= 0: a vertex exactly on the level is inside.  An item or
 *   boundary facet with a NaN t or a vertex id outside [0, nv) emits nothing; so does a boundary facet whose item index is out of range.
 *   An OUTPUT VERTEX has the key (side, a, b): a == b and w = 0 for an original vertex; for the cut point of the edge a-b, a is the
 *   inside and b the outside vertex and w = t_a / (t_a - t_b) (t_a >= 0 > t_b: no cancellation).  As a 64-bit integer the key is
 *   side * 2^62 + a * nv + b; the unique keys in ascending order number the output vertices.  The position and every field is
 *   (1 - w) F[a] + w F[b], every operation rounded on its own, F the side's array: an original vertex returns F[a] exactly.
 *   CUT FACES of a tetrahedron, p < q < u the inside local indices, r < t < u' the outside ones, xy the cut point of the edge x-y:
 *       1 inside / 3 outside   triangle (pr, pt, pu')          sequence (p, r, t, u')   reversed iff sign < 0
 *       3 inside / 1 outside   triangle (pr, qr, ur)           sequence (r, p, q, u)    reversed iff sign > 0
 *       2 inside / 2 outside   quad (pr, pt, qt, qr), split    sequence (p, q, r, t)    reversed iff sign < 0
 *                              as (0, 1, 2), (0, 2, 3)
 *   sign = sign(D) * parity(sequence), D = det[x1 - x0, x2 - x0, x3 - x0] of the item in its stored order (every operation rounded on
 *   its own, first row expanded: (e00 c0 + e01 c1) + e02 c2), parity the sign of the sequence as a permutation of the local indices:
 *   the sign of det[r-p, t-p, u'-p], det[p-r, q-r, u-r], det[q-p, r-p, t-p].  A reversed triangle swaps its last two vertices.  The
 *   normal of a cut face then points from the inside vertices to the outside ones, out of the kept solid; the decision never looks at
 *   the emitted triangle, so degenerate output is oriented like its neighbours.
 *   A triangle item gives a SEGMENT by the same rule one dimension down: 1 inside (p; r < t) -> (pr, pt), sequence (p, r, t), reversed
 *   iff sign < 0; 2 inside (p < q; r) -> (pr, qr), sequence (r, p, q), reversed iff sign > 0; a reversed segment swaps its ends.  In
 *   2D D = det[x1 - x0, x2 - x0]; for a facet of a 3D mesh D = +1: the stored order is the orientation.  Direction convention: seen
 *   from the side the item's normal (x1 - x0) x (x2 - x0) points to (2D: from +z) the kept part lies to the LEFT of the segment.
 *   A boundary facet is CLIPPED to the inside, keeping its cyclic order: 3 inside the facet itself; 1 inside (a; b, c next in cyclic
 *   order) (a, ab, ac); 2 inside (a, b before the outside c in cyclic order) (a, b, bc) and (a, bc, ac); 0 nothing.  An edge (2D):
 *   both inside itself, v0 only (v0, v0v1), v1 only (v1v0, v1).
 *   ORDER: the cut elements of item 0, 1, .. (local order as above), then the clipped elements of boundary facet 0, 1, ..: the scan
 *   of the counts fixes it, the same input gives the same arrays bit for bit.  Zero-area elements (a vertex exactly on the level)
 *   are kept.  Every element carries its item, that item's reference id and a kind (0 cut, 1 boundary).
 *
 * Sequence of a build: [knp_surface_plane] -> knp_surface_count -> the caller's exclusive scan of counts (int64 offsets) and one
 * read-back of the total -> knp_surface_emit -> the caller's sort + deduplication of element_keys -> knp_surface_vertices,
 * knp_surface_remap.  Per record: knp_surface_gather.  Kernels launch at most 1024 blocks of 256 lanes and stride over longer lists. */
#define KNP_SURFACE_MAX_FIELDS 16
/* s[v] = ((x0 - o0) n0 + (x1 - o1) n1) + (x2 - o2) n2, every operation rounded on its own; origin, normal: HOST [dim] */
int knp_surface_plane(int32_t dim, int64_t n_vertices, const double* coords, const double* origin, const double* normal, double* s,
                      void* stream);
/* counts [n_items + n_bfacets]: elements each item, then each boundary facet, emits */
int knp_surface_count(int32_t nodes_per_item, int64_t n_items, int64_t n_vertices, const int32_t* items, int64_t n_bfacets,
                      const int32_t* bfacets, const int32_t* bfacet_item, const double* s, double iso, int32_t* counts, void* stream);
/* offsets [n_items + n_bfacets]: the exclusive scan of counts; element_keys [n_elements * (npi - 1)], element_item / element_tag /
 * element_kind [n_elements].  (dim, npi) is (2, 3), (3, 3) or (3, 4); coords may be NULL for (3, 3).  An item whose elements would
 * not fit into n_elements writes nothing. */
int knp_surface_emit(int32_t dim, int32_t nodes_per_item, int64_t n_items, int64_t n_vertices, const int32_t* items, const uint8_t* item_side,
                     const int32_t* item_ref, int64_t n_bfacets, const int32_t* bfacets, const int32_t* bfacet_item, const double* s, double iso,
                     const double* coords, const int64_t* offsets, int64_t n_elements, int64_t* element_keys, int32_t* element_item,
                     int32_t* element_tag, uint8_t* element_kind, void* stream);
/* unique_keys [n_out] sorted -> vertex_a, vertex_b, vertex_w, vertex_side [n_out] and xyz [n_out * dim] */
int knp_surface_vertices(int32_t dim, int64_t n_vertices, int64_t n_out, const int64_t* unique_keys, const double* s, double iso,
                         const double* coords, int32_t* vertex_a, int32_t* vertex_b, double* vertex_w, uint8_t* vertex_side, double* xyz,
                         void* stream);
/* elements [n_keys] = position of element_keys[i] among unique_keys (binary search) */
int knp_surface_remap(int64_t n_keys, int64_t n_out, const int64_t* element_keys, const int64_t* unique_keys, int32_t* elements, void* stream);
/* out[f * n_out + k] = (1 - w_k) F_f[a_k] + w_k F_f[b_k], F_f = fields_i[f] where vertex_side[k] == 0, fields_e[f] where it is 1; NaN where
 * that pointer is NULL.  fields_i / fields_e: HOST tables of n_fields device pointers [n_vertices each]; one of the tables may be NULL.
 * n_fields in 0 .. KNP_SURFACE_MAX_FIELDS.  One launch (n_fields in the grid's y), no host copy, no synchronisation. */
int knp_surface_gather(int32_t n_fields, int64_t n_out, const int32_t* vertex_a, const int32_t* vertex_b, const double* vertex_w,
                       const uint8_t* vertex_side, const double* const* fields_i, const double* const* fields_e, double* out, void* stream);
/* measure [n_elements]: length of a segment (nodes_per_element 2) or area of a triangle (3, dim 3) from xyz [n_out * dim]; NaN for an
 * element with a vertex number outside [0, n_out) */
int knp_surface_measure(int32_t dim, int32_t nodes_per_element, int64_t n_elements, int64_t n_out, const int32_t* elements, const double* xyz,
                        double* measure, void* stream);
/* the launch geometry of the last knp_surface_* call of this process that launched a kernel (host state only; not thread-safe): the
 * first min(n, KNP_SI_COUNT) slots are written.  KNP_E_ARG for a null argument or n <= 0. */
enum { KNP_SK_PLANE = 1, KNP_SK_COUNT = 2, KNP_SK_EMIT = 3, KNP_SK_VERTICES = 4, KNP_SK_REMAP = 5, KNP_SK_GATHER = 6, KNP_SK_MEASURE = 7 };
enum { KNP_SI_KERNEL = 0 /* KNP_SK_* of the call, 0: none yet */, KNP_SI_BLOCKS = 1 /* grid x */, KNP_SI_THREADS = 2 /* lanes per block */,
       KNP_SI_N = 3 /* work items */, KNP_SI_TRIPS = 4 /* iterations of the grid-stride loop: > 1 when the list wrapped */,
       KNP_SI_GRID_Y = 5 /* grid y (fields of a gather) */, KNP_SI_COUNT = 6 };
int knp_surface_get_info(int32_t* out /* host [n] */, int n);

#ifdef __cplusplus
}
#endif
#endif /* KNPEMI_HIP_H */
