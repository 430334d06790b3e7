"""``SolverEMI``: the reference's EMI time loop (src/CGx/EMI/EMIx_solver.py) on the library's preconditioned conjugate gradients.

A step is one membrane right-hand side (knp_emi_assemble_rhs) and one PCG solve (knp_emi_cg_solve); the matrix is written once.
Deviations from the reference's class defaults (EMIx_solver.py:543-561), both forced by the problem being symmetric positive
semi-definite and by the library having no factorisation:
  * ``ksp_type = "cg"``; "gmres" and anything else raise NotImplementedError;
  * the direct solver is emulated by PCG at rtol 1e-12 (as the KNP-EMI solver emulates its direct solve).
``pc_type``: hypre | amg (the native aggregation hierarchy, built on the EMI matrix itself), jacobi, none.
"""
from __future__ import annotations

import os
import time
from types import SimpleNamespace

import numpy as np

from . import _lib, amg
from .emi_problem import ProblemEMI


def build_emi_hierarchy(A, pure_neumann, theta, coarse_size, smoother_degree, setup="host", device=None):
    """Aggregation hierarchy on the EMI matrix for the generic level-by-level cycle (A, P, R per level and the dense coarse inverse).
    ``pure_neumann``: A 1 = 0, so one coarse mode is the image of the constant; it is left out of the coarse inverse whatever
    eigenvalue the transfer operators gave it (``amg.dense_pseudo_inverse``)."""
    if setup == "gpu":
        from . import amg_gpu
        h = amg_gpu.build_hierarchy(A, theta=theta, coarse_size=coarse_size, device=device, smoother_degree=smoother_degree)
    else:
        h = amg.build_hierarchy(A, theta=theta, coarse_size=coarse_size, smoother_degree=smoother_degree)
    for lv in h.levels:
        lv.S = lv.Rt = lv.U = None
    if pure_neumann and h.coarse_inv is not None:
        h.coarse_inv = np.ascontiguousarray(amg.dense_pseudo_inverse(h.levels[-1].A, null_dim=1))
    return h


class SolverEMI:
    # ---- default iterative solver parameters (EMIx_solver.py:543-561)
    ksp_rtol = 1e-6
    ksp_max_it = 1000
    ksp_type = "cg"
    pc_type = "hypre"
    norm_type = "preconditioned"
    max_amg_iter = 1
    use_P_mat = True
    verbose = False
    use_block_Jacobi = True
    nonzero_init_guess = True
    save_interval = 1
    tot_its = 0
    tot_assembly_time = 0
    tot_solver_time = 0
    # the emulated direct solve
    direct_rtol = 1e-12
    # native AMG parameters: V(1,1), Chebyshev degree 1 (pre == post keeps the cycle symmetric)
    amg_theta = 0.08
    amg_coarse_size = 200
    amg_sweeps = 1
    amg_cheby_degree = 1
    amg_fp32 = False
    amg_setup = "host"     # "host" (SciPy, cgx_hip/amg.py) | "gpu" (torch sparse products, cgx_hip/amg_gpu.py)
    # True, or a mapping with threshold [V], repolarisation_threshold [V], tags (the output key save_activation of the KNP-EMI solver):
    # activation times, peaks and conduction velocity on the membrane, armed before the first step, one detector launch per step,
    # activation*.npy in the output directory after the last (cgx_hip/activation.py).  Off: nothing is allocated or launched.
    save_activation = False

    def __init__(self, problem: ProblemEMI, use_direct_solver: bool = True, save_xdmfs: bool = False, save_pngs: bool = False,
                 save_mat: bool = False):
        self.problem = problem
        self.comm = problem.comm
        self.time_steps = problem.time_steps
        self.direct_solver = use_direct_solver
        self.save_xdmfs = save_xdmfs
        self.save_pngs = save_pngs
        self.save_mat = save_mat
        self.out_file_prefix = problem.output_dir
        if self.ksp_type != "cg":
            raise NotImplementedError(f"ksp_type '{self.ksp_type}': the EMI matrix is symmetric, only 'cg' is implemented natively.")
        if self.pc_type not in ("hypre", "amg", "jacobi", "none"):
            raise NotImplementedError(f"pc_type '{self.pc_type}' has no native counterpart (hypre|amg|jacobi|none).")
        if self.norm_type not in ("preconditioned", "unpreconditioned", "natural"):
            raise NotImplementedError(f"norm_type '{self.norm_type}' (preconditioned|unpreconditioned|natural)")
        self.problem.setup_bilinear_form()
        self.problem.setup_linear_form()
        if self.use_block_Jacobi:
            self.problem.setup_preconditioner()
        self.backend = problem.backend
        self.iterations, self.reasons, self.solve_time, self.assembly_time = [], [], [], []
        self.out = None
        self.surfaces = []         # add_surface(): (name, LevelSetSurface, fields, interval)
        if save_xdmfs or save_pngs or save_mat:
            os.makedirs(self.out_file_prefix, exist_ok=True)
        if save_xdmfs:
            self.init_xdmf_savefile()
        if save_pngs:
            self.init_png_savefile()
        if self.save_mat:
            self.time_steps = 1
        self._solver_ready = False

    def print(self, *a, **k):
        self.problem.print(*a, **k)

    # ---- assembly
    def assemble_system(self):
        """The matrix is constant in time and already on the device (knp_emi_setup); the right-hand side is per step."""
        self.assemble_rhs()

    def assemble_rhs(self):
        p = self.problem
        for model in p.ionic_models:
            model.refresh(float(p.t.value))
        self.backend.refresh_program_constants()
        self.backend.assemble_rhs(p.rhs_scale)

    def create_and_set_nullspace(self):
        """Pure Neumann: the constant over all nodes of both sides (the library projects b and the preconditioner's output)."""
        on = not (self.problem.dirichlet_bcs and len(self.problem.bc_vertices))
        self.backend.set_nullspace(on)
        return on

    def build_hierarchy(self):
        """Aggregation hierarchy on the EMI matrix itself (level 0 = A with the Dirichlet elimination)."""
        p = self.problem
        A = getattr(p, "P", None)
        if A is None:
            A = p.setup_preconditioner()
        neumann = not (p.dirichlet_bcs and len(p.bc_vertices)) and not len(getattr(self.backend, "bc_nodes", ()))
        return build_emi_hierarchy(A, neumann, self.amg_theta, self.amg_coarse_size, self.amg_cheby_degree, self.amg_setup, self.backend.device)

    def setup_solver(self):
        be = self.backend
        self.create_and_set_nullspace()
        if self.pc_type in ("hypre", "amg"):
            tic = time.perf_counter()
            be.check(be.lib.knp_amg_set_precision(be.ctx, 1 if self.amg_fp32 else 0))
            self.hierarchy = self.build_hierarchy()
            amg.upload(be.lib, be.ctx, be.check, self.hierarchy, self.amg_sweeps, self.amg_sweeps, self.amg_cheby_degree, index=0)
            be.pc_setup(_lib.PC_AMG)
            self.print(f"AMG hierarchy: {self.hierarchy.describe()} ({time.perf_counter() - tic:0.3f} s)")
        else:
            be.pc_setup(_lib.PC_VBJACOBI if self.pc_type == "jacobi" else _lib.PC_NONE)
        if self.direct_solver:
            self.print("Using the emulated direct solver (PCG at rtol %.0e) ..." % self.direct_rtol)
        else:
            self.print("Setting up iterative solver ...")
        self._solver_ready = True

    def add_surface(self, name, S, fields=None, interval=None):
        """Record nodal fields on the built surface ``S`` (cgx_hip/surfaces.py; ``problem.clip_surface(...)``) at step 0 and at every
        ``interval``-th step (default ``save_interval``), one gather launch per record: ``fields`` None for ``phi`` (phi_i on
        intracellular elements, phi_e on extracellular ones) or a mapping name -> (function_i, function_e).  The run ends with
        surface_<name>.xdmf / .h5 in the output directory.  Call it before ``solve()``."""
        from .surfaces import check_add_surface
        if self._solver_ready:
            raise RuntimeError("add_surface() must be called before solve()")
        self.surfaces.append(check_add_surface(self, name, S, fields, interval, self.surfaces))

    # ---- time loop
    def solve(self):
        p = self.problem
        be = self.backend
        tic = time.perf_counter()
        self.setup_solver()
        setup_timer = time.perf_counter() - tic
        rtol = self.direct_rtol if self.direct_solver else self.ksp_rtol
        norm = "unpreconditioned" if self.direct_solver else self.norm_type
        dt = float(p.dt.value)
        from .activation import ActivationMap, parse_activation_key
        act = parse_activation_key({"save_activation": self.save_activation}, p.gamma_tags)
        self.activation = ActivationMap(p, **act) if act is not None else None
        recorders = []
        if self.surfaces:
            from .surfaces import SurfaceRecorder, named_functions
            recorders = [SurfaceRecorder(name, S, *named_functions(p, fields), interval, self.time_steps, self.out_file_prefix)
                         for name, S, fields, interval in self.surfaces]
            for r in recorders:
                r.record(0, float(p.t.value))
        be.timer_mark()
        try:
            for i in range(self.time_steps):
                p.t.value = float(p.t.value) + dt
                if p.MMS_test:
                    p.update_mms(float(p.t.value))
                self.assemble_rhs()
                be.timer_mark()
                if not self.nonzero_init_guess:
                    be.x.zero_()
                its, rn, reason = be.cg(rtol, max_it=self.ksp_max_it, norm_type=norm)
                be.update(p.wh[0], p.wh[1], p.phi_M)
                for model in p.ionic_models:
                    model.update()
                p.u_p[0].x.array.copy_(p.wh[0].x.array)
                p.u_p[1].x.array.copy_(p.wh[1].x.array)
                be.timer_mark()
                self.iterations.append(its)
                self.reasons.append(reason)
                self.rnorm = rn
                if reason < 0:
                    raise RuntimeError(f"EMI step {i + 1}: PCG ended with {_lib.REASONS.get(reason, reason)} after {its} iterations (residual {rn:.3e})")
                if self.verbose:
                    self.print(f"step {i + 1}: {its} iterations, residual {rn:.3e}")
                if self.save_xdmfs and (i + 1) % self.save_interval == 0:
                    self.save_xdmf()
                if self.save_pngs:
                    self.save_png()
                if self.activation is not None:
                    self.activation.update()
                for r in recorders:
                    r.record(i + 1, float(p.t.value))
        finally:
            for r in recorders:
                r.save()
            t = be.timer_read()
            self.assembly_time = list(t[0::2][:len(self.iterations)])
            self.solve_time = list(t[1::2][:len(self.iterations)])
            if self.save_xdmfs:
                self.close_xdmf()
        self.tot_its = int(sum(self.iterations))
        self.tot_assembly_time, self.tot_solver_time = float(sum(self.assembly_time)), float(sum(self.solve_time))
        if self.save_pngs:
            self.print_figures()
        if self.activation is not None:
            self.activation.save(self.out_file_prefix)
        if self.save_mat:
            import scipy.sparse as sp
            sp.save_npz(os.path.join(self.out_file_prefix, "Amat.npz"), be.csr())
        self.print("\nTotal setup time:", setup_timer)
        self.print("Total assembly time:", self.tot_assembly_time)
        self.print("Total solve time:", self.tot_solver_time)
        self.print_info()
        if p.MMS_test:
            p.print_errors()

    def potential_norms(self):
        """L2 norms of phi_i over the intracellular and phi_e over the extracellular cells (reference EMI/main.py:33-39)"""
        import ctypes as C
        be, p = self.backend, self.problem
        out = (C.c_double * 2)()
        be.check(be.lib.knp_l2_norms(be.ctx, C.c_void_p(p.wh[0].data_ptr()), C.c_void_p(p.wh[1].data_ptr()), out))
        return float(np.sqrt(out[0])), float(np.sqrt(out[1]))

    def print_info(self):
        p = self.problem
        self.print("\n#------------ PROBLEM -------------#\n")
        self.print("MPI Size = ", self.comm.size)
        self.print("Input mesh = ", p.input_files["mesh_file"])
        self.print("Global # mesh cells = ", p.mesh.num_cells)
        self.print("Global # dofs = ", self.backend.n_nodes)
        self.print("FEM order = ", p.fem_order)
        self.print("# Time steps = ", self.time_steps)
        self.print("dt = ", float(p.dt.value))
        self.print("Using Dirichlet BCs." if p.dirichlet_bcs else "Using Neumann BCs.")
        self.print("\n#------------ SOLVER -------------#\n")
        if self.direct_solver:
            self.print(f"Direct solver emulated by [cg+{self.pc_type}] at rtol {self.direct_rtol:.0e}.")
        else:
            self.print("Solver type: [" + self.ksp_type + "+" + self.pc_type + "]")
            self.print(f"Tolerance: {self.ksp_rtol:.2e}")
        if self.iterations:
            self.print("Average iterations: " + str(sum(self.iterations) / len(self.iterations)))

    # ---- output
    def init_xdmf_savefile(self):
        """subdomains.xdmf and solution.xdmf (phi_i, phi_e per saved step) through the package's XDMF / HDF5 writer"""
        from .output import RunOutput
        p = self.problem
        view = SimpleNamespace(local_mesh=p.local_mesh, comm=p.comm, num_variables=1, wh=[[p.u_p[0]], [p.u_p[1]]], t=p.t, print=p.print)
        self.out = RunOutput.__new__(RunOutput)
        self.out.p, self.out.prefix, self.out.xdmf = view, self.out_file_prefix, None
        self.out.init_xdmf_savefile()

    def save_xdmf(self):
        self.out.save_xdmf()

    def close_xdmf(self):
        if self.out is not None:
            self.out.close_xdmf()

    def init_png_savefile(self):
        p = self.problem
        fv = p._fv
        self.point_to_plot = int(fv[0, 0]) if len(fv) else 0
        self.v_t = [1000.0 * float(p.phi_M.x.array[self.point_to_plot])]
        self.gates_t = [[float(getattr(p, g).x.array[self.point_to_plot]) for g in "nmh"]] if hasattr(p, "n") else None

    def save_png(self):
        p = self.problem
        self.v_t.append(1000.0 * float(p.phi_M.x.array[self.point_to_plot]))
        if self.gates_t is not None:
            self.gates_t.append([float(getattr(p, g).x.array[self.point_to_plot]) for g in "nmh"])

    def print_figures(self):
        """v.png (membrane potential at one membrane vertex, mV) and gating.png; the traces are also kept as v.npy"""
        np.save(os.path.join(self.out_file_prefix, "v.npy"), np.array(self.v_t))
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError:
            self.print("matplotlib is not installed: traces saved as v.npy only")
            return
        tt = np.linspace(0, 1000 * self.time_steps * float(self.problem.dt.value), len(self.v_t))
        plt.figure()
        plt.plot(tt, self.v_t)
        plt.xlabel("Time (ms)")
        plt.ylabel("Membrane potential (mV)")
        plt.savefig(os.path.join(self.out_file_prefix, "v.png"))
        plt.close()
        if self.gates_t is not None:
            plt.figure()
            for k, nm in enumerate("nmh"):
                plt.plot(tt, [g[k] for g in self.gates_t], label=nm)
            plt.legend()
            plt.xlabel("Time (ms)")
            plt.savefig(os.path.join(self.out_file_prefix, "gating.png"))
            plt.close()
