"""``ProblemEMI``: the reference's EMI problem (src/CGx/EMI/EMIx_problem.py) on the MI355X-native library.

EMI is the cell-by-cell model that KNP-EMI extends: two potentials with constant conductivities, one unknown per node (vertex,
side).  The discrete problem (P1; K, M the per-side stiffness / mass matrices, M_G the mass matrix of the membrane facets):

    A = [ dt s_i K_i + C_M M_G      -C_M M_G          ]        (EMIx_problem.py:152-157)
        [ -C_M M_G                  dt s_e K_e + C_M M_G ]
    b_i = dt M_i f_i + s int_G (C_M phi_M - dt I_ch) v dS,    b_e = dt M_e f_e - s (the same)

with s = 1: the consistent backward-Euler form the reference's own tested script uses (EMI/tests/square_test.py:352-355).  The
reference's ``ProblemEMI`` multiplies the membrane integral by dt once more (EMIx_problem.py:215-217); the class attribute
``literal_reference_rhs = True`` selects that form (s = dt).  The matrix, the right-hand side, the preconditioner and the
conjugate-gradient solve are HIP kernels behind ``knp_emi_*`` (include/knpemi_hip.h, csrc/knp_emi.inc); ``EmiBackend`` is the
ctypes handle on them.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import yaml

from . import _lib, fem
from .backend import ActivationCalls, StateUpdate
from . import mesh as meshmod
from .emi_models import HH_model, IonicModel, Passive_model, g_syn_none
from .fem import Function, FunctionSpace
from .problem import MixedDimensionalProblem, range_constructor


def _f64(a):
    return a.ctypes.data_as(_lib.f64p)


def _i32(a):
    return a.ctypes.data_as(_lib.i32p)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class EmiBackend(StateUpdate, ActivationCalls):
    """Owns the ``knp_ctx`` of an EMI problem and the device vectors b, x [n_nodes]."""

    def __init__(self, problem, gamma_prog):
        self.p = problem
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.KnpError("No HIP device visible: the EMI assemble-and-solve path runs on the GPU only "
                                "(there is deliberately no CPU fallback).")
        self.device = torch.device("cuda", torch.cuda.current_device())
        lm = problem.local_mesh
        coords = np.ascontiguousarray(lm.coords, dtype=np.float64)
        cells = np.ascontiguousarray(lm.cells, dtype=np.int32)
        side = np.ascontiguousarray(problem.cell_side, dtype=np.uint8)
        gamma = np.ascontiguousarray(lm.gamma, dtype=np.int32)
        gprog = np.ascontiguousarray(gamma_prog, dtype=np.int32)
        qp = np.ascontiguousarray(problem.q_pts, dtype=np.float64)
        qw = np.ascontiguousarray(problem.q_w, dtype=np.float64)
        self._keep = [coords, cells, side, gamma, gprog, qp, qw]
        desc = _lib.MeshDesc()
        desc.dim = coords.shape[1]
        desc.n_vertices = desc.n_vertices_owned = coords.shape[0]
        desc.n_cells = desc.n_cells_owned = cells.shape[0]
        desc.cells, desc.coords = _i32(cells), _f64(coords)
        desc.cell_side = side.ctypes.data_as(_lib.u8p)
        desc.n_gamma = gamma.shape[0]
        desc.gamma = _i32(gamma) if gamma.size else None
        desc.gamma_prog = _i32(gprog) if gprog.size else None
        desc.n_q, desc.q_pts, desc.q_w = qw.shape[0], _f64(qp), _f64(qw)
        ctx = C.c_void_p()
        rc = self.lib.knp_create(C.byref(ctx), C.byref(desc))
        self.ctx = ctx
        if rc != 0:
            msg = self.lib.knp_last_error(ctx) if ctx else b"allocation failed"
            if ctx:
                self.lib.knp_destroy(ctx)
                self.ctx = None
            raise _lib.KnpError(f"knp_create failed ({rc}): {msg.decode()}")
        self.check(self.lib.knp_set_stream(self.ctx, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        sz = (C.c_int64 * _lib.KNP_SZ_COUNT)()
        self.check(self.lib.knp_get_sizes(self.ctx, sz))
        self.n_nodes = int(sz[_lib.SZ_N_NODES_OWNED])
        self.n_pairs = int(sz[_lib.SZ_N_PAIRS])
        self.n_gamma_pairs = int(sz[_lib.SZ_N_GAMMA_PAIRS])
        nv = coords.shape[0]
        self.node_i = np.empty(nv, dtype=np.int32)
        self.node_e = np.empty(nv, dtype=np.int32)
        self.check(self.lib.knp_get_layout(self.ctx, _i32(self.node_i), _i32(self.node_e)))
        self.b = torch.zeros(self.n_nodes, dtype=torch.float64, device=self.device)
        self.x = torch.zeros(self.n_nodes, dtype=torch.float64, device=self.device)
        self.g = None               # Dirichlet values [n_nodes] on the device
        self.f_i = self.f_e = None  # nodal volume sources (device tensors [n_vertices]) or None
        self._fields = None

    def check(self, rc):
        _lib.check(self.ctx, rc)

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self.lib.knp_destroy(self.ctx)
                self.ctx = None
        except Exception:      # noqa: BLE001
            pass

    # ---- set-up
    def setup(self, dt, C_M, sigma_i, sigma_e):
        self.check(self.lib.knp_emi_setup(self.ctx, float(dt), float(C_M), float(sigma_i), float(sigma_e)))

    def set_dirichlet(self, nodes, values=None):
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        self.check(self.lib.knp_emi_set_dirichlet(self.ctx, len(nodes), _i32(nodes) if len(nodes) else None))
        self.bc_nodes = torch.as_tensor(nodes.astype(np.int64), device=self.device)
        self.g = torch.zeros(self.n_nodes, dtype=torch.float64, device=self.device) if len(nodes) else None
        if values is not None and len(nodes):
            self.set_dirichlet_values(values)

    def set_dirichlet_values(self, values):
        self.g[self.bc_nodes] = torch.as_tensor(np.asarray(values, dtype=np.float64), device=self.device)

    def set_nullspace(self, on=True):
        self.check(self.lib.knp_set_nullspace(self.ctx, 1 if on else 0))

    def upload_programs(self, programs):
        self.programs = programs
        for pid, spec in enumerate(programs):
            code = np.ascontiguousarray(spec.code, dtype=np.int32)
            consts = spec.constants()
            self.check(self.lib.knp_set_program(self.ctx, pid, code.shape[0], _i32(code), consts.shape[0], _f64(consts) if consts.size else None))

    def refresh_program_constants(self):
        for pid, spec in enumerate(self.programs):
            consts = spec.constants()
            if consts.size:
                self.check(self.lib.knp_set_program_constants(self.ctx, pid, consts.shape[0], _f64(consts)))

    def fields(self):
        if self._fields is None:
            p = self.p
            f = _lib.Fields()
            f.phi_m = p.phi_M.data_ptr()
            aux = getattr(p, "aux_functions", None)      # n, m, h when they exist, then the declared states (compile_programs)
            if aux is None:
                aux = (p.n, p.m, p.h) if hasattr(p, "n") else ()
            for k, fn in enumerate(aux):
                f.aux[k] = fn.data_ptr()
            self._fields = f
        return self._fields

    # ---- per step
    def assemble_rhs(self, scale=1.0):
        f = self.fields()
        self.check(self.lib.knp_emi_assemble_rhs(self.ctx, C.byref(f), _ptr(self.f_i), _ptr(self.f_e), _ptr(self.g), float(scale), _ptr(self.b)))

    def pc_setup(self, kind):
        self.check(self.lib.knp_emi_pc_setup(self.ctx, int(kind)))

    def pc_apply(self, r, z):
        self.check(self.lib.knp_emi_pc_apply(self.ctx, _ptr(r), _ptr(z)))

    def spmv(self, x, y):
        self.check(self.lib.knp_emi_spmv(self.ctx, _ptr(x), _ptr(y)))

    NORMS = {"preconditioned": 0, "unpreconditioned": 1, "natural": 2}

    def cg(self, rtol, atol=1e-50, max_it=1000, norm_type="preconditioned"):
        its, rn, reason = C.c_int32(), C.c_double(), C.c_int32()
        self.check(self.lib.knp_emi_cg_solve(self.ctx, _ptr(self.b), _ptr(self.x), float(rtol), float(atol), int(max_it),
                                             self.NORMS[norm_type], C.byref(its), C.byref(rn), C.byref(reason)))
        return its.value, rn.value, reason.value

    def update(self, phi_i, phi_e, phi_m):
        self.check(self.lib.knp_emi_update(self.ctx, _ptr(self.x), C.c_void_p(phi_i.data_ptr()), C.c_void_p(phi_e.data_ptr()), C.c_void_p(phi_m.data_ptr())))

    def hh_update(self, phi_m, n, m, h, dt, phi_rest, rush_larsen, substeps):
        self.check(self.lib.knp_hh_update(self.ctx, C.c_void_p(phi_m.data_ptr()), C.c_void_p(n.data_ptr()), C.c_void_p(m.data_ptr()),
                                          C.c_void_p(h.data_ptr()), int(phi_m.x.array.numel()), dt, phi_rest, int(rush_larsen), int(substeps)))

    def timer_mark(self):
        self.check(self.lib.knp_timer_mark(self.ctx, 0))

    def timer_read(self):
        n = int(self.lib.knp_timer_pending(self.ctx))
        out = (C.c_double * max(n, 1))()
        k = C.c_int32()
        self.check(self.lib.knp_timer_read(self.ctx, max(n, 1), out, C.byref(k)))
        return np.array(out[:k.value], dtype=np.float64)

    def launch_info(self):
        """the fields of ``knp_get_launch_info`` that bear on the EMI kernels (8 lanes per node, fixed): the graph sizes"""
        out = (C.c_int32 * 10)()      # KNP_LI_COUNT
        self.check(self.lib.knp_get_launch_info(self.ctx, out, 10))
        return {"max_node_cells": int(out[6]), "max_node_pairs": int(out[7]), "emi_group": 8}

    # ---- export
    def csr(self, eliminated=False):
        """the EMI matrix as SciPy CSR (columns sorted); ``eliminated``: Dirichlet rows and columns replaced by the identity, the
        operator the solver works with and the hierarchy is built on"""
        import scipy.sparse as sp
        sz = (C.c_int64 * _lib.KNP_SZ_COUNT)()
        self.check(self.lib.knp_get_sizes(self.ctx, sz))
        nnz = int(sz[_lib.SZ_EMI_NNZ])
        rp = np.empty(self.n_nodes + 1, dtype=np.int32)
        ci = np.empty(nnz, dtype=np.int32)
        va = np.empty(nnz, dtype=np.float64)
        self.check(self.lib.knp_emi_get_csr(self.ctx, _i32(rp), _i32(ci), _f64(va)))
        A = sp.csr_matrix((va, ci, rp), shape=(self.n_nodes, self.n_nodes))
        A.sort_indices()
        bc = getattr(self, "bc_nodes", None)
        if eliminated and bc is not None and len(bc):
            keep = np.ones(self.n_nodes)
            keep[bc.cpu().numpy()] = 0.0
            D = sp.diags(keep)
            A = (D @ A @ D + sp.diags(1.0 - keep)).tocsr()
            A.eliminate_zeros()
            A.sort_indices()
        return A


class ProblemEMI(MixedDimensionalProblem):

    # ---- class defaults (EMIx_problem.py:311-332)
    C_M = 0.1
    sigma_i = 1
    sigma_e = 1
    source_i = 0.0
    source_e = 0.0
    phi_e_init = 0
    phi_M_init = -0.06774
    mesh_conversion_factor = 1
    fem_order = 1
    MMS_test = False
    dirichlet_bcs = False
    # False: s = 1, the consistent backward-Euler right-hand side (EMI/tests/square_test.py:352-355); True: s = dt, the reference's
    # literal EMIx_problem.py:215-217, whose membrane term carries a second factor dt
    literal_reference_rhs = False

    def read_config_file(self, config_file):
        yaml.add_constructor("!range", range_constructor, Loader=yaml.FullLoader)
        if isinstance(config_file, dict):
            config = dict(config_file)
        else:
            with open(config_file, "r") as file:
                config = dict(yaml.load(file, Loader=yaml.FullLoader))
        if self.comm.size > 1:
            raise NotImplementedError("the EMI model runs on one GPU (one rank) only")
        if str(config.get("problem_type", "EMI")) != "EMI":
            raise RuntimeError(f"ProblemEMI needs problem_type: EMI (got '{config.get('problem_type')}')")
        # the reference's EMI/config.yaml has no solver section (SolverEMI takes its options as constructor arguments)
        config.setdefault("solver", {})
        if "cell_tag_file" not in config and "mesh_file" in config:
            config["cell_tag_file"] = config["mesh_file"]
        config.setdefault("facet_tag_file", config.get("cell_tag_file"))
        super().read_config_file(config)
        for key in ("C_M", "sigma_i", "sigma_e"):
            if key in config:
                setattr(self, key, float(config[key]))
        if "literal_reference_rhs" in config:
            self.literal_reference_rhs = bool(config["literal_reference_rhs"])
        self.boundary_tag = self.boundary_tags[0] if len(self.boundary_tags) else None

    # ---- MixedDimensionalProblem hooks
    def init(self):
        if self.MMS_test:
            self.setup_MMS_params()

    def setup_constants(self):
        for key in ("C_M", "sigma_i", "sigma_e"):
            if not float(getattr(self, key)) > 0.0:
                raise ValueError(f"{key} must be positive")

    def setup_spaces(self):
        self.print("Setting up function spaces ...")
        self.V = FunctionSpace(self.mesh)
        self.W = [self.V.clone(), self.V.clone()]
        self.wh = [Function(self.W[0], "phi_i"), Function(self.W[1], "phi_e")]
        self.u_p = [Function(self.W[0], "phi_i"), Function(self.W[1], "phi_e")]
        self.phi_M = Function(self.V, "phi_M")      # set to phi_M_init by setup_bilinear_form

    def setup_boundary_conditions(self):
        """phi_e is prescribed on the exterior boundary when ``dirichlet_bcs`` (EMIx_problem.py:80-105); pure Neumann otherwise"""
        self.print("Setting up boundary conditions ...")
        self.bcs = []
        self.bc_vertices = np.zeros(0, dtype=np.int32)
        if self.dirichlet_bcs:
            fverts, _, _ = meshmod.exterior_facets(self.local_mesh.cells)
            v = np.unique(fverts).astype(np.int32)
            has_e = np.zeros(self.mesh.num_vertices, dtype=bool)
            has_e[np.unique(self.local_mesh.cells[self.cell_side == 1])] = True
            self.bc_vertices = v[has_e[v]]
            self.bc_values = self._phi_e_boundary(0.0)
            self.bcs = [("extra", 0, self.bc_vertices, self.bc_values)]

    def _phi_e_boundary(self, t):
        if self.MMS_test:
            return self.mms_exact(self.mesh.geometry.x[self.bc_vertices], t)[1]
        return np.full(len(self.bc_vertices), float(self.phi_e_init))

    def setup_source_terms(self):
        raise NotImplementedError("source_terms: ion_injection belongs to the KNP-EMI problem")

    # ---- membrane models (EMIx_problem.py:24-33)
    def add_ionic_model(self, model, tags=None, stim_fun=g_syn_none):
        model = model[0] if isinstance(model, (list, tuple)) else model
        name = model if isinstance(model, str) else str(model)
        if name in ("Hodgkin-Huxley", "HH"):
            new = HH_model(self, tags, stim_fun)
        elif name == "Passive":
            new = Passive_model(self, tags)
        else:
            raise RuntimeError(f'Model type {name} not supported. Choose either "HH" or "Passive".')
        self.ionic_models.append(new)
        return new

    def init_ionic_model(self, ionic_models=None):
        """Initialise the registered models (``add_ionic_model``); a model list given here is adopted when none was registered."""
        if not self.ionic_models and ionic_models is not None:
            self.ionic_models = list(ionic_models) if isinstance(ionic_models, (list, tuple)) else [ionic_models]
        tags = set()
        for model in self.ionic_models:
            if not isinstance(model, IonicModel):
                raise TypeError("ionic models must derive from cgx_hip.emi_models.IonicModel")
            if self.MMS_test:
                model.tags = tuple(self.gamma_tags)
            model._init()
            tags.update(model.tags)
        missing = sorted(set(self.gamma_tags) - tags)
        if self.ionic_models and missing:
            raise RuntimeError(f"Mismatch between membrane tags and ionic models tags: no model on membrane tags {missing}")
        self.state_variables, self.state_rush_larsen, self.state_substeps = fem.collect_states(self.ionic_models)
        self.print("# Membrane tags = ", len(self.gamma_tags))
        self.print("# Ionic models  = ", len(self.ionic_models), "\n")

    init_ionic_models = init_ionic_model

    def advance_states(self, model):
        """``IonicModel.update()`` of a model with declared states: one launch advances the states of all models, at the call of
        the first model that has any"""
        owners = [m for m in self.ionic_models if getattr(m, "states", None)]
        if owners and model is owners[0]:
            self.backend.state_update()

    # ---- forms
    def setup_bilinear_form(self):
        """Create the library context and write the matrix on the device (knp_emi_setup)."""
        self.print("Setting up bilinear form ...")
        if len(self.ionic_models) == 0:
            raise RuntimeError("\nNo ionic model(s) specified.\nCall init_ionic_model() to provide ionic models.\n")
        for model in self.ionic_models:
            if not hasattr(model, "g_stim") and isinstance(model, HH_model):
                model._init()
        init = self.phi_M_init
        self.phi_M.x.array[:] = torch.as_tensor(np.broadcast_to(np.asarray(init, dtype=np.float64), (self.mesh.num_vertices,)).copy(),
                                                device=self.mesh.device)
        model_of_tag = {}
        for k, model in enumerate(self.ionic_models):
            for tag in model.tags:
                model_of_tag.setdefault(int(tag), k)
        gamma_prog = np.array([model_of_tag[int(t)] for t in self.local_mesh.gamma_tags], dtype=np.int32)
        self.backend = be = EmiBackend(self, gamma_prog)
        be.setup(float(self.dt.value), self.C_M, self.sigma_i, self.sigma_e)
        if self.dirichlet_bcs and len(self.bc_vertices):
            be.set_dirichlet(be.node_e[self.bc_vertices], self.bc_values)
            be.set_nullspace(False)
        else:
            be.set_nullspace(True)
        self.a = "knp_emi_setup"

    def setup_linear_form(self):
        """Compile the channel currents of the models to membrane programs and hand them to the library."""
        self.print("Setting up linear form ...")
        assert self.backend is not None, "setup_bilinear_form() first"
        self.backend.upload_programs(self.compile_programs())
        if self.state_variables:
            self.backend.state_setup()
        self.L = "knp_emi_assemble_rhs"

    def compile_programs(self):
        """one bytecode program per model: KNP_OP_PHIM, KNP_OP_AUX (n, m, h in 0..2 when they exist, then the declared states),
        constants, KNP_OP_OUT 0; and one program per declared state"""
        states = getattr(self, "state_variables", [])
        aux = [self.n, self.m, self.h] if hasattr(self, "n") else []
        aux += [st.function for st in states if not any(st.function is f for f in aux)]
        n_known = len(aux)
        if n_known > _lib.KNP_MAX_AUX:
            raise ValueError(f"more than {_lib.KNP_MAX_AUX} auxiliary nodal fields in membrane expressions")
        roles = {id(self.phi_M): ("PHIM", 0)}
        self.programs = [fem.compile_program([model._eval()], roles, aux_functions=aux) for model in self.ionic_models]
        for st in states:
            fem.compile_state_program(st, roles, aux)
        if len(aux) > n_known:
            raise ValueError("EMI membrane models may only read phi_M, the gating variables n, m, h and the declared states")
        self.aux_functions = aux
        return self.programs

    def assemble_scalar(self, integrand_i=None, integrand_e=None, tags=None, degree=2):
        """``ProblemKNPEMI.assemble_scalar`` for the EMI model: every Function (phi_i, phi_e, phi_M, gates, states, the user's own)
        is an aux field of the functional.  Needs the library context, i.e. ``setup_bilinear_form()`` first."""
        from .functionals import assemble_scalar
        return assemble_scalar(self, integrand_i, integrand_e, tags, degree)

    def assemble_scalar_membrane(self, integrand, tags=None, degree=10):
        """``dfx.fem.assemble_scalar(dfx.fem.form(integrand * dS(tags)))``: the integral of ``integrand`` over the membrane tags
        (default every tag of ``gamma_tags``), summed over the tags, with a facet rule exact to ``degree``.  Besides what
        ``assemble_scalar`` takes (every Function is an aux field here) the integrand may hold restricted derivatives (``fem.grad(f)[a]('+')``: the intracellular cell,
        ``('-')``: the extracellular one), ``fem.FacetNormal`` and ``fem.NormalDerivative`` / ``fem.dot``.  A float for a single
        expression, else an array.  One launch pair (knp_membrane_functional_eval) and one read-back; keep a
        ``functionals.MembraneFunctional`` to integrate again or to have the rows per tag."""
        from .functionals import assemble_scalar_membrane
        return assemble_scalar_membrane(self, integrand, tags, degree)

    def cell_field(self, expr_i=None, expr_e=None, tags=None, degree=1, name="field"):
        """a ``fields.CellField``: the mean of ``expr_i`` / ``expr_e`` on every cell of the chosen tags, kept on the device (the
        expressions and ``tags`` of ``assemble_scalar``); ``F()`` evaluates it, ``F.to_nodes()`` averages it onto the vertices"""
        from .fields import CellField
        return CellField(self, expr_i, expr_e, tags, degree, name)

    def facet_field(self, expr, tags=None, degree=1, name="field"):
        """a ``fields.FacetField``: the mean of ``expr`` on every membrane facet of the chosen tags, kept on the device (the
        expressions and ``tags`` of ``assemble_scalar_membrane``)"""
        from .fields import FacetField
        return FacetField(self, expr, tags, degree, name)

    def assemble_vector(self, integrand_i=None, integrand_e=None, tags=None, degree=2):
        """``ProblemKNPEMI.assemble_vector`` for the EMI model: ``int integrand v dx(tags)`` per vertex against the P1 test
        functions, NumPy [2, n_out, n_vertices] (every Function is an aux field).  Needs ``setup_bilinear_form()`` first.  There
        are no step hooks on this problem: its right-hand side is projected and Dirichlet-lifted inside the library's assembly."""
        from .linear_forms import assemble_vector
        return assemble_vector(self, integrand_i, integrand_e, tags, degree)

    def assemble_vector_membrane(self, integrand, tags=None, degree=10):
        """``ProblemKNPEMI.assemble_vector_membrane`` for the EMI model: ``int integrand v dS(tags)`` per vertex, NumPy
        [n_out, n_vertices]"""
        from .linear_forms import assemble_vector_membrane
        return assemble_vector_membrane(self, integrand, tags, degree)

    def activation_map(self, threshold, repolarisation_threshold=None, tags=None):
        """an ``activation.ActivationMap`` of ``phi_M`` on the membranes tagged ``tags`` (default every tag of ``gamma_tags``), armed
        now: call its ``update()`` after every step, then ``result()``, ``velocity()``, ``per_tag()``"""
        from .activation import ActivationMap
        return ActivationMap(self, threshold, repolarisation_threshold, tags)

    def setup_preconditioner(self):
        """The preconditioner matrix is the EMI matrix itself (with the Dirichlet elimination).  The reference's P = sigma K + M per side
        (EMIx_problem.py:225-248) is nearly singular per side in SI units and is not built."""
        self.print("Setting up preconditioner ...")
        self.P = self.backend.csr(eliminated=True)
        return self.P

    @property
    def rhs_scale(self):
        return float(self.dt.value) if self.literal_reference_rhs else 1.0

    # ---- manufactured solution (EMI/tests/square_test.py:140-172)
    @staticmethod
    def mms_exact(x, t):
        s = np.sin(2 * np.pi * x[:, 0]) * np.sin(2 * np.pi * x[:, 1])
        return s * (1.0 + np.exp(-t)), s

    def setup_MMS_params(self):
        if self.dim != 2:
            raise NotImplementedError("the EMI manufactured solution is two-dimensional (square_test.py)")
        self.dirichlet_bcs = True
        ui, ue = self.mms_exact(self.mesh.geometry.x, 0.0)
        self.phi_M_init = ui - ue
        self.source_i, self.source_e = Function(FunctionSpace(self.mesh), "f_i"), Function(FunctionSpace(self.mesh), "f_e")

    def update_mms(self, t):
        """sources and boundary values at the new time"""
        x = self.mesh.geometry.x
        s = 8 * np.pi ** 2 * np.sin(2 * np.pi * x[:, 0]) * np.sin(2 * np.pi * x[:, 1])
        dev = self.mesh.device
        self.source_i.x.array[:] = torch.as_tensor(s * (1.0 + np.exp(-t)), device=dev)
        self.source_e.x.array[:] = torch.as_tensor(s, device=dev)
        be = self.backend
        be.f_i, be.f_e = self.source_i.x.array, self.source_e.x.array
        be.set_dirichlet_values(self._phi_e_boundary(t))

    def print_errors(self):
        """Nodal L2 errors over each side's vertices, weighted with the row sums of the side's mass matrix."""
        lm = self.local_mesh
        d = lm.coords.shape[1]
        X = lm.coords[lm.cells]
        vol = np.abs(np.linalg.det(X[:, 1:, :] - X[:, :1, :])) / float(np.prod(np.arange(1, d + 1)))
        ui, ue = self.mms_exact(lm.coords, float(self.t.value))
        errs = []
        for s, (uh, u) in enumerate(((self.wh[0].numpy(), ui), (self.wh[1].numpy(), ue))):
            w = np.zeros(lm.coords.shape[0])
            sel = self.cell_side == s
            np.add.at(w, lm.cells[sel].ravel(), np.repeat(vol[sel] / (d + 1.0), d + 1))
            errs.append(float(np.sqrt(np.sum(w * (uh - u) ** 2))))
        self.print("#-------------- ERRORS --------------#")
        self.print(f"L2 phi_i error: {errs[0]:.2e}")
        self.print(f"L2 phi_e error: {errs[1]:.2e}")
        self.errors = errs
        return errs
