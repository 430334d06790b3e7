"""Independent NumPy / SciPy restatement of the EMI model (reference src/CGx/EMI), the checker of tests/test_emi_host.py and
tests/test_gpu_emi.py.  It shares nothing with the code under test except the mesh generators.

P1 on simplices; phi_i lives on the vertices of intracellular cells, phi_e on those of extracellular cells, a membrane vertex carries
both.  Unknown = node: vertices in order, a membrane vertex contributes its intra node, then its extra node.

    A = [ dt s_i K_i + C_M M_G      -C_M M_G          ]        (EMIx_problem.py:152-157)
        [ -C_M M_G                  dt s_e K_e + C_M M_G ]
    b_i = dt M_i f_i + s int_G (C_M phi_M - dt I_ch) v dS,    b_e = dt M_e f_e - s (the same)

s = 1: the consistent backward-Euler form of EMI/tests/square_test.py:352-355; s = dt: the literal EMIx_problem.py:215-217.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


# ------------------------------------------------------------------------------------------ quadrature
def facet_quadrature(dim, degree=10):
    """Points (barycentric, on the reference facet) and weights (sum 1) exact to ``degree``: Gauss-Legendre on an edge, the collapsed
    Gauss-Jacobi product rule on a triangle."""
    m = degree // 2 + 1
    xg, wg = np.polynomial.legendre.leggauss(m)
    t, wt = 0.5 * (xg + 1.0), 0.5 * wg
    if dim == 2:
        return np.column_stack([1.0 - t, t]), wt
    from scipy.special import roots_jacobi
    xj, wj = roots_jacobi(m, 1.0, 0.0)
    u, wu = 0.5 * (xj + 1.0), 0.25 * wj            # weight (1 - u) on [0, 1]
    pts = np.array([(1.0 - a - b * (1.0 - a), a, b * (1.0 - a)) for a in u for b in t])
    w = np.array([p * q for p in wu for q in wt])
    return pts, w / w.sum()


# ------------------------------------------------------------------------------------------ membrane models
def g_syn(t):
    """the stimulus of EMIx_ionic_model.py:15-23"""
    return 40.0 * np.exp(-np.mod(t, 0.01) / 0.002)


HH = dict(g_Na_bar=1200.0, g_K_bar=360.0, g_Na_leak=1.0, g_K_leak=4.0, g_Cl_leak=0.0, V_rest=-0.065, E_Na=54.8e-3, E_K=-88.98e-3,
          E_Cl=0.0, n0=0.27622914792, m0=0.03791834627, h0=0.68848921811, substeps=25)


def passive_current(phi, n, m, h, t):
    return phi


def hh_current(phi, n, m, h, t, stim=g_syn):
    g_Na = HH["g_Na_leak"] + HH["g_Na_bar"] * m ** 3 * h + stim(t)
    g_K = HH["g_K_leak"] + HH["g_K_bar"] * n ** 4
    return g_Na * (phi - HH["E_Na"]) + g_K * (phi - HH["E_K"]) + HH["g_Cl_leak"] * (phi - HH["E_Cl"])


def hh_gating_step(phi, n, m, h, dt, rush_larsen=True, substeps=25, V_rest=-0.065):
    """EMIx_ionic_model.py:139-200"""
    V = 1000.0 * (phi - V_rest)
    a_n = 0.01e3 * (10.0 - V) / (np.exp((10.0 - V) / 10.0) - 1.0)
    b_n = 0.125e3 * np.exp(-V / 80.0)
    a_m = 0.1e3 * (25.0 - V) / (np.exp((25.0 - V) / 10.0) - 1.0)
    b_m = 4.0e3 * np.exp(-V / 18.0)
    a_h = 0.07e3 * np.exp(-V / 20.0)
    b_h = 1.0e3 / (np.exp((30.0 - V) / 10.0) + 1.0)
    dto = dt / substeps
    out = []
    for y, a, b in ((n, a_n, b_n), (m, a_m, b_m), (h, a_h, b_h)):
        y = y.copy()
        if rush_larsen:
            tau = 1.0 / (a + b)
            yinf, e = a * tau, np.exp(-dto / tau)
            for _ in range(substeps):
                y = yinf + (y - yinf) * e
        else:
            for _ in range(substeps):
                y = y + dto * a * (1.0 - y) - dto * b * y
        out.append(y)
    return out


# ------------------------------------------------------------------------------------------ the discrete problem
class EmiRef:
    def __init__(self, coords, cells, side, gamma, dt, C_M=1.0, sigma_i=1.0, sigma_e=1.0, facet_model=None, degree=10):
        """side: 0 intra / 1 extra per cell; gamma: rows (cell+, lf+, cell-, lf-), '+' intracellular; facet_model: per membrane facet
        the index into ``self.models`` (default all 0)."""
        self.coords = np.asarray(coords, dtype=np.float64)
        self.cells = np.asarray(cells, dtype=np.int64)
        self.side = np.asarray(side, dtype=np.int64)
        self.dim = d = self.coords.shape[1]
        self.dt, self.C_M, self.sigma = float(dt), float(C_M), (float(sigma_i), float(sigma_e))
        nv = self.coords.shape[0]
        in_i, in_e = np.zeros(nv, bool), np.zeros(nv, bool)
        in_i[self.cells[self.side == 0].ravel()] = True
        in_e[self.cells[self.side == 1].ravel()] = True
        cnt = in_i.astype(np.int64) + in_e
        off = np.cumsum(cnt) - cnt
        self.node_i = np.where(in_i, off, -1)
        self.node_e = np.where(in_e, off + in_i, -1)
        self.n = int(cnt.sum())
        self.node_vertex = np.empty(self.n, dtype=np.int64)
        self.node_side = np.empty(self.n, dtype=np.int64)
        for s, nd in ((0, self.node_i), (1, self.node_e)):
            v = np.nonzero(nd >= 0)[0]
            self.node_vertex[nd[v]] = v
            self.node_side[nd[v]] = s
        # volume matrices per side
        X = self.coords[self.cells]
        J = X[:, 1:, :] - X[:, :1, :]
        vol = np.abs(np.linalg.det(J)) / math.factorial(d)
        Gm = np.transpose(np.linalg.inv(J), (0, 2, 1))                     # rows: grad lambda_1..d
        G = np.concatenate([-Gm.sum(axis=1, keepdims=True), Gm], axis=1)   # (nc, d+1, d)
        Kc = vol[:, None, None] * np.einsum("cak,cbk->cab", G, G)
        Mc = vol[:, None, None] / ((d + 1.0) * (d + 2.0)) * (1.0 + np.eye(d + 1))[None]
        cn = np.where(self.side[:, None] == 0, self.node_i[self.cells], self.node_e[self.cells])
        r = np.repeat(cn, d + 1, axis=1).ravel()
        c = np.tile(cn, (1, d + 1)).ravel()
        self.K = sp.csr_matrix((Kc.ravel(), (r, c)), shape=(self.n, self.n))
        self.M = sp.csr_matrix((Mc.ravel(), (r, c)), shape=(self.n, self.n))
        sig = np.where(self.side == 0, self.sigma[0], self.sigma[1])
        Ks = sp.csr_matrix(((sig[:, None, None] * Kc).ravel(), (r, c)), shape=(self.n, self.n))
        # membrane
        gamma = np.asarray(gamma, dtype=np.int64).reshape(-1, 4)
        loc = np.array([[a for a in range(d + 1) if a != lf] for lf in range(d + 1)])
        self.fv = self.cells[gamma[:, 0][:, None], loc[gamma[:, 1]]] if len(gamma) else np.zeros((0, d), dtype=np.int64)
        Xf = self.coords[self.fv]
        if d == 2:
            self.fmeas = np.linalg.norm(Xf[:, 1] - Xf[:, 0], axis=1)
        else:
            self.fmeas = 0.5 * np.linalg.norm(np.cross(Xf[:, 1] - Xf[:, 0], Xf[:, 2] - Xf[:, 0]), axis=1)
        Mg = self.fmeas[:, None, None] / (d * (d + 1.0)) * (1.0 + np.eye(d))[None]
        fi, fe = self.node_i[self.fv], self.node_e[self.fv]
        rows, cols, vals = [], [], []
        for ra, ca, sg in ((fi, fi, 1.0), (fe, fe, 1.0), (fi, fe, -1.0), (fe, fi, -1.0)):
            rows.append(np.repeat(ra, d, axis=1).ravel())
            cols.append(np.tile(ca, (1, d)).ravel())
            vals.append(sg * self.C_M * Mg.ravel())
        G_ = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(self.n, self.n))
        self.A = (self.dt * Ks + G_).tocsr()
        self.A.sum_duplicates()
        self.A.sort_indices()
        self.absA_gamma = abs(G_)
        # sum of the magnitudes of the cell and facet terms behind each entry of A: an entry whose terms cancel is known to eps of this
        absKs = sp.csr_matrix((np.abs(sig[:, None, None] * Kc).ravel(), (r, c)), shape=(self.n, self.n))
        self.absA_terms = (self.dt * absKs + self.absA_gamma).tocsr()
        self.q_pts, self.q_w = facet_quadrature(d, degree)
        self.facet_model = np.zeros(len(self.fv), dtype=np.int64) if facet_model is None else np.asarray(facet_model, dtype=np.int64)
        self.models = [passive_current]
        self.bc_nodes = np.zeros(0, dtype=np.int64)
        self.nullspace = False
        self._lu = None
        # lumped mass per node (row sums of the side's mass matrix): the weights of the nodal L2 norm
        self.m_lumped = np.asarray(self.M.sum(axis=1)).ravel()

    # ---- boundary conditions
    def exterior_extra_nodes(self):
        """extra nodes of the vertices on the exterior boundary (facets with one cell)"""
        d = self.dim
        f = np.vstack([np.sort(np.delete(self.cells, lf, axis=1), axis=1) for lf in range(d + 1)])
        u, cnt = np.unique(f, axis=0, return_counts=True)
        v = np.unique(u[cnt == 1].ravel())
        nd = self.node_e[v]
        return nd[nd >= 0]

    def set_dirichlet(self, nodes):
        self.bc_nodes = np.asarray(nodes, dtype=np.int64)
        self._lu = None

    def operator(self):
        """A with the Dirichlet rows and columns eliminated (identity there)"""
        if len(self.bc_nodes) == 0:
            return self.A
        keep = np.ones(self.n)
        keep[self.bc_nodes] = 0.0
        D = sp.diags(keep)
        return (D @ self.A @ D + sp.diags(1.0 - keep)).tocsr()

    # ---- right-hand side
    def membrane_terms(self, phi_m, n=None, m=None, h=None, t=0.0):
        """(+ part, |.| part) of int_G (C_M phi_M - dt I_ch) v dS per vertex-of-facet, as arrays (n_facets, d)"""
        lam = self.q_pts                                           # (q, d)
        at = lambda nodal: nodal[self.fv] @ lam.T                  # (nf, q)
        ph = at(phi_m)
        zero = np.zeros_like(phi_m)
        gates = [at(zero if g is None else g) for g in (n, m, h)]
        I = np.zeros_like(ph)
        for k, model in enumerate(self.models):
            sel = self.facet_model == k
            if sel.any():
                I[sel] = model(ph[sel], gates[0][sel], gates[1][sel], gates[2][sel], t)
        fg = self.C_M * ph - self.dt * I
        w = self.fmeas[:, None] * self.q_w[None, :]
        val = np.einsum("fq,qa->fa", w * fg, lam)
        mag = np.einsum("fq,qa->fa", w * (np.abs(self.C_M * ph) + np.abs(self.dt * I)), lam)
        return val, mag

    def rhs(self, phi_m, n=None, m=None, h=None, t=0.0, f_i=None, f_e=None, g=None, scale=1.0, with_magnitude=False):
        """b and (optionally) S, the sum of the magnitudes of everything added into each row"""
        b = np.zeros(self.n)
        S = np.zeros(self.n)
        f_nodal = np.zeros(self.n)
        for s, f in ((0, f_i), (1, f_e)):
            if f is not None:
                sel = self.node_side == s
                f_nodal[sel] = np.asarray(f)[self.node_vertex[sel]]
        b += self.dt * (self.M @ f_nodal)
        S += self.dt * (abs(self.M) @ np.abs(f_nodal))
        val, mag = self.membrane_terms(phi_m, n, m, h, t)
        np.add.at(b, self.node_i[self.fv].ravel(), scale * val.ravel())
        np.add.at(b, self.node_e[self.fv].ravel(), -scale * val.ravel())
        np.add.at(S, self.node_i[self.fv].ravel(), abs(scale) * mag.ravel())
        np.add.at(S, self.node_e[self.fv].ravel(), abs(scale) * mag.ravel())
        if len(self.bc_nodes):
            gv = np.zeros(self.n)
            gv[self.bc_nodes] = np.asarray(g)[self.bc_nodes] if g is not None else 0.0
            b -= self.A @ gv
            S += abs(self.A) @ np.abs(gv)
            b[self.bc_nodes] = gv[self.bc_nodes]
            S[self.bc_nodes] = np.abs(gv[self.bc_nodes])
        elif self.nullspace:
            b -= b.mean()
            S += np.abs(S).mean()
        return (b, S) if with_magnitude else b

    # ---- direct solve
    def solve(self, b):
        """sparse LU; pure Neumann: the constant is fixed by a Lagrange multiplier (mean-zero solution)"""
        if len(self.bc_nodes) or not self.nullspace:
            if self._lu is None:
                self._lu = spla.splu(self.operator().tocsc())
            return self._lu.solve(b)
        if self._lu is None:
            one = sp.csr_matrix(np.ones((self.n, 1)))
            self._lu = spla.splu(sp.bmat([[self.A, one], [one.T, None]]).tocsc())
        return self._lu.solve(np.concatenate([b, [0.0]]))[:self.n]

    # ---- k steps of preconditioned conjugate gradients
    def pcg(self, b, k, pc="none", norm_type="preconditioned", x0=None, dtype=np.float64):
        """Exactly ``k`` iterations of the recurrence that ``knp_emi_cg_solve`` documents (include/knpemi_hip.h; PETSc's KSPCG with a
        projected preconditioner), on ``self.operator()``, in ``dtype`` (``np.longdouble`` for the reference's own rounding spread):

            x = x0 (b on the Dirichlet nodes);  r = b - A x, its mean removed once when the null space is on
            z = B r;  z' = z - mean(z) (null space on);  beta = r . z';  p = z'
            k times:  alpha = beta / (p . A p);  x += alpha p;  r -= alpha A p;  z, z', beta_new as above;  p = z' + (beta_new / beta) p

        ``pc``: "none" (B = I) or "jacobi" (B = 1 / diag A; 1 on Dirichlet nodes).  Norms: preconditioned ||z'||_2, unpreconditioned
        ||r||_2, natural sqrt|r . z'|.  Returns x, r and the k + 1 norms (before the first iteration, then after each).  Sums are
        NumPy's own (pairwise): nothing of the kernels' block order is restated."""
        A = self.operator().tocsr()
        A.sort_indices()
        T = np.dtype(dtype).type
        n = self.n
        ns = self.nullspace and len(self.bc_nodes) == 0
        data, indices, starts = A.data.astype(T), A.indices, A.indptr[:-1]
        assert np.all(np.diff(A.indptr) > 0)                       # every row holds its diagonal: reduceat sees no empty segment
        mul = (lambda v: A @ v) if T is np.float64 else (lambda v: np.add.reduceat(data * v[indices], starts))
        if pc == "jacobi":
            d = A.diagonal().astype(T)
            d[self.bc_nodes] = 1
            B = lambda v: v / d
        elif pc == "none":
            B = lambda v: v.copy()
        else:
            raise ValueError(pc)
        b = np.asarray(b).astype(T)
        x = np.zeros(n, dtype=T) if x0 is None else np.asarray(x0).astype(T)
        x[self.bc_nodes] = b[self.bc_nodes]
        r = b - mul(x)
        if ns:
            r = r - r.sum() / T(n)

        def apply(r):
            z = B(r)
            if ns:
                z = z - z.sum() / T(n)
            beta = r @ z
            norm = {"preconditioned": np.sqrt(z @ z), "unpreconditioned": np.sqrt(r @ r), "natural": np.sqrt(abs(beta))}[norm_type]
            return z, beta, norm
        z, beta, norm = apply(r)
        p = z.copy()
        norms = [norm]
        for _ in range(k):
            q = mul(p)
            alpha = beta / (p @ q)
            x = x + alpha * p
            r = r - alpha * q
            z, beta_new, norm = apply(r)
            p = z + (beta_new / beta) * p
            beta = beta_new
            norms.append(norm)
        return x, r, np.array(norms, dtype=T)

    def split(self, x):
        """nodal phi_i, phi_e (0 where a vertex has no node of that side) and phi_M = phi_i - phi_e"""
        nv = self.coords.shape[0]
        pi, pe = np.zeros(nv), np.zeros(nv)
        vi, ve = self.node_i >= 0, self.node_e >= 0
        pi[vi] = x[self.node_i[vi]]
        pe[ve] = x[self.node_e[ve]]
        return pi, pe, pi - pe


def from_tags(coords, cells, cell_tags, intra_tags, gamma, **kw):
    side = np.where(np.isin(cell_tags, intra_tags), 0, 1)
    return EmiRef(coords, cells, side, gamma, **kw)


# ------------------------------------------------------------------------------------------ time stepping
def hh_trajectory(ref, steps, phi0=-0.06774, rush_larsen=True, stim=g_syn, scale=1.0):
    """``steps`` HH steps from rest by LU: per step the right-hand side at the new time with the current phi_M and gates, the solve,
    phi_M = phi_i - phi_e, then the gating update (25 sub-steps)."""
    nv = ref.coords.shape[0]
    ref.models = [lambda p, n, m, h, t: hh_current(p, n, m, h, t, stim)]
    ref.nullspace = len(ref.bc_nodes) == 0
    phi = np.full(nv, phi0)
    n, m, h = np.full(nv, HH["n0"]), np.full(nv, HH["m0"]), np.full(nv, HH["h0"])
    t = 0.0
    for _ in range(steps):
        t += ref.dt
        x = ref.solve(ref.rhs(phi, n, m, h, t, scale=scale))
        phi = ref.split(x)[2]
        n, m, h = hh_gating_step(phi, n, m, h, ref.dt, rush_larsen, HH["substeps"], HH["V_rest"])
    return phi, n, m, h


# ------------------------------------------------------------------------------------------ manufactured solution (square_test.py:140-172)
def mms_exact(x, t):
    s = np.sin(2 * np.pi * x[:, 0]) * np.sin(2 * np.pi * x[:, 1])
    return s * (1.0 + np.exp(-t)), s


def mms_sources(x, t):
    s = 8 * np.pi ** 2 * np.sin(2 * np.pi * x[:, 0]) * np.sin(2 * np.pi * x[:, 1])
    return s * (1.0 + np.exp(-t)), s


def mms_errors(ref, phi_i, phi_e, t):
    """lumped-mass nodal L2 errors over each side's nodes"""
    ui, ue = mms_exact(ref.coords, t)
    out = []
    for s, (uh, u) in enumerate(((phi_i, ui), (phi_e, ue))):
        sel = ref.node_side == s
        v = ref.node_vertex[sel]
        out.append(float(np.sqrt(np.sum(ref.m_lumped[sel] * (uh[v] - u[v]) ** 2))))
    return out


def mms_problem(N, dt=0.01):
    """unit square, inner box [0.25, 0.75]^2 intracellular, passive membrane, C_M = sigma = 1, phi_e Dirichlet on the exterior"""
    from cgx_hip import mesh as meshmod
    coords, cells = meshmod.create_unit_square(N)
    tags = meshmod.mark_subdomains_box(coords, cells)
    gamma, _, _ = meshmod.gamma_integration_entities(cells, tags, (1,), (2,), None)
    ref = from_tags(coords, cells, tags, (1,), gamma, dt=dt, C_M=1.0, sigma_i=1.0, sigma_e=1.0)
    ref.set_dirichlet(ref.exterior_extra_nodes())
    return ref


def mms_run(N, dt=0.01, steps=2):
    ref = mms_problem(N, dt)
    ui0, ue0 = mms_exact(ref.coords, 0.0)
    phi_m = ui0 - ue0
    t = 0.0
    for _ in range(steps):
        t += dt
        fi, fe = mms_sources(ref.coords, t)
        g = np.zeros(ref.n)
        g[ref.bc_nodes] = mms_exact(ref.coords, t)[1][ref.node_vertex[ref.bc_nodes]]
        x = ref.solve(ref.rhs(phi_m, t=t, f_i=fi, f_e=fe, g=g))
        phi_i, phi_e, phi_m = ref.split(x)
    return mms_errors(ref, phi_i, phi_e, t), ref
