"""What tests/test_functionals_irregular_host.py (no GPU) and tests/test_gpu_functionals_irregular.py share: the problems on the irregular
meshes of tests/irregular_meshes.py, the integrands of every case that reads a derivative or the normal, and per case the rounding
floor of the fp64 reference, from which the GPU test takes its tolerance.

The floor of a case is max over rows and outputs of |fp64 reference - long-double-geometry reference| / sum |w f|: how far two
correct evaluations of the same geometry are apart on that mesh.  The device is held to ``max(TOL, 8 * floor)``; the factor 8 covers
a different but equally valid fp64 evaluation order (adjugate against LU, fused multiply-adds).  The host test asserts that this
stays <= 1e-10 for every case and prints the table of DESIGN.md section 4."""
import numpy as np
import torch

import functional_ref
import irregular_meshes as IM
import membrane_functional_ref as mref
from functional_ref import TOL

TWO_TAG = "delaunay3d_5_two_tag"
EMI_HUB = "hub3d_5_60m"
VOLUME_MESHES = ["delaunay2d_12_cw", "hub2d_12_48m_cw", "hub2d_12_300", "delaunay3d_5", "hub3d_5_60", TWO_TAG]
MEMBRANE_MESHES = ["delaunay2d_12_cw", "hub2d_12_48m_cw", "delaunay3d_7", TWO_TAG]
CW = list(IM.ORIENTED)
BOUND = 1e-10                      # the largest tolerance a derivative case may take
SEEDS = {"delaunay2d_12": 11, "hub2d_12_48m": 12, "hub2d_12_300": 13, "delaunay3d_5": 14, "hub3d_5_60": 15, "delaunay3d_7": 16,
         TWO_TAG: 17, EMI_HUB: 18, "delaunay2d_92": 19}


def tolerance(floor):
    return max(TOL, 8.0 * floor)


class Prob:
    """a problem on one mesh with random nodal fields (``test_gpu_functionals._randomize``; a reoriented mesh takes its parent's seed,
    so the two hold the same fields) and the user's Functions: ``user`` random, ``lin`` affine with offset 1e3, ``const``"""

    def __init__(self, tmp, name, backend=False):
        from cgx_hip import fem
        from parity_utils import make_problem
        from test_gpu_functionals import _randomize
        self.name = name
        p = self.p = make_problem(IM.two_tag_config(tmp) if name == TWO_TAG else IM.config(tmp, name), "ci")
        self.be = p.create_backend() if backend else None
        self.user = _randomize(p, SEEDS[IM.PARENT.get(name, name)])
        lm = p.local_mesh
        self.dim = lm.coords.shape[1]
        self.L = float(np.ptp(lm.coords, axis=0).max())
        rng = np.random.default_rng(3)
        self.slope = rng.uniform(0.5, 1.5, self.dim) / self.L          # a . x spans about one unit over the mesh
        self.lin, self.const = fem.Function(p.V, "lin"), fem.Function(p.V, "const")
        write(self.lin, lm.coords @ self.slope + 1e3)
        write(self.const, np.full(lm.coords.shape[0], 7.25))
        nco = int(lm.n_cells_owned)
        self.h = float(functional_ref.cell_volumes(lm.coords[lm.cells[:nco]]).mean()) ** (1.0 / self.dim)      # a cell's length
        self.amp = fem.Constant(p.mesh, 0.25)


def write(fn, v):
    fn.x.array.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(fn.x.array.device))


def emi_problem(tmp, backend=False):
    """``ProblemEMI`` on hub3d_5_60m (Hodgkin-Huxley) with random potentials, phi_M and gates; every Function is an aux field"""
    from cgx_hip.emi_models import g_syn
    from cgx_hip.emi_problem import ProblemEMI
    cfg = {"problem_type": "EMI", "dt": 5e-5, "time_steps": 1, "C_M": 0.02, "sigma_i": 0.7, "sigma_e": 1.3, "quiet": True,
           "mesh_conversion_factor": 1e-6}
    cfg.update(IM.emi_config(tmp, EMI_HUB))
    p = ProblemEMI(cfg)
    p.add_ionic_model("HH", stim_fun=g_syn)
    p.init_ionic_model()
    if backend:
        p.setup_bilinear_form()
        p.setup_linear_form()
    rng = np.random.default_rng(SEEDS[EMI_HUB])
    nv = p.local_mesh.coords.shape[0]
    for f in (p.wh[0], p.wh[1], p.phi_M):
        write(f, rng.uniform(-0.1, 0.1, nv))
    write(p.n, rng.uniform(0.01, 0.99, nv))
    return p


# ---------------------------------------------------------------------------------------------- integrands
def normal(p, r="+"):
    from cgx_hip import fem
    return [c(r) for c in fem.FacetNormal(p.mesh)]


def grad(f, r):
    from cgx_hip import fem
    return [g(r) for g in fem.grad(f)]


def volume_forms(P, case):
    """(integrand_i, integrand_e, degree) of a volume case"""
    from cgx_hip import fem
    p, dim, h, user = P.p, P.dim, P.h, P.user
    if case == "mass_stiffness":      # u v and grad u . grad v: u a concentration (KI / KE), v the potential (an aux field)
        return tuple([p.wh[s][0] * p.wh[s][3], fem.inner(fem.grad(p.wh[s][0]), fem.grad(p.wh[s][3]))] for s in range(2)) + (2,)
    if case == "nonlinear":           # the mix of test_nonlinear_integrands_and_a_time_dependent_constant and a derivative per axis
        x = fem.SpatialCoordinate(p.mesh)
        xc = float(p.local_mesh.coords[:, 0].mean())
        forms = []
        for s in range(2):
            c, phi = p.wh[s][2], p.wh[s][p.N_ions]
            third = P.amp * fem.conditional(fem.lt(x[0], xc), c, -2.0 * p.wh[s][0]) * phi ** 2
            if dim == 3:
                third = third + fem.grad(phi)[2] * h * c
            forms.append([c * fem.ln(c / 75.0) + fem.grad(user)[0] * h * c,
                          fem.exp(12.0 * phi) + fem.sqrt(abs(user) + 1.0) * fem.grad(phi)[1] * h, third])
        return forms[0], forms[1], 4
    raise KeyError(case)


def membrane_outs(P, case):
    """(integrand, degree) of a membrane case of a KNP-EMI problem"""
    from cgx_hip import fem
    p, dim, user, lin = P.p, P.dim, P.user, P.lin
    h = float(p._fmeas.mean()) ** (1.0 / (dim - 1))      # a facet's length: derivatives times h are of the fields' order
    n = normal(p)
    x = list(fem.SpatialCoordinate(p.mesh))
    if case == "x_dot_n":
        return [fem.inner(x, n), fem.inner(x, normal(p, "-"))], 1
    if case == "normal":
        return n, 1
    if case == "affine_plus":
        return grad(lin, "+"), 1
    if case == "affine_minus":
        return grad(lin, "-"), 1
    if case == "affine_dn":           # the reference's outputs; affine_dn_device holds the sums the device must cancel
        return [fem.NormalDerivative(lin, "+"), fem.NormalDerivative(lin, "-")], 1
    ci, ce, phi_e = p.wh[0][1], p.wh[1][2], p.wh[1][3]
    if case == "random_plus":         # value, d/dx_a on the '+' cell, d/dn('+'), normal components: 2 dim + 2 aux slots (8 in 3D)
        outs = [fem.exp(ci / 150.0) * fem.grad(user)[0]("+") * h + ci * n[0], user * p.phi_m_prev * ci / ce + fem.grad(user)[1]("+") * h * n[1],
                fem.NormalDerivative(user, "+") * h * ce + n[dim - 1] ** 2 + (fem.grad(user)[2]("+") * h if dim == 3 else 0.0)]
        return outs, 4
    if case == "random_minus":        # d/dx_a on the '-' cell, d/dn('-'), the other side's normal
        nm = normal(p, "-")
        outs = [fem.sqrt(abs(fem.grad(user)[0]("-")) * h + 1.0) * ce, fem.grad(phi_e)[1] * h * ci + fem.grad(user)[dim - 1]("-") * h * nm[0],
                fem.NormalDerivative(user, "-") * h * user + fem.NormalDerivative(phi_e) * h * nm[dim - 1]]
        return outs, 4
    if case in ("flux_i", "flux_e"):  # the forms of utils/calc_fluxes.py, as tests/test_gpu_membrane_functionals.py writes them
        s, r = (0, "+") if case == "flux_i" else (1, "-")
        phi = p.wh[s][p.N_ions]
        dphi = fem.dot(grad(phi, r), normal(p, r))
        return [-ion["Di"] * (fem.dot(grad(p.wh[s][j], r), normal(p, r)) + (ion["z"] / p.psi) * p.wh[s][j] * dphi)
                for j, ion in enumerate(p.ion_list)], 10
    raise KeyError(case)


def affine_dn_device(P):
    """d/dn('+'), the two sides' normal derivatives added, and dot() with the other side's normal added to d/dn('+'): the last two
    integrate to zero for a nodally affine field"""
    from cgx_hip import fem
    dp, dm = fem.NormalDerivative(P.lin, "+"), fem.NormalDerivative(P.lin, "-")
    return [dp, dp + dm, fem.dot(grad(P.lin, "+"), normal(P.p, "-")) + dp]


def emi_outs(p):
    """the integrand of test_gpu_membrane_functionals.test_emi_transmembrane_current"""
    from cgx_hip import fem
    return [-p.sigma_i * fem.dot(grad(p.wh[0], "+"), normal(p)), -p.sigma_e * fem.NormalDerivative(p.wh[1]), p.phi_M * p.n + (p.wh[0] - p.wh[1])]


def closed_groups(P):
    """rows whose facets close around whole intracellular cells: one membrane tag on the single-cell meshes; on the two-tag split the
    two membranes pooled (the cells 2 and 3 touch at x = 0.5, where there is no membrane)"""
    return [tuple(int(t) for t in P.p.gamma_tags)]


VOLUME_CASES = ["mass_stiffness", "nonlinear"]
MEMBRANE_CASES = ["x_dot_n", "normal", "affine_plus", "affine_minus", "affine_dn", "random_plus", "random_minus", "flux_i", "flux_e"]
CLOSED = ("x_dot_n", "normal", "affine_plus", "affine_minus", "affine_dn")      # cases over closed_groups


def volume_reference(P, case, longdouble=False):
    fi, fe, degree = volume_forms(P, case)
    return functional_ref.reference(P.p, fi, fe, degree=degree, longdouble=longdouble)[2:]


def membrane_reference(P, case, longdouble=False):
    outs, degree = membrane_outs(P, case)
    return mref.reference(P.p, outs, tags=closed_groups(P) if case in CLOSED else None, degree=degree, longdouble=longdouble)[1:]


_FLOORS = {}


def _floor(key, ref):
    if key not in _FLOORS:
        (v, s), (vl, _) = ref(False), ref(True)
        assert np.all(s > 0), key
        _FLOORS[key] = float(np.max(np.abs(v - vl) / s))
    return _FLOORS[key]


def volume_floor(P, case):
    return _floor(("volume", P.name, case), lambda ld: volume_reference(P, case, ld))


def membrane_floor(P, case):
    return _floor(("membrane", P.name, case), lambda ld: membrane_reference(P, case, ld))


def emi_floor(p):
    return _floor(("membrane", EMI_HUB, "emi_current"), lambda ld: mref.reference(p, emi_outs(p), longdouble=ld)[1:])


def floor_table():
    """the floors computed so far, as the lines of DESIGN.md's table"""
    return [f"{kind:9s} {mesh:22s} {case:15s} floor {f:.2e}  tolerance {tolerance(f):.2e}" for (kind, mesh, case), f in sorted(_FLOORS.items())]


# ---------------------------------------------------------------------------------------------- mesh statistics
def mesh_stats(coords, cells, tags, intra=(1,), extra=(2,), how=None):
    """what the issue's table lists: share of det < 0, the largest condition number of an edge matrix, per membrane facet the local
    index of its opposite vertex in T+ and T-, and the facet measures"""
    from cgx_hip import mesh as meshmod
    E = coords[cells][:, 1:, :] - coords[cells][:, :1, :]
    det = np.linalg.det(E)
    gamma, gtags, fv = meshmod.gamma_integration_entities(cells, tags, intra, extra, how)
    opp = mref.opposite_vertices(cells, gamma, fv)
    local = np.stack([np.argmax(cells[gamma[:, c]] == opp[:, s:s + 1], axis=1) for s, c in enumerate((0, 2))], axis=1)
    X = coords[fv]
    e = X[:, 1:, :] - X[:, :1, :]
    meas = np.linalg.norm(e[:, 0], axis=1) if fv.shape[1] == 2 else np.linalg.norm(np.cross(e[:, 0], e[:, 1]), axis=1) / 2.0
    return {"neg": float((det < 0).mean()), "cond": float(np.linalg.cond(E).max()), "local": local, "meas": meas, "fv": fv, "gamma": gamma,
            "n_cells": cells.shape[0], "n_facets": fv.shape[0], "opp": opp}


# ---------------------------------------------------------------------------------------------- block edges (raw ABI)
def _one(n):
    return [0, n]


SEG_PTRS = {
    "n1": _one(1), "n127": _one(127), "n128": _one(128), "n129": _one(129), "n257": _one(257),
    "end127_one_one": [0, 127, 128, 129],
    "two_blocks": [0, 128, 256],
    "empties": [0, 0, 1, 1, 128, 128, 257],
    "straddle_empty_last": [0, 126, 130, 130],
    "64_ones_then_65": list(range(65)) + [129],
}
FN_BT = 128


def seg_ptr_for(name, n_items):
    """the named map with its last entry capped at ``n_items`` (n = 257 is for the cells; the facet meshes have at least 129 facets)"""
    sp = np.minimum(np.array(SEG_PTRS[name], dtype=np.int32), n_items)
    return sp


def nodal_rounding_bounds(P):
    """Per side, the bound on the integral over all membrane facets of any directional derivative of ``P.lin`` that comes from storing
    the nodal values in fp64: the values lie in [1000, 1024), so each is off by at most 2^-44 and a difference f_b - f_0 by 2^-43;
    sum_b g_b (f_b - f_0) with |g_b . w| <= |g_b|_1 for |w|_2 <= 1 moves by at most 2^-43 sum_b |grad(lambda_b)|_1 per facet."""
    p = P.p
    lm = p.local_mesh
    fv = np.asarray(p._fv)
    opp = mref.opposite_vertices(np.asarray(lm.cells), np.asarray(lm.gamma), fv)
    assert 1000.0 <= P.lin.numpy().min() and P.lin.numpy().max() < 1024.0
    out = []
    for s in range(2):
        G = functional_ref.simplex_gradients(lm.coords[np.concatenate([fv, opp[:, s:s + 1]], axis=1)])
        out.append(float((np.asarray(p._fmeas) * np.abs(G[:, 1:, :]).sum(axis=(1, 2))).sum() * 2.0 ** -43))
    return out
