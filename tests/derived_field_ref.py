"""NumPy fp64 reference of the derived fields (cgx_hip/fields.py, csrc/knp_fields.inc): the mean of an expression per cell and per
membrane facet, and the measure-weighted projection of item values onto the vertices.

Per-item means: the rule and the expressions as tests/functional_ref.py / tests/membrane_functional_ref.py take them
(``fem.evaluate_numpy``, derivatives from the simplex gradients with the differences first, the normal from the intracellular cell),
without the measure: mean_i = sum_q q_w[q] f(x_q), and each item's scale sum_q |q_w[q] f(x_q)|.  ``longdouble``: the geometry
(gradients, normal) from ``functional_ref.geometry_longdouble``; the distance of the two is the rounding floor of a case
(``floor``), from which the GPU test takes ``functionals_irregular.tolerance``.

Projection: ``inverted_index`` restates the builder of knp_project_create (per vertex the items that hold it, ascending), ``project``
sums every list in that order, with the scale sum |measure value| / sum measure; ``plan_info`` restates the lane rule and the split
rule of the plan."""
import math

import numpy as np

import functional_ref
import membrane_functional_ref as mref

SPLIT = 512          # PROJ_SPLIT of csrc/knp_fields.inc: a longer list is cut into chunks of this many entries
LANES = (2, 4, 8, 16, 32)      # the instantiated lane widths of k_project


def _means(exprs, env, qw, n):
    from cgx_hip import fem
    mean, scale = [], []
    for e in exprs:
        wf = qw[None, :] * np.broadcast_to(fem.evaluate_numpy(e, env), (n, len(qw)))
        mean.append(np.array([math.fsum(r) for r in wf]))
        scale.append(np.abs(wf).sum(axis=1))
    return np.stack(mean, axis=1).reshape(n, len(exprs)), np.stack(scale, axis=1).reshape(n, len(exprs))


def cell_means(coords, cells, exprs, qb, qw, longdouble=False):
    """(mean [n, n_out], scale [n, n_out]) over the cells [n, d + 1]"""
    X = coords[cells]
    n, d = len(cells), coords.shape[1]
    G = functional_ref.simplex_gradients(X, longdouble)
    xq = np.einsum("qa,nak->nqk", qb, X)
    fields, grads = {}, {}
    for e in exprs:
        for f in functional_ref.functions_of(e):
            if id(f) in fields:
                continue
            fv = f.numpy()[cells]
            fields[id(f)] = np.einsum("qa,na->nq", qb, fv)
            for k in range(d):
                grads[(id(f), k)] = np.broadcast_to((G[:, 1:, k] * (fv[:, 1:] - fv[:, :1])).sum(axis=1)[:, None], (n, len(qw)))
    return _means(exprs, {"x": [xq[:, :, k] for k in range(d)], "fields": fields, "grads": grads}, qw, n)


def facet_means(coords, fv, opp, exprs, qp, qw, sides=None, longdouble=False):
    """(mean [n, n_out], scale [n, n_out]) over the facets ``fv`` [n, d] with the opposite vertices ``opp`` [n, 2]; ``sides`` as
    ``membrane_functional_ref.integrate_facets`` takes it"""
    sides = sides or {}
    n, d = fv.shape
    xq = np.einsum("qa,nak->nqk", qp, coords[fv])
    bc = lambda a: np.broadcast_to(np.asarray(a)[:, None], (n, len(qw)))
    cellv, G = [], []
    for s in range(2):
        ok = n > 0 and np.all(opp[:, s] >= 0)
        cellv.append(np.concatenate([fv, opp[:, s:s + 1]], axis=1) if ok else None)
        G.append(functional_ref.simplex_gradients(coords[cellv[s]], longdouble) if ok else None)
    nrm = None
    if G[0] is not None and longdouble:
        g = functional_ref.geometry_longdouble(coords[cellv[0]])[0][:, d, :]
        nrm = (-g / np.sqrt((g * g).sum(axis=1))[:, None]).astype(np.float64)
    elif G[0] is not None:
        g = G[0][:, d, :]
        nrm = -g / np.linalg.norm(g, axis=1)[:, None]
    fields, grads, nds = {}, {}, {}
    for e in exprs:
        for f in mref.functions_of(e):
            if id(f) in fields:
                continue
            val = f.numpy()
            fields[id(f)] = np.einsum("qa,na->nq", qp, val[fv])
            for s, r in enumerate("+-"):
                if G[s] is None or nrm is None:
                    continue
                fc = val[cellv[s]]
                diff = fc[:, 1:] - fc[:, :1]
                for k in range(d):
                    grads[(id(f), k, r)] = bc((G[s][:, 1:, k] * diff).sum(axis=1))
                gn = np.einsum("nbk,nk->nb", G[s][:, 1:, :], nrm if s == 0 else -nrm)
                nds[(id(f), r)] = bc((gn * diff).sum(axis=1))
                if sides.get(id(f)) == s:
                    nds[(id(f), None)] = nds[(id(f), r)]
                    for k in range(d):
                        grads[(id(f), k)] = grads[(id(f), k, r)]
    env = {"x": [xq[:, :, k] for k in range(d)], "fields": fields, "grads": grads, "normal_derivs": nds,
           "normal": None if nrm is None else [bc(nrm[:, k]) for k in range(d)]}
    return _means(exprs, env, qw, n)


def _exprs(g):
    return list(g) if isinstance(g, (list, tuple)) else [g]


def cell_field(problem, expr_i=None, expr_e=None, tags=None, degree=1, longdouble=False):
    """(cells, side, mean, scale) in the order of ``CellField``: the intracellular cells of the chosen tags first, each side's ascending"""
    from cgx_hip.functionals import quadrature
    p = problem
    lm = p.local_mesh
    nco = int(lm.n_cells_owned)
    qb, qw = quadrature(lm.coords.shape[1], degree)
    side_tags = [[int(t) for t in p.intra_tags], [int(t) for t in np.ravel(p.extra_tag)]]
    ctags = np.asarray(lm.cell_tags[:nco])
    cells, side, mean, scale = [], [], [], []
    for s, g in enumerate((expr_i, expr_e)):
        if g is None:
            continue
        chosen = side_tags[s] if tags is None else [int(t) for t in tags if int(t) in side_tags[s]]
        idx = np.nonzero(np.isin(ctags, chosen))[0]
        m, sc = cell_means(lm.coords, np.asarray(lm.cells)[idx], _exprs(g), qb, qw, longdouble)
        cells.append(idx); side.append(np.full(len(idx), s)); mean.append(m); scale.append(sc)
    return np.concatenate(cells), np.concatenate(side), np.concatenate(mean), np.concatenate(scale)


def facet_field(problem, expr, tags=None, degree=1, longdouble=False):
    """(facets, mean, scale) in the order of ``FacetField``: the facets of the chosen membrane tags, ascending"""
    from cgx_hip.mesh import facet_quadrature
    p = problem
    lm = p.local_mesh
    qp, qw = facet_quadrature(lm.coords.shape[1], degree)
    ftags = np.asarray(p.gamma_facet_tags)
    chosen = [int(t) for t in p.gamma_tags] if tags is None else [int(t) for t in np.ravel(tags)]
    idx = np.nonzero(np.isin(ftags, chosen))[0]
    fv = np.asarray(p._fv)
    opp = mref.opposite_vertices(np.asarray(lm.cells), np.asarray(lm.gamma), fv)
    m, sc = facet_means(lm.coords, fv[idx], opp[idx], _exprs(expr), np.asarray(qp), np.asarray(qw), mref.default_sides(p), longdouble)
    return idx, m, sc


def floor(ref):
    """``ref(longdouble)`` -> (mean, scale): the largest |fp64 - long-double geometry| / scale over items and outputs"""
    (v, s), (vl, _) = ref(False), ref(True)
    assert np.all(s > 0)
    return float(np.max(np.abs(v - vl) / s))


# ---------------------------------------------------------------------------------------------- projection
def inverted_index(n_vertices, item_vertices):
    """(ptr [n_vertices + 1], items [n_entries]): per vertex the items that hold it, ascending -- the builder of knp_project_create,
    restated as a counting sort over the items in order"""
    iv = np.asarray(item_vertices, dtype=np.int64)
    ptr = np.zeros(n_vertices + 1, dtype=np.int64)
    for w in iv:
        for v in w:
            ptr[v + 1] += 1
    np.cumsum(ptr, out=ptr)
    nxt, items = ptr[:-1].copy(), np.zeros(ptr[-1], dtype=np.int64)
    for i, w in enumerate(iv):
        for v in w:
            items[nxt[v]] = i
            nxt[v] += 1
    return ptr, items


def plan_info(ptr):
    """what knp_project_get_info reports for the index ``ptr``: the lanes per list (the smallest power of two in 2 .. 32 that is not
    below the mean length of the non-empty lists), the longest list, the lists cut into chunks of SPLIT, the units"""
    ln = np.diff(ptr)
    mean = ln.sum() / max(int((ln > 0).sum()), 1)
    lanes = 2
    while lanes < 32 and lanes < mean:
        lanes *= 2
    split = ln > SPLIT
    units = int((~split).sum() + (-(-ln[split] // SPLIT)).sum())
    return {"lanes": lanes, "longest": int(ln.max(initial=0)), "n_split": int(split.sum()), "n_units": units, "split": SPLIT}


def project(n_vertices, item_vertices, measure, values, fill=np.nan):
    """(out [n_out, n_vertices], scale [n_out, n_vertices], ptr): out[j][v] = sum over v's list of measure_i values[i][j] / sum of
    measure_i, ``fill`` for an empty list; scale = sum |measure_i values[i][j]| / sum measure_i (1 for an empty list)"""
    values = np.asarray(values, dtype=np.float64).reshape(len(measure), -1)
    ptr, items = inverted_index(n_vertices, item_vertices)
    out = np.full((values.shape[1], n_vertices), fill, dtype=np.float64)
    scale = np.ones((values.shape[1], n_vertices))
    for v in range(n_vertices):
        it = items[ptr[v]:ptr[v + 1]]
        if not len(it):
            continue
        m = np.asarray(measure)[it]
        tot = math.fsum(m)
        for j in range(values.shape[1]):
            out[j, v] = math.fsum(m * values[it, j]) / tot
            scale[j, v] = np.abs(m * values[it, j]).sum() / tot
    return out, scale, ptr


# ---------------------------------------------------------------------------------------------- the cases of the two test files
CELL_MESHES = ["delaunay2d_12_cw", "hub2d_12_300", "hub3d_5_60", "delaunay3d_5_two_tag"]
FACET_MESHES = ["delaunay2d_12_cw", "hub2d_12_48m_cw", "delaunay3d_7"]
CELL_CASES = ["value", "grad_phi", "ion_flux", "ion_flux_degree3"]
FACET_CASES = ["value", "flux_dn", "flux_dn_degree3", "I_ch"]
DERIVATIVE_CASES = ("grad_phi", "ion_flux", "ion_flux_degree3", "flux_dn", "flux_dn_degree3")


def cell_forms(P, case):
    """(expr_i, expr_e, degree) of a cell-field case on a ``functionals_irregular.Prob``"""
    from cgx_hip import fem
    p = P.p
    forms = []
    for s in range(2):
        phi = p.wh[s][p.N_ions]
        if case == "value":                      # one output, values only
            forms.append(p.wh[s][2] * fem.exp(12.0 * phi) + P.user)
        elif case == "grad_phi":                 # dim outputs
            forms.append(list(fem.grad(phi)))
        else:                                    # the flux of ion 1: a gradient inside a product
            ion, c = p.ion_list[1], p.wh[s][1]
            D = ion["Di" if s == 0 else "De"]
            forms.append([-D * (fem.grad(c)[a] + (ion["z"] / p.psi) * c * fem.grad(phi)[a]) for a in range(P.dim)])
    return forms[0], forms[1], {"value": 3, "grad_phi": 1, "ion_flux": 1, "ion_flux_degree3": 3}[case]


def facet_forms(P, case):
    """(expr, degree) of a facet-field case"""
    from cgx_hip import fem
    p = P.p
    if case == "value":
        return P.user * p.phi_m_prev + p.wh[0][0], 2
    if case == "I_ch":                           # three outputs
        return [p.ion_list[j]["I_ch"][p.gamma_tags[0]] for j in range(3)], 2
    phi = p.wh[0][p.N_ions]                      # two outputs: the trans-membrane flux of two ions out of the intracellular cell
    outs = [-ion["Di"] * (fem.NormalDerivative(p.wh[0][j], "+") + (ion["z"] / p.psi) * p.wh[0][j] * fem.NormalDerivative(phi, "+"))
            for j, ion in enumerate(p.ion_list[:2])]
    return outs, 1 if case == "flux_dn" else 3


def emi_cell_forms(p):
    from cgx_hip import fem
    return [-p.sigma_i * g for g in fem.grad(p.wh[0])], [-p.sigma_e * g for g in fem.grad(p.wh[1])], 1


_FLOORS = {}


def cell_floor(P, case):
    if ("cell", P.name, case) not in _FLOORS:
        fi, fe, deg = cell_forms(P, case)
        _FLOORS[("cell", P.name, case)] = floor(lambda ld: cell_field(P.p, fi, fe, degree=deg, longdouble=ld)[2:])
    return _FLOORS[("cell", P.name, case)]


def facet_floor(P, case):
    if ("facet", P.name, case) not in _FLOORS:
        e, deg = facet_forms(P, case)
        _FLOORS[("facet", P.name, case)] = floor(lambda ld: facet_field(P.p, e, degree=deg, longdouble=ld)[1:])
    return _FLOORS[("facet", P.name, case)]


def floor_table():
    return [f"{kind:6s} {mesh:22s} {case:17s} floor {f:.2e}" for (kind, mesh, case), f in sorted(_FLOORS.items())]
