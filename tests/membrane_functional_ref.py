"""NumPy reference of the membrane functionals (cgx_hip/functionals.py, csrc/knp_membrane_functional.inc): the same facet rule, the
expressions through ``fem.evaluate_numpy``, one-sided derivatives from ``functional_ref.simplex_gradients`` on the two cells next to
a facet (differences first), the normal from the gradient of the intracellular cell's barycentric coordinate of its vertex off the
facet.  Besides the integrals it returns sum |w f| per row and output; the tests hold the device to ``functional_ref.TOL`` of it."""
import math

import numpy as np

from functional_ref import TOL, functions_of as _volume_functions_of, geometry_longdouble, simplex_gradients  # noqa: F401  (TOL is re-exported)


def functions_of(e, found=None):
    from cgx_hip import fem
    found = [] if found is None else found
    e = fem.as_expr(e)
    if isinstance(e, fem.NormalDerivative):
        found.append(e.function)
    elif isinstance(e, fem.Op):
        for a in e.args:
            functions_of(a, found)
    else:
        _volume_functions_of(e, found)
    return found


def opposite_vertices(cells, gamma, fv):
    """per membrane facet the vertex of the intracellular and of the extracellular cell that is not on the facet (-1: none)"""
    opp = np.full((len(fv), 2), -1, dtype=np.int64)
    for s, col in enumerate((0, 2)):
        cv = cells[gamma[:, col]]
        off = ~(cv[:, :, None] == fv[:, None, :]).any(axis=2)
        one = off.sum(axis=1) == 1
        opp[one, s] = cv[one][off[one]]
    return opp


def facet_measures_longdouble(coords, fv):
    """|F| of the facets ``fv`` [n, d] from their coordinates in ``np.longdouble`` (edge length / triangle area), rounded to fp64 once"""
    X = np.asarray(coords[fv], dtype=np.longdouble)
    e = X[:, 1:, :] - X[:, :1, :]
    if fv.shape[1] == 2:
        return np.sqrt((e[:, 0] ** 2).sum(axis=1)).astype(np.float64)
    u, w = e[:, 0], e[:, 1]
    c = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
    return (np.sqrt((c ** 2).sum(axis=1)) / 2).astype(np.float64)


def integrate_facets(coords, fv, opp, meas, exprs, qp, qw, sides=None, longdouble=False):
    """per expression: (sum, sum of absolute values) of |F| q_w f over the facets ``fv`` [n, d] with the opposite vertices ``opp``
    [n, 2] and the measures ``meas``.  ``sides``: {id(Function): 0 | 1}, the side an unrestricted derivative is taken on.
    ``longdouble``: the measures (``meas`` is not read), the gradients of the two cells and the normal are computed in
    ``np.longdouble`` (``functional_ref.geometry_longdouble``) and rounded to fp64 once; everything else stays as it is."""
    from cgx_hip import fem
    sides = sides or {}
    n, d = fv.shape
    Xf = coords[fv]
    xq = np.einsum("qa,nak->nqk", qp, Xf)
    bc = lambda a: np.broadcast_to(np.asarray(a)[:, None], (n, len(qw)))
    cellv, G = [], []
    for s in range(2):
        ok = n > 0 and np.all(opp[:, s] >= 0)
        cv = np.concatenate([fv, opp[:, s:s + 1]], axis=1) if ok else None
        cellv.append(cv)
        G.append(simplex_gradients(coords[cv], longdouble) if ok else None)
    nrm = None
    if G[0] is not None and longdouble:
        g = geometry_longdouble(coords[cellv[0]])[0][:, d, :]
        nrm = (-g / np.sqrt((g * g).sum(axis=1))[:, None]).astype(np.float64)
    elif G[0] is not None:
        g = G[0][:, d, :]
        nrm = -g / np.linalg.norm(g, axis=1)[:, None]
    if longdouble and n > 0:
        meas = facet_measures_longdouble(coords, fv)
    fields, grads, nds = {}, {}, {}
    for e in exprs:
        for f in functions_of(e):
            if id(f) in fields:
                continue
            val = f.numpy()
            fields[id(f)] = np.einsum("qa,na->nq", qp, val[fv])
            for s, r in enumerate("+-"):
                if G[s] is None or nrm is None:
                    continue
                fc = val[cellv[s]]
                diff = fc[:, 1:] - fc[:, :1]                  # differences first, as the kernel does
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
    w = meas[:, None] * qw[None, :]
    out = []
    for e in exprs:
        wf = w * np.broadcast_to(fem.evaluate_numpy(e, env), w.shape)
        out.append((math.fsum(wf.ravel()), float(np.abs(wf).sum())))
    return out


def default_sides(p):
    wh = [list(w) if isinstance(w, (list, tuple)) else [w] for w in p.wh]
    return {id(f): s for s in range(2) for f in wh[s]}


def reference(problem, integrand, tags=None, degree=10, longdouble=False):
    """(tags [rows], value [rows, n_out], scale [rows, n_out]): rows as ``MembraneFunctional`` orders them (``tags`` None: every tag of
    ``gamma_tags`` on its own; an entry may be a tuple of tags pooled into one row)"""
    from cgx_hip.diagnostics import facet_group_map
    from cgx_hip.mesh import facet_quadrature
    p = problem
    lm = p.local_mesh
    d = lm.coords.shape[1]
    qp, qw = facet_quadrature(d, degree)
    exprs = list(integrand) if isinstance(integrand, (list, tuple)) else [integrand]
    groups = [(int(t),) for t in p.gamma_tags] if tags is None else [tuple(int(t) for t in g) if isinstance(g, (list, tuple)) else (int(g),)
                                                                    for g in tags]
    seg_ptr, facets = facet_group_map(p, groups)
    fv = np.asarray(p._fv)
    opp = opposite_vertices(np.asarray(lm.cells), np.asarray(lm.gamma), fv)
    sides = default_sides(p)
    val, scale = [], []
    for t in range(len(groups)):
        sel = facets[seg_ptr[t]:seg_ptr[t + 1]]
        r = integrate_facets(lm.coords, fv[sel], opp[sel], p._fmeas[sel], exprs, qp, qw, sides, longdouble)
        val.append([a for a, _ in r])
        scale.append([b for _, b in r])
    return np.array([g[0] for g in groups]), np.array(val), np.array(scale)
