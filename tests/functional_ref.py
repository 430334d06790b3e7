"""NumPy reference of the volume functionals (cgx_hip/functionals.py, csrc/knp_functional.inc): the same quadrature rule, the
expressions through ``fem.evaluate_numpy``, derivatives from the cells' simplex gradients.  Besides the integrals it returns
sum |w f| per tag and output, the scale of the rounding error of any summation order: the tests hold the device to 1e-12 of it."""
import math

import numpy as np

TOL = 1e-12


def geometry_longdouble(X):
    """(G, det) of ``simplex_gradients`` and the edge determinant in ``np.longdouble``, unrounded: the inverse of the edge matrix by
    explicit cofactors (d = 2, 3), no LAPACK.  The more precise twin of the fp64 geometry: the difference of the two references is
    the rounding floor of any fp64 evaluation of the same geometry."""
    X = np.asarray(X, dtype=np.longdouble)
    E = X[:, 1:, :] - X[:, :1, :]
    d = E.shape[2]
    if d == 2:
        cof = np.stack([np.stack([E[:, 1, 1], -E[:, 1, 0]], axis=1), np.stack([-E[:, 0, 1], E[:, 0, 0]], axis=1)], axis=1)
        det = E[:, 0, 0] * E[:, 1, 1] - E[:, 0, 1] * E[:, 1, 0]
    else:
        cross = lambda u, w: np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                                       u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
        cof = np.stack([cross(E[:, 1], E[:, 2]), cross(E[:, 2], E[:, 0]), cross(E[:, 0], E[:, 1])], axis=1)
        det = (E[:, 0] * cof[:, 0]).sum(axis=1)
    G = np.empty_like(X)
    G[:, 1:, :] = cof / det[:, None, None]           # grad(lambda_{a+1}) = cofactor row a / det
    G[:, 0, :] = -G[:, 1:, :].sum(axis=1)
    return G, det


def simplex_gradients(X, longdouble=False):
    """X [n, d + 1, d] vertex coordinates -> G [n, d + 1, d], G[c, a] = grad(lambda_a) on cell c (``longdouble``: computed by
    ``geometry_longdouble`` and rounded to fp64 once)"""
    if longdouble:
        return geometry_longdouble(X)[0].astype(np.float64)
    E = X[:, 1:, :] - X[:, :1, :]                    # rows: edges from vertex 0; p - x0 = lambda[1:] @ E
    Einv = np.linalg.inv(E)                          # lambda_{a+1} = (p - x0) @ Einv[:, a]
    G = np.empty_like(X)
    G[:, 1:, :] = np.swapaxes(Einv, 1, 2)
    G[:, 0, :] = -G[:, 1:, :].sum(axis=1)
    return G


def cell_volumes(X, longdouble=False):
    d = X.shape[2]
    if longdouble:
        return (np.abs(geometry_longdouble(X)[1]) / math.factorial(d)).astype(np.float64)
    return np.abs(np.linalg.det(X[:, 1:, :] - X[:, :1, :])) / math.factorial(d)


def functions_of(e, found=None):
    from cgx_hip import fem
    found = [] if found is None else found
    e = fem.as_expr(e)
    if isinstance(e, fem.Function):
        found.append(e)
    elif isinstance(e, fem.Derivative):
        found.append(e.function)
    elif isinstance(e, fem.Op):
        for a in e.args:
            functions_of(a, found)
    return found


def integrate_cells(coords, cells, exprs, qb, qw, longdouble=False):
    """per expression: (sum, sum of absolute values) of |T| q_w f over the given cells [n, d + 1] and all points.  ``longdouble``: the
    volumes and the gradients of the barycentric coordinates come from ``geometry_longdouble``; everything else stays as it is."""
    from cgx_hip import fem
    X = coords[cells]
    d = X.shape[2]
    vol, G = cell_volumes(X, longdouble), simplex_gradients(X, longdouble)
    xq = np.einsum("qa,nak->nqk", qb, X)
    fields, grads = {}, {}
    for e in exprs:
        for f in functions_of(e):
            if id(f) in fields:
                continue
            fv = f.numpy()[cells]
            fields[id(f)] = np.einsum("qa,na->nq", qb, fv)
            for k in range(d):
                # sum_b grad(lambda_b) f_b with the differences f_b - f_0 taken first, as the kernel does (sum_b grad(lambda_b) = 0)
                grads[(id(f), k)] = np.broadcast_to((G[:, 1:, k] * (fv[:, 1:] - fv[:, :1])).sum(axis=1)[:, None], (len(cells), len(qw)))
    env = {"x": [xq[:, :, k] for k in range(d)], "fields": fields, "grads": grads}
    w = vol[:, None] * qw[None, :]
    out = []
    for e in exprs:
        wf = w * np.broadcast_to(fem.evaluate_numpy(e, env), w.shape)
        out.append((math.fsum(wf.ravel()), float(np.abs(wf).sum())))
    return out


def reference(problem, integrand_i=None, integrand_e=None, tags=None, degree=2, longdouble=False):
    """(tags, side, value [n_tags, n_out], scale [n_tags, n_out]): rows as ``VolumeFunctional`` orders them -- the intracellular
    tags first, each side's in the order given (``tags`` None: every tag of the sides that have an integrand)"""
    from cgx_hip.functionals import quadrature
    p = problem
    lm = p.local_mesh
    nco = int(lm.n_cells_owned)
    qb, qw = quadrature(lm.coords.shape[1], degree)
    side_tags = [[int(t) for t in p.intra_tags], [int(t) for t in np.ravel(p.extra_tag)]]
    rows_t, rows_s, val, scale = [], [], [], []
    for s, g in enumerate((integrand_i, integrand_e)):
        if g is None:
            continue
        exprs = list(g) if isinstance(g, (list, tuple)) else [g]
        for t in (side_tags[s] if tags is None else [int(t) for t in tags if int(t) in side_tags[s]]):
            c = lm.cells[:nco][np.asarray(lm.cell_tags[:nco]) == t]
            r = integrate_cells(lm.coords, c, exprs, qb, qw, longdouble)
            rows_t.append(t)
            rows_s.append(s)
            val.append([a for a, _ in r])
            scale.append([b for _, b in r])
    return np.array(rows_t), np.array(rows_s), np.array(val), np.array(scale)


def mass_form(coords, cells, u, v):
    """u^T M v with M_ab = |T| (1 + delta_ab) / ((d + 1)(d + 2)): (sum, sum of absolute values of the terms)"""
    X = coords[cells]
    d = X.shape[2]
    vol = cell_volumes(X)
    M = (np.ones((d + 1, d + 1)) + np.eye(d + 1)) / ((d + 1) * (d + 2))
    terms = vol[:, None, None] * M[None] * u[cells][:, :, None] * v[cells][:, None, :]
    return math.fsum(terms.ravel()), float(np.abs(terms).sum())


def stiffness_form(coords, cells, u, v):
    """u^T K v with K_ab = |T| grad(lambda_a) . grad(lambda_b): (sum, sum of absolute values of the terms)"""
    X = coords[cells]
    vol, G = cell_volumes(X), simplex_gradients(X)
    K = vol[:, None, None] * np.einsum("nak,nbk->nab", G, G)
    terms = K * u[cells][:, :, None] * v[cells][:, None, :]
    return math.fsum(terms.ravel()), float(np.abs(terms).sum())
