"""Independent fp64 NumPy evaluation of the per-tag membrane-potential reduction (test infrastructure: the checker of
k_diag_phim in csrc/knp_diagnostics.inc and ``ProblemKNPEMI.membrane_potential``).  Written from the definition, with an explicit
loop over the groups and their facets; the facets' vertices and measures come from the mesh's cells and coordinates, not from the
problem's facet tables.  For each group t of membrane tags, with d the number of facet vertices and phi the nodal phi_m,

    I_t = sum_F |F| (1/d) sum_a phi(v_a(F))      A_t = sum_F |F|      min_t / max_t over all vertices of the group's facets

over this rank's facets (the owner of the facet's first vertex counts it; a facet goes to the first group that lists its tag).
Besides these it returns the magnitude sum S_t = sum_F |F|/d sum_a |phi(v_a)| that the tests scale the integral's tolerance with
(|I_gpu - I_ref| <= TOL * S_t: the two differ by summation order only, and the signed values cancel), and per group the indices
(rows of the mesh's gamma list) of the facets it covered.  A group without facets gives I = A = S = 0, min = +inf, max = -inf.
"""
import math

import numpy as np

TOL = 1e-12


def facet_vertices(p):
    """vertices of every membrane facet [n_gamma, d], in the order of the intracellular cell's vertex list"""
    lm = p.local_mesh
    cells, gamma = np.asarray(lm.cells), np.asarray(lm.gamma)
    d = np.asarray(lm.coords).shape[1]
    if gamma.shape[0] == 0:
        return np.zeros((0, d), dtype=np.int64)
    keep = np.arange(d + 1)[None, :] != gamma[:, 1][:, None]
    return cells[gamma[:, 0]][keep].reshape(-1, d)


def facet_measure(x):
    """length of a segment / area of a triangle from its vertex coordinates [d, d]"""
    if x.shape[0] == 2:
        return math.hypot(*(x[1] - x[0]))
    n = np.cross(x[1] - x[0], x[2] - x[0])
    return 0.5 * math.sqrt(float(n @ n))


def phim_ref(p, phi, groups):
    """``phi``: nodal phi_m on the host.  Returns I, A, min, max, S (float64 [n_groups]) and the covered facet indices per group."""
    lm = p.local_mesh
    coords = np.asarray(lm.coords, dtype=np.float64)
    phi = np.asarray(phi, dtype=np.float64)
    fv = facet_vertices(p)
    tags = np.asarray(lm.gamma_tags)
    d = coords.shape[1]
    n = len(groups)
    I, A, S = np.zeros(n), np.zeros(n), np.zeros(n)
    lo, hi = np.full(n, np.inf), np.full(n, -np.inf)
    cover = []
    first = {}                                   # membrane tag -> the first group that lists it
    for t, group in enumerate(groups):
        for g in group:
            first.setdefault(int(g), t)
    group_of = np.array([first.get(int(g), -1) for g in tags], dtype=np.int64)
    for t in range(n):
        mine = []
        for F in np.nonzero(group_of == t)[0]:
            if fv[F, 0] >= lm.n_vertices_owned:
                continue
            mine.append(F)
            meas = facet_measure(coords[fv[F]])
            vals = [float(phi[v]) for v in fv[F]]
            I[t] += meas / d * math.fsum(vals)
            S[t] += meas / d * math.fsum(abs(v) for v in vals)
            A[t] += meas
            lo[t] = min([lo[t]] + vals)
            hi[t] = max([hi[t]] + vals)
        cover.append(np.array(mine, dtype=np.int64))
    return I, A, lo, hi, S, cover
