"""Independent fp64 NumPy evaluation of the trans-membrane molar ion fluxes (test infrastructure: the checker of
cgx_hip/fluxes.py and k_diag_fluxes).  Per selected membrane facet F with intracellular cell T+ and extracellular cell T-,

    flux[t][s][k] = sum_F -D_k |F| sum_q w_q m(x_q) (grad c_k^s . n_s + (z_k/psi) c_k^s(x_q) grad phi^s . n_s)

written from the definition: P1 gradients from the inverse of each cell's [1 x] vertex matrix, the normal from the facet's edge /
cross product oriented away from T+'s opposite vertex, an explicit loop over the quadrature points.  Nothing here is shared with
the library's per-facet records.  Besides the fluxes it returns, per entry, the magnitude sum

    S = sum_F D_k (W0 sum_a |g_a| |c_a| + |z_k/psi| (sum_b |W_b| |c_b|) (sum_a |g_a| |phi_a|))

that the tests scale their tolerance with (|gpu - ref| <= TOL * S): the gradient of a nearly constant field cancels, so a bound
has to follow |c| |grad lambda|, not the result.
"""
import numpy as np

TOL = 1e-12


def host_fields(p):
    """the nodal fields of a problem copied to the host"""
    n = p.N_ions
    return {"k_i": [p.wh[0][j].numpy().copy() for j in range(n)], "k_e": [p.wh[1][j].numpy().copy() for j in range(n)],
            "phi_i": p.wh[0][n].numpy().copy(), "phi_e": p.wh[1][n].numpy().copy()}


def coefficients(p):
    psi = float(p.psi.value)
    return (np.array([float(ion["Di"].value) for ion in p.ion_list]), np.array([float(ion["z"].value) / psi for ion in p.ion_list]))


def region_box(p):
    """the stimulus region as (axis, lo, hi) triples, straight from the problem's attributes; [] without one"""
    if not getattr(p, "stimulus_region", False):
        return []
    if p.multiple_stimulus_directions:
        return [(ax, float(p.stimulus_region_range[i][0]), float(p.stimulus_region_range[i][1]))
                for i, ax in enumerate(p.stimulus_region_directions)]
    return [(p.stimulus_region_direction, float(p.stimulus_region_range[0]), float(p.stimulus_region_range[1]))]


def _cell_gradients(X):
    """X [n, d+1, d] -> grad lambda_a [n, d+1, d] from the inverse of the [1 x] vertex matrix"""
    n, nv, d = X.shape
    A = np.concatenate([np.ones((n, nv, 1)), X], axis=2)     # row a: [1, x_a]; lambda_a(x) = [1 x] . inv[:, a]
    inv = np.linalg.inv(A)
    return np.transpose(inv[:, 1:, :], (0, 2, 1))


def flux_ref(p, fields, D, zpsi, groups, box=()):
    """Fluxes [n_groups, 2, n_ions], magnitude sums S of the same shape and, per group, the covered fraction sum_q w_q m_q of each
    of its facets.  ``groups``: lists of membrane tags, a facet goes to the first group listing its tag; this rank's facets only
    (owner of the facet's first vertex).  ``box``: (axis, lo, hi) triples, strict inequalities at the quadrature points."""
    lm = p.local_mesh
    coords, cells, gamma = np.asarray(lm.coords, dtype=np.float64), np.asarray(lm.cells), np.asarray(lm.gamma)
    d = coords.shape[1]
    lam, w = np.asarray(p.q_pts, dtype=np.float64), np.asarray(p.q_w, dtype=np.float64)
    n_ions = len(D)
    flux = np.zeros((len(groups), 2, n_ions))
    S = np.zeros_like(flux)
    cover = [np.zeros(0) for _ in groups]
    if gamma.shape[0] == 0:
        return flux, S, cover
    cp, lf, cm = gamma[:, 0], gamma[:, 1], gamma[:, 2]
    keep = np.arange(d + 1)[None, :] != lf[:, None]
    fv = cells[cp][keep].reshape(-1, d)                       # facet vertices in the order of T+'s vertex list
    opp = cells[cp][~keep]
    tags = np.asarray(lm.gamma_tags)
    owned = fv[:, 0] < lm.n_vertices_owned
    taken = np.zeros(len(tags), dtype=bool)
    for t, group in enumerate(groups):
        sel = np.nonzero(owned & np.isin(tags, list(group)) & ~taken)[0]
        taken[sel] = True
        if not len(sel):
            continue
        Xf = coords[fv[sel]]                                  # [n, d, d]
        if d == 2:
            e = Xf[:, 1] - Xf[:, 0]
            nrm = np.stack([e[:, 1], -e[:, 0]], axis=1)
            meas = np.linalg.norm(e, axis=1)
        else:
            nrm = np.cross(Xf[:, 1] - Xf[:, 0], Xf[:, 2] - Xf[:, 0])
            meas = 0.5 * np.linalg.norm(nrm, axis=1)
        nrm = nrm / np.linalg.norm(nrm, axis=1)[:, None]
        inward = np.einsum("nk,nk->n", nrm, coords[opp[sel]] - Xf[:, 0]) > 0
        nrm[inward] *= -1.0                                   # n_0: out of T+
        mq = np.ones((len(sel), len(w)))
        for q in range(len(w)):
            xq = np.einsum("b,nbk->nk", lam[q], Xf)
            for ax, lo, hi in box:
                mq[:, q] *= ((xq[:, ax] > lo) & (xq[:, ax] < hi))
        cover[t] = mq @ w
        W0 = meas * (mq @ w)
        Wb = meas[:, None] * np.einsum("nq,q,qb->nb", mq, w, lam)
        for s, (cell, sign, cs, ph) in enumerate(((cp[sel], 1.0, fields["k_i"], fields["phi_i"]),
                                                  (cm[sel], -1.0, fields["k_e"], fields["phi_e"]))):
            cv = cells[cell]                                  # [n, d+1]
            G = _cell_gradients(coords[cv])
            n_s = sign * nrm
            g = np.einsum("nak,nk->na", G, n_s)
            gphi = np.einsum("nak,na->nk", G, ph[cv])
            dphi_n = np.einsum("nk,nk->n", gphi, n_s)
            for k in range(n_ions):
                c = cs[k]
                dc_n = np.einsum("nk,nk->n", np.einsum("nak,na->nk", G, c[cv]), n_s)
                acc = np.zeros(len(sel))
                for q in range(len(w)):
                    cq = c[fv[sel]] @ lam[q]
                    acc += w[q] * mq[:, q] * (dc_n + zpsi[k] * cq * dphi_n)
                flux[t, s, k] = np.sum(-D[k] * meas * acc)
                S[t, s, k] = np.sum(D[k] * (W0 * np.sum(np.abs(g) * np.abs(c[cv]), axis=1)
                                            + abs(zpsi[k]) * np.sum(np.abs(Wb) * np.abs(c[fv[sel]]), axis=1)
                                            * np.sum(np.abs(g) * np.abs(ph[cv]), axis=1)))
    return flux, S, cover


def intra_volume(p):
    """volume of this rank's owned intracellular cells"""
    lm = p.local_mesh
    nco = int(lm.n_cells_owned)
    X = np.asarray(lm.coords)[np.asarray(lm.cells)[:nco]]
    d = X.shape[2]
    vol = np.abs(np.linalg.det(X[:, 1:, :] - X[:, :1, :])) / (2.0 if d == 2 else 6.0)
    return float(vol[np.asarray(p.cell_side)[:nco] == 0].sum())
