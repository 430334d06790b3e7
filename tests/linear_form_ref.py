"""NumPy fp64 reference of the linear forms (cgx_hip/linear_forms.py, csrc/knp_fields.inc): per item and local vertex a the element
vector ``meas sum_q q_w[q] lambda_a(q) f(x_q)``, and per vertex the sum of its entries.

Element vectors: the rule and the expressions as tests/derived_field_ref.py takes them (``fem.evaluate_numpy``, derivatives from the
simplex gradients with the differences first, the normal from the intracellular cell) with the weights ``q_w[q] lambda_a(q)`` in the
place of ``q_w[q]`` -- lambda_a(q) is the a-th barycentric coordinate of point q, positive at every point of the rules -- summed with
``math.fsum`` and multiplied with the measure; next to each its scale ``meas sum_q |q_w lambda_a f|``.  ``longdouble``: the geometry
(measures, gradients, normal) from ``functional_ref.geometry_longdouble``; the distance of the two over the scale is the rounding floor
of a case (``floor``), from which the GPU test takes ``functionals_irregular.tolerance``.

Gather: ``entries`` restates the builder of knp_scatter_create (per vertex the entries (i, a) that name it, ascending in i, kept as
i nv + a); ``gather`` adds every list (``math.fsum``: exact, so the order does not show) and the scales likewise."""
import math
import os

import numpy as np

import derived_field_ref as DR
import functional_ref
import membrane_functional_ref as mref


def cell_loads(coords, cells, exprs, qb, qw, longdouble=False):
    """(load [n, d + 1, n_out], scale [n, d + 1, n_out]) over the cells [n, d + 1]"""
    vol = functional_ref.cell_volumes(coords[cells], longdouble)
    parts = [DR.cell_means(coords, cells, exprs, qb, qw * qb[:, a], longdouble) for a in range(cells.shape[1])]
    return _with_measure(vol, parts)


def facet_loads(coords, fv, opp, meas, exprs, qp, qw, sides=None, longdouble=False):
    """(load [n, d, n_out], scale [n, d, n_out]) over the facets ``fv`` [n, d] of the measures ``meas`` (not read with ``longdouble``)"""
    if longdouble and len(fv):
        meas = mref.facet_measures_longdouble(coords, fv)
    parts = [DR.facet_means(coords, fv, opp, exprs, qp, qw * qp[:, a], sides, longdouble) for a in range(fv.shape[1])]
    return _with_measure(np.asarray(meas, dtype=np.float64), parts)


def _with_measure(meas, parts):
    load = np.stack([m for m, _ in parts], axis=1) * meas[:, None, None]
    scale = np.stack([s for _, s in parts], axis=1) * meas[:, None, None]
    return load, scale


def entries(n_vertices, item_vertices):
    """(ptr [n_vertices + 1], flat [n_entries]): per vertex its entries i nv + a with item_vertices[i, a] == v, ascending in i"""
    iv = np.asarray(item_vertices, dtype=np.int64)
    nv = iv.shape[1] if iv.ndim == 2 else 1
    ptr = np.zeros(n_vertices + 1, dtype=np.int64)
    np.add.at(ptr, iv.ravel() + 1, 1)
    np.cumsum(ptr, out=ptr)
    nxt, flat = ptr[:-1].copy(), np.zeros(ptr[-1], dtype=np.int64)
    for i, w in enumerate(iv):
        for a, v in enumerate(w):
            flat[nxt[v]] = i * nv + a
            nxt[v] += 1
    return ptr, flat


def gather(n_vertices, item_vertices, values):
    """(out [n_out, n_vertices], ptr): out[j][v] = sum over v's entries of values[i, a, j]; 0 for an empty list"""
    values = np.asarray(values, dtype=np.float64)
    n_out = values.shape[-1]
    flatv = values.reshape(-1, n_out)
    ptr, flat = entries(n_vertices, item_vertices)
    out = np.zeros((n_out, n_vertices))
    for v in range(n_vertices):
        e = flat[ptr[v]:ptr[v + 1]]
        for j in range(n_out):
            out[j, v] = math.fsum(flatv[e, j])
    return out, ptr


def _exprs(g):
    from cgx_hip import fem
    return [fem.as_expr(e) for e in (g if isinstance(g, (list, tuple)) else [g])]


def volume_form(problem, integrand_i=None, integrand_e=None, tags=None, degree=2, longdouble=False):
    """(vector [2, n_out, n_vertices], scale, touched [2, n_vertices]): what ``VolumeLinearForm`` returns, the scale of every entry and
    which vertices have a listed cell of the side"""
    from cgx_hip.functionals import quadrature
    p = problem
    lm = p.local_mesh
    nco, n_v = int(lm.n_cells_owned), lm.coords.shape[0]
    qb, qw = quadrature(lm.coords.shape[1], degree)
    side_tags = [[int(t) for t in p.intra_tags], [int(t) for t in np.ravel(p.extra_tag)]]
    ctags = np.asarray(lm.cell_tags[:nco])
    n_out = max(len(_exprs(g)) for g in (integrand_i, integrand_e) if g is not None)
    vec, scale, touched = np.zeros((2, n_out, n_v)), np.zeros((2, n_out, n_v)), np.zeros((2, n_v), dtype=bool)
    for s, g in enumerate((integrand_i, integrand_e)):
        if g is None:
            continue
        chosen = side_tags[s] if tags is None else [int(t) for t in tags if int(t) in side_tags[s]]
        cells = np.asarray(lm.cells)[np.nonzero(np.isin(ctags, chosen))[0]]
        if not len(cells):
            continue
        load, sc = cell_loads(lm.coords, cells, _exprs(g), qb, qw, longdouble)
        vec[s], ptr = gather(n_v, cells, load)
        scale[s], _ = gather(n_v, cells, sc)
        touched[s] = np.diff(ptr) > 0
    return vec, scale, touched


def membrane_facets(problem, tags=None):
    """the facets (indices into the gamma list, ascending) of the membrane tags or pooled groups ``tags``"""
    p = problem
    chosen = [int(t) for t in p.gamma_tags] if tags is None else [int(t) for g in tags for t in (g if isinstance(g, (list, tuple)) else [g])]
    return np.nonzero(np.isin(np.asarray(p.gamma_facet_tags), chosen))[0]


def membrane_form(problem, integrand, tags=None, degree=10, longdouble=False):
    """(vector [n_out, n_vertices], scale, touched [n_vertices]): what ``MembraneLinearForm`` returns"""
    from cgx_hip.mesh import facet_quadrature
    p = problem
    lm = p.local_mesh
    n_v = lm.coords.shape[0]
    qp, qw = facet_quadrature(lm.coords.shape[1], degree)
    idx = membrane_facets(p, tags)
    fv = np.asarray(p._fv)
    opp = mref.opposite_vertices(np.asarray(lm.cells), np.asarray(lm.gamma), fv)
    load, sc = facet_loads(lm.coords, fv[idx], opp[idx], np.asarray(p._fmeas)[idx], _exprs(integrand), np.asarray(qp), np.asarray(qw),
                           mref.default_sides(p), longdouble)
    vec, ptr = gather(n_v, fv[idx], load)
    scale, _ = gather(n_v, fv[idx], sc)
    return vec, scale, np.diff(ptr) > 0


def floor(ref):
    """``ref(longdouble)`` -> (vector, scale, touched): the largest |fp64 - long-double geometry| / scale over the entries of the
    touched vertices; a touched entry of scale 0 has the value 0 in both"""
    (v, s, on), (vl, _, _) = ref(False), ref(True)
    on = np.broadcast_to(on[..., None, :] if v.ndim == on.ndim + 1 else on, v.shape)
    assert on.any() and np.all(v[~on] == 0.0) and np.all(v[on & (s == 0)] == vl[on & (s == 0)])
    sel = on & (s > 0)
    return float(np.max(np.abs(v - vl)[sel] / s[sel]))


# ---------------------------------------------------------------------------------------------- the cases of the two test files
def volume_case(P, case):
    """(integrand_i, integrand_e, degree) of a ``functionals_irregular`` volume case as a linear form: the rule of the integrand's
    degree plus one for the test function"""
    import functionals_irregular as FI
    fi, fe, degree = FI.volume_forms(P, case)
    return fi, fe, degree + 1


def membrane_case(P, case):
    """(integrand, tags, degree) of a ``functionals_irregular`` membrane case as a linear form: the closed cases over the pooled group"""
    import functionals_irregular as FI
    outs, degree = FI.membrane_outs(P, case)
    return outs, (FI.closed_groups(P) if case in FI.CLOSED else None), degree + 1


_FLOORS = {}


def volume_floor(P, case):
    if ("volume", P.name, case) not in _FLOORS:
        fi, fe, deg = volume_case(P, case)
        _FLOORS[("volume", P.name, case)] = floor(lambda ld: volume_form(P.p, fi, fe, degree=deg, longdouble=ld))
    return _FLOORS[("volume", P.name, case)]


def membrane_floor(P, case):
    if ("membrane", P.name, case) not in _FLOORS:
        e, tags, deg = membrane_case(P, case)
        _FLOORS[("membrane", P.name, case)] = floor(lambda ld: membrane_form(P.p, e, tags, degree=deg, longdouble=ld))
    return _FLOORS[("membrane", P.name, case)]


def floor_table():
    import functionals_irregular as FI
    return [f"{kind:9s} {mesh:22s} {case:15s} floor {f:.2e}  tolerance {FI.tolerance(f):.2e}" for (kind, mesh, case), f in sorted(_FLOORS.items())]


# ---------------------------------------------------------------------------------------------- the step tests
def step_problems(tmp_path=None, steps=3):
    """the two problems of the step tests (shared with the GPU file): the tissue lattice with ``source_terms: ion_injection`` and
    the same lattice without it.  The CI square has no cell inside the reference's injection cube at N = 8, and from N = 10 on the
    cube lies inside its one cell, where the extracellular nodal source acts on no node; on the lattice the cube covers the gap
    between the four cells, so the nodal path really adds to the right-hand side."""
    from parity_utils import make_problem, tissue_config
    out = []
    for src in (True, False):
        cfg = tissue_config(2, 20, 2, steps=steps, rtol=1e-11, stimulus=False)
        cfg["quiet"] = True
        if tmp_path is not None:
            cfg["output_dir"] = str(tmp_path / ("nodal" if src else "form")) + os.sep
        if src:
            cfg["source_terms"] = "ion_injection"
        out.append(make_problem(cfg, "passive"))
    return out


def nodal_and_form(p, f):
    """per vertex the extracellular entries of the two formulas for a nodal source ``f``: (sum_b M_ab f_b with the mass matrix of
    ``functional_ref.mass_form``, the degree-2 form of tests/linear_form_ref.py, the scale sum_b |M_ab f_b|)"""
    import functionals_irregular as FI
    from cgx_hip import fem
    lm = p.local_mesh
    nco, d = int(lm.n_cells_owned), lm.coords.shape[1]
    cells = np.asarray(lm.cells)[:nco]
    cells = cells[np.isin(np.asarray(lm.cell_tags[:nco]), [int(t) for t in np.ravel(p.extra_tag)])]
    vol = functional_ref.cell_volumes(lm.coords[cells])
    M = (np.ones((d + 1, d + 1)) + np.eye(d + 1)) / ((d + 1) * (d + 2))
    terms = vol[:, None, None] * M[None] * f[cells][:, None, :]                  # [cell, a, b]
    nodal, scale = np.zeros(len(f)), np.zeros(len(f))
    ptr, flat = entries(len(f), cells)
    per_entry, abs_entry = terms.reshape(-1, d + 1), np.abs(terms).reshape(-1, d + 1)
    for v in range(len(f)):
        e = flat[ptr[v]:ptr[v + 1]]
        nodal[v], scale[v] = math.fsum(per_entry[e].ravel()), abs_entry[e].sum()
    fn = fem.Function(p.V, "f_copy")
    FI.write(fn, f)
    form = volume_form(p, None, fn, degree=2)[0][1, 0]
    return nodal, form, scale
