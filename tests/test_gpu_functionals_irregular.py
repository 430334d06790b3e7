"""The two functional kernels (csrc/knp_functional.inc, csrc/knp_membrane_functional.inc) on the irregular meshes of
tests/irregular_meshes.py and at their limits; tests/test_gpu_functionals.py and tests/test_gpu_membrane_functionals.py run them on
generated grids only: one cell volume, one facet measure, right-angled cells of one orientation, axis-aligned normals.  Here cells of
both orientations (in 2D through the reoriented ``_cw`` meshes: the det < 0 branch of every 2D kernel), every local facet index on both
sides, edge matrices of condition up to 234, facet measures over a factor of 55; tag maps cut at the edges of the 128-item blocks; the
largest rules (125 points) and a program on all 48 registers.  The inputs are pinned by tests/test_functionals_irregular_host.py.

Tolerances: |device - reference| <= tol * sum |w f| per row and output.  tol is ``functional_ref.TOL`` (1e-12) for integrands of values
only, and ``max(TOL, 8 * floor)`` for a case that reads a derivative or the normal, the floor being the distance of the fp64 reference
from its long-double-geometry twin on that mesh (tests/functionals_irregular.py; printed here and by the host test: every floor is
below 1e-15, so every tolerance is 1e-12).

Clockwise invariance: the rule is a collapsed Gauss-Jacobi rule and not symmetric under a permutation of a cell's vertices, so only
integrands it integrates exactly (1, u v, grad u . grad v) agree between a ``_cw`` mesh and its parent to TOL; for the nonlinear mix
the two orientations differ by the quadrature error (4e-3, host test), and the device's difference is held to the reference's."""
import math

import numpy as np
import pytest

import functional_ref
import functionals_irregular as FI
import irregular_meshes as IM
import membrane_functional_ref as mref
from functional_raw import RawMembrane, RawVolume
from functional_ref import TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probs(tmp_path_factory):
    """one problem with its backend per mesh, random fields; shared by the tests, none of which writes a field"""
    cache = {}
    tmp = tmp_path_factory.mktemp("functionals_irregular")

    def get(name):
        if name not in cache:
            cache[name] = FI.Prob(tmp, name, backend=True)
        return cache[name]
    return get


def _check(got, want, scale, what, tol=TOL, slack=0.0):
    got, want, scale = (np.asarray(a, dtype=np.float64) for a in (got, want, scale))
    err = np.abs(got - want)
    print(f"{what}: max |device - host| / sum|w f| = {np.max(err / np.maximum(scale, 1e-300)):.3e} (tol {tol:.1e}, slack {np.max(slack):.1e})")
    assert got.shape == want.shape and np.all(np.isfinite(got))
    assert np.all(err <= tol * scale + slack), (what, err, tol * scale + slack)


def _tag_cells(p, tag):
    lm = p.local_mesh
    nco = int(lm.n_cells_owned)
    return lm.cells[:nco][np.asarray(lm.cell_tags[:nco]) == tag]


# ================================================================================================ the volume kind
@pytest.mark.parametrize("name", FI.VOLUME_MESHES)
def test_volume_closed_forms(probs, name):
    from cgx_hip import fem
    from cgx_hip.functionals import VolumeFunctional
    P = probs(name)
    p, be = P.p, P.be
    coords = p.local_mesh.coords
    F = VolumeFunctional(p, 1.0, 1.0)
    lay = be.budget_layout()
    assert np.array_equal(F.tags, lay.tags)
    if name == FI.TWO_TAG:
        assert list(F.tags) == [2, 3, 1]
    vol = np.array([math.fsum(functional_ref.cell_volumes(coords[_tag_cells(p, t)])) for t in F.tags])
    assert np.all(vol > 0)
    _check(F.value()[:, 0], vol, vol, f"{name}: integrand 1 against the volumes")
    fi, fe, degree = FI.volume_forms(P, "mass_stiffness")
    tol = FI.tolerance(FI.volume_floor(P, "mass_stiffness"))
    print(f"{name}: floor {FI.volume_floor(P, 'mass_stiffness'):.2e}")
    M = VolumeFunctional(p, fi, fe, degree=degree)
    got = M.value()
    tags, side, want_ref, scale = functional_ref.reference(p, fi, fe, degree=degree)
    assert np.array_equal(tags, M.tags)
    want = np.array([[functional_ref.mass_form(coords, _tag_cells(p, t), p.wh[s][0].numpy(), p.wh[s][3].numpy())[0],
                      functional_ref.stiffness_form(coords, _tag_cells(p, t), p.wh[s][0].numpy(), p.wh[s][3].numpy())[0]]
                     for t, s in zip(tags, side)])
    assert np.abs(want).min() > 0
    _check(got[:, 0], want[:, 0], scale[:, 0], f"{name}: u^T M v")
    _check(got[:, 1], want[:, 1], scale[:, 1], f"{name}: u^T K v", tol)
    _check(got, want_ref, scale, f"{name}: both against the reference", tol)
    # a constant field under grad: the kernel takes the differences of the vertex values first, so every row is exactly zero
    Z = VolumeFunctional(p, [fem.grad(P.const)[0] * p.wh[0][0], fem.inner(fem.grad(P.const), fem.grad(P.user))],
                         [fem.grad(P.const)[0] * p.wh[1][0], fem.inner(fem.grad(P.const), fem.grad(P.user))])
    z = Z.value()
    assert z.shape == (len(F.tags), 2) and np.all(z == 0.0), z


@pytest.mark.parametrize("name", FI.VOLUME_MESHES)
def test_volume_nonlinear_integrands(probs, name):
    from cgx_hip.functionals import VolumeFunctional
    P = probs(name)
    p = P.p
    P.amp.value = 0.25
    floor = FI.volume_floor(P, "nonlinear")
    tol = FI.tolerance(floor)
    print(f"{name}: floor {floor:.2e}")
    fi, fe, degree = FI.volume_forms(P, "nonlinear")
    F = VolumeFunctional(p, fi, fe, degree=degree)
    assert F.n_out == 3 and F.spec.q_w.shape[0] == 3 ** P.dim
    for sp in F.spec.sides:
        assert set(range(P.dim)) <= set(sp.spec.aux_derivs) and -1 in sp.spec.aux_derivs      # a derivative slot per axis
    try:
        for value in (0.25, -1.75):
            P.amp.value = value
            _, _, want, scale = functional_ref.reference(p, fi, fe, degree=degree)
            assert np.abs(want).min() > 0
            _check(F.value(), want, scale, f"{name}: nonlinear integrands, amplitude {value}", tol)
    finally:
        P.amp.value = 0.25


@pytest.mark.parametrize("name", FI.CW)
def test_clockwise_cells_give_the_counter_clockwise_integrals(probs, name):
    from cgx_hip.functionals import VolumeFunctional
    P, P0 = probs(name), probs(IM.PARENT[name])
    assert np.array_equal(P.user.numpy(), P0.user.numpy()) and not np.array_equal(P.p.local_mesh.cells, P0.p.local_mesh.cells)
    got = {}
    for Q in (P, P0):
        Q.amp.value = 0.25
        fi, fe, degree = FI.volume_forms(Q, "mass_stiffness")
        one = VolumeFunctional(Q.p, 1.0, 1.0)
        ms = VolumeFunctional(Q.p, fi, fe, degree=degree)
        ni, ne, nd = FI.volume_forms(Q, "nonlinear")
        nl = VolumeFunctional(Q.p, ni, ne, degree=nd)
        got[Q.name] = (one.tags, one.value(), ms.value(), nl.value(), functional_ref.reference(Q.p, fi, fe, degree=degree)[3],
                       functional_ref.reference(Q.p, ni, ne, degree=nd)[2:])
    a, b = got[P.name], got[P0.name]
    assert np.array_equal(a[0], b[0])
    _check(a[1][:, 0], b[1][:, 0], np.abs(b[1][:, 0]), f"{name}: integrand 1, cw against ccw")
    _check(a[2], b[2], b[4], f"{name}: u v and grad u . grad v, cw against ccw")
    # not exact for the rule: the orientations differ by the quadrature error, the device's difference is the reference's
    tol = FI.tolerance(max(FI.volume_floor(P, "nonlinear"), FI.volume_floor(P0, "nonlinear")))
    (ra, sa), (rb, _) = a[5], b[5]
    print(f"{name}: nonlinear mix, cw - ccw: device {np.max(np.abs(a[3] - b[3]) / sa):.3e}, reference {np.max(np.abs(ra - rb) / sa):.3e}")
    _check(a[3] - b[3], ra - rb, sa, f"{name}: nonlinear mix, (cw - ccw) against the reference's", 2.0 * tol)


@pytest.mark.parametrize("name,degree,powers,n_q", [("delaunay3d_5", 9, (3, 3, 3), 125), ("delaunay2d_12_cw", 21, (11, 10), 121)])
def test_volume_rule_limit(probs, name, degree, powers, n_q):
    """the largest rule the header admits (KNP_FUNCTIONAL_MAX_Q = 125 points), one monomial of full degree"""
    from cgx_hip import fem
    from cgx_hip.functionals import VolumeFunctional
    P = probs(name)
    p = P.p
    x = fem.SpatialCoordinate(p.mesh)
    mono = x[0] ** powers[0]
    for k in range(1, P.dim):
        mono = mono * x[k] ** powers[k]
    F = VolumeFunctional(p, mono, mono, degree=degree)
    assert F.spec.q_w.shape[0] == n_q and sum(powers) == degree
    got = F.value()
    _, _, want, scale = functional_ref.reference(p, mono, mono, degree=degree)
    _check(got, want, scale, f"{name}: x^{powers} with {n_q} points, per tag")
    lo, hi = p.local_mesh.coords.min(axis=0), p.local_mesh.coords.max(axis=0)
    assert np.all(lo == 0.0)
    closed = float(np.prod([hi[k] ** (e + 1) / (e + 1) for k, e in enumerate(powers)]))
    print(f"{name}: sum over the tags / closed form - 1 = {got.sum() / closed - 1.0:.3e}")
    assert abs(got.sum() - closed) <= TOL * scale.sum()


# ================================================================================================ the membrane kind
def _facet_rows(p, groups):
    from cgx_hip.diagnostics import facet_group_map
    seg_ptr, facets = facet_group_map(p, groups)
    return [facets[seg_ptr[t]:seg_ptr[t + 1]] for t in range(len(groups))]


@pytest.mark.parametrize("name", FI.MEMBRANE_MESHES)
def test_membrane_closed_forms(probs, name):
    from cgx_hip.functionals import MembraneFunctional
    P = probs(name)
    p = P.p
    lm = p.local_mesh
    F = MembraneFunctional(p, 1.0)
    each = [(int(t),) for t in p.gamma_tags]
    area = np.array([math.fsum(np.asarray(p._fmeas)[r]) for r in _facet_rows(p, each)])
    assert len(area) == (2 if name == FI.TWO_TAG else 1) and np.all(area > 0)
    _check(F.value()[:, 0], area, area, f"{name}: integrand 1 against the facet measures")
    groups = FI.closed_groups(P)
    outs, degree = FI.membrane_outs(P, "x_dot_n")
    floor = FI.membrane_floor(P, "x_dot_n")
    X = MembraneFunctional(p, outs, tags=groups, degree=degree)
    got = X.value()
    want_ref, scale = FI.membrane_reference(P, "x_dot_n")
    vol = functional_ref.cell_volumes(lm.coords[lm.cells])
    want = P.dim * math.fsum(vol[np.isin(lm.cell_tags, [int(t) for t in p.intra_tags])])
    print(f"{name}: floors x.n {floor:.2e}, normal {FI.membrane_floor(P, 'normal'):.2e}")
    assert got.shape == (1, 2) and want > 0
    _check(got[:, 0], [want], scale[:, 0], f"{name}: x . n('+') against dim * volume", FI.tolerance(floor))
    _check(got[:, 1], [-want], scale[:, 1], f"{name}: x . n('-')", FI.tolerance(floor))
    _check(got, want_ref, scale, f"{name}: x . n against the reference", FI.tolerance(floor))
    outs, degree = FI.membrane_outs(P, "normal")
    N = MembraneFunctional(p, outs, tags=groups, degree=degree)
    _, scale = FI.membrane_reference(P, "normal")
    _check(N.value(), np.zeros((1, P.dim)), scale, f"{name}: the normal's components over the closed membrane",
           FI.tolerance(FI.membrane_floor(P, "normal")))


@pytest.mark.parametrize("name", FI.MEMBRANE_MESHES)
def test_membrane_affine_field_with_a_large_offset(probs, name):
    """f = a . x + 1000 with a . x of order one: the offset cancels in the kernel's differences.  Against the closed forms the nodal
    values' own rounding (2^-44 each, amplified by the gradients of the barycentric coordinates) is allowed for by
    ``nodal_rounding_bounds``; against the reference, which reads the same rounded values, the plain tolerance holds."""
    from cgx_hip.functionals import MembraneFunctional
    P = probs(name)
    p = P.p
    groups = FI.closed_groups(P)
    area = math.fsum(np.asarray(p._fmeas))
    B = FI.nodal_rounding_bounds(P)
    for s, case in enumerate(("affine_plus", "affine_minus")):
        outs, degree = FI.membrane_outs(P, case)
        tol = FI.tolerance(FI.membrane_floor(P, case))
        got = MembraneFunctional(p, outs, tags=groups, degree=degree).value()
        want, scale = FI.membrane_reference(P, case)
        _check(got, want, scale, f"{name}: {case} against the reference", tol)
        _check(got[0], P.slope * area, scale[0], f"{name}: {case} against a x area", tol, B[s])
    tol = FI.tolerance(FI.membrane_floor(P, "affine_dn"))
    got = MembraneFunctional(p, FI.affine_dn_device(P), tags=groups, degree=1).value()
    want, scale = FI.membrane_reference(P, "affine_dn")
    assert np.all(scale > 0)
    _check(got[:, 0], want[:, 0], scale[:, 0], f"{name}: df/dn('+') against the reference", tol)
    _check(got[:, 0], [0.0], scale[:, 0], f"{name}: df/dn('+') over the closed membrane", tol, B[0])
    _check(got[:, 1], [0.0], scale[:, 0] + scale[:, 1], f"{name}: df/dn('+') + df/dn('-')", tol, B[0] + B[1])
    _check(got[:, 2], [0.0], 2.0 * scale[:, 0], f"{name}: dot(grad('+'), n('-')) + df/dn('+')", tol, 2.0 * B[0])


@pytest.mark.parametrize("name", FI.MEMBRANE_MESHES)
def test_membrane_random_fields_in_every_slot_mode(probs, name):
    """Every slot mode of the mesh's dimension: 3 dim + 4 of them, and a plan has 8 aux slots, so two functionals of three outputs
    at degree 4: the value, d/dx_a on the '+' cell, d/dn('+') and the normal in one, d/dx_a on the '-' cell and d/dn('-') in the other"""
    from cgx_hip.functionals import MembraneFunctional
    P = probs(name)
    p, dim = P.p, P.dim
    seen = set()
    for case in ("random_plus", "random_minus"):
        outs, degree = FI.membrane_outs(P, case)
        floor = FI.membrane_floor(P, case)
        F = MembraneFunctional(p, outs, degree=degree)
        seen |= set(F.spec.spec.aux_derivs)
        assert F.n_out == 3 and degree == 4
        want, scale = FI.membrane_reference(P, case)
        assert np.abs(want).min() > 0
        print(f"{name}: {case} floor {floor:.2e}, modes {sorted(F.spec.spec.aux_derivs)}")
        _check(F.value(), want, scale, f"{name}: {case}", FI.tolerance(floor))
    assert seen >= {-1, 6, 7} | set(range(dim)) | set(range(3, 3 + dim)) | set(range(8, 8 + dim)), seen


@pytest.mark.parametrize("name", FI.MEMBRANE_MESHES)
def test_membrane_functionals_against_the_hard_wired_kernels(probs, name):
    """the six flux integrands against knp_diag_membrane_fluxes and phi_m against knp_diag_membrane_potential, with the tolerance of
    tests/test_gpu_membrane_functionals.py"""
    from cgx_hip.functionals import MembraneFunctional
    P = probs(name)
    p = P.p
    hard = p.membrane_fluxes()
    for case, key in (("flux_i", "flux_i"), ("flux_e", "flux_e")):
        outs, degree = FI.membrane_outs(P, case)
        F = MembraneFunctional(p, outs)
        assert F.degree == degree
        got = F.value()
        tags, want, scale = mref.reference(p, outs)
        assert np.array_equal(tags, hard["tag"]) and np.abs(want).min() > 0
        _check(got, hard[key], scale, f"{name}: {key} against knp_diag_membrane_fluxes")
        _check(got, want, scale, f"{name}: {key} against the reference", FI.tolerance(FI.membrane_floor(P, case)))
    F = MembraneFunctional(p, p.phi_m_prev, degree=1)
    got = F.value()[:, 0]
    pot = p.membrane_potential()
    _, _, scale = mref.reference(p, p.phi_m_prev, degree=1)
    assert np.array_equal(pot["tag"], F.tags)
    _check(got, pot["mean"] * pot["area"], scale[:, 0], f"{name}: phi_m against mean x area of knp_diag_membrane_potential")


def test_emi_on_the_membrane_hub(tmp_path):
    """ProblemEMI on hub3d_5_60m: 17 facets at the hub, facet measures over a factor of 55"""
    from cgx_hip.functionals import MembraneFunctional
    p = FI.emi_problem(tmp_path, backend=True)
    meas = np.asarray(p._fmeas)
    assert meas.max() / meas.min() > 50.0
    outs = FI.emi_outs(p)
    floor = FI.emi_floor(p)
    F = MembraneFunctional(p, outs)
    assert sorted(F.spec.spec.aux_derivs) == [-1, -1, -1, -1, 6, 7]
    _, want, scale = mref.reference(p, outs)
    assert want.shape == (1, 3) and np.abs(want).min() > 0
    print(f"hub3d_5_60m: floor {floor:.2e}")
    _check(F.value(), want, scale, "hub3d_5_60m: EMI trans-membrane current", FI.tolerance(floor))
    area = math.fsum(meas)
    _check(MembraneFunctional(p, 1.0).value()[:, 0], [area], [area], "hub3d_5_60m: integrand 1 against the areas")


# ================================================================================================ block edges, through the raw ABI
def _two_output_program():
    """OUT_0 = aux_0 ^ 2, OUT_1 = 1 (constant 0)"""
    from cgx_hip._lib import OPS
    return dict(code=np.array([[OPS["AUX"], 0, 0, 0], [OPS["MUL"], 1, 0, 0], [OPS["OUT"], 0, 0, 1], [OPS["CONST"], 2, 0, 0],
                               [OPS["OUT"], 0, 1, 2]], dtype=np.int32), n_instr=5, n_consts=1, consts=np.array([1.0]), n_out=2)


class _Edge:
    """one kind on one mesh: the raw helper, the fields, and the reference of a list of items"""

    def __init__(self, P, kind):
        from cgx_hip import _lib
        p = P.p
        lm = p.local_mesh
        self.P, self.kind = P, kind
        self.fields = _lib.Fields()
        self.fields.aux[0] = P.user.data_ptr()
        if kind == "cells":
            self.n_items = int(lm.n_cells_owned)
            self.raw = RawVolume(P.be, self.n_items, P.dim)
            self.rule = (self.raw.args["q_bary"], self.raw.args["q_w"])
        else:
            self.fv = np.asarray(p._fv)
            self.n_items = len(self.fv)
            self.raw = RawMembrane(P.be, self.n_items, P.dim)
            self.rule = (self.raw.args["q_pts"], self.raw.args["q_w"])
            self.opp = mref.opposite_vertices(np.asarray(lm.cells), np.asarray(lm.gamma), self.fv)

    def reference(self, items, exprs, rule=None):
        lm = self.P.p.local_mesh
        qp, qw = rule or self.rule
        if self.kind == "cells":
            return functional_ref.integrate_cells(lm.coords, lm.cells[items], exprs, qp, qw)
        return mref.integrate_facets(lm.coords, self.fv[items], self.opp[items], np.asarray(self.P.p._fmeas)[items], exprs, qp, qw)

    def rows(self, seg_ptr, items):
        """[n_tags, 2] reference and scale of (user^2, 1); empty tags are zero"""
        want, scale = np.zeros((len(seg_ptr) - 1, 2)), np.zeros((len(seg_ptr) - 1, 2))
        for t in range(len(seg_ptr) - 1):
            sel = items[seg_ptr[t]:seg_ptr[t + 1]]
            if sel.size:
                r = self.reference(sel, [self.P.user * self.P.user, 1.0])
                want[t], scale[t] = [a for a, _ in r], [b for _, b in r]
        return want, scale

    def plan(self, seg_ptr, items, **kw):
        rc, fid = self.raw.create(n_tags=len(seg_ptr) - 1, seg_ptr=np.ascontiguousarray(seg_ptr, dtype=np.int32),
                                  **{self.raw.ITEMS: np.ascontiguousarray(items, dtype=np.int32)}, **kw)
        assert rc == 0, self.raw.error()
        return fid

    def eval(self, fid, n_rows, n_out):
        rc, out = self.raw.eval(fid, self.fields, n_rows, n_out)
        assert rc == 0, self.raw.error()
        return out


@pytest.fixture(scope="module")
def edges(probs):
    cache = {}

    def get(kind, name):
        if (kind, name) not in cache:
            cache[(kind, name)] = _Edge(probs(name), kind)
        return cache[(kind, name)]
    return get


EDGE_CASES = [("cells", m, s) for m in ("delaunay2d_12_cw", "delaunay3d_5") for s in FI.SEG_PTRS] + \
             [("facets", m, s) for m in ("delaunay3d_7", "delaunay2d_92") for s in FI.SEG_PTRS if s != "n257"]


@pytest.mark.parametrize("kind,name,seg", EDGE_CASES)
def test_tag_maps_at_the_block_edges(edges, kind, name, seg):
    """fn_lane / diag_chunk_partials at FN_BT = 128: tags that end on item 127, start on item 128, hold one item at the edge, are
    empty, or leave all but one lane of the last block idle.  The second output integrates 1: the rows' measures."""
    E = edges(kind, name)
    seg_ptr = FI.seg_ptr_for(seg, E.n_items)
    n, n_tags = int(seg_ptr[-1]), len(seg_ptr) - 1
    rng = np.random.default_rng(sum(map(ord, kind + name + seg)))
    items = rng.permutation(E.n_items)[:n].astype(np.int32)      # a random selection in random order
    prog = _two_output_program()
    fid = E.plan(seg_ptr, items, **prog)
    # a second live plan with another map: its scratch is its own
    other_ptr = np.array([0, min(130, E.n_items - 1), E.n_items - 1], dtype=np.int32)
    other_items = rng.permutation(E.n_items)[:E.n_items - 1].astype(np.int32)
    other = E.plan(other_ptr, other_items, **prog)
    try:
        got = E.eval(fid, n_tags, 2)
        between = E.eval(other, 2, 2)
        again = E.eval(fid, n_tags, 2)
        want, scale = E.rows(seg_ptr, items)
        empty = np.diff(seg_ptr) == 0
        print(f"{kind} {name} {seg}: seg_ptr {seg_ptr.tolist() if n_tags < 10 else '64 x 1 + 65'}, {empty.sum()} empty tags")
        assert np.all(got[empty] == 0.0) and np.all(scale[~empty] > 0)
        _check(got, want, scale, f"{kind} {name} {seg}")
        assert again.tobytes() == got.tobytes()
        w2, s2 = E.rows(other_ptr, other_items)
        _check(between, w2, s2, f"{kind} {name} {seg}: the plan evaluated in between")
    finally:
        assert E.raw.destroy(fid) == 0 and E.raw.destroy(other) == 0


# ================================================================================================ the register limit
def _register_programs():
    """aux_0 into register 47, moved down through every register to 0, then OUT_0 = r0^2, OUT_1 = r0, OUT_2 = 1; and the same
    arithmetic on registers 0..2"""
    from cgx_hip import _lib
    from cgx_hip._lib import OPS
    top = _lib.KNP_MAX_PROG_REGS - 1
    tail = [[OPS["MUL"], 1, 0, 0], [OPS["OUT"], 0, 0, 1], [OPS["OUT"], 0, 1, 0], [OPS["CONST"], 2, 0, 0], [OPS["OUT"], 0, 2, 2]]
    chain = [[OPS["AUX"], top, 0, 0]] + [[OPS["MOV"], r, r + 1, 0] for r in range(top - 1, -1, -1)] + tail
    short = [[OPS["AUX"], 0, 0, 0]] + tail
    mk = lambda rows: dict(code=np.array(rows, dtype=np.int32), n_instr=len(rows), n_consts=1, consts=np.array([1.0]), n_out=3)
    return mk(chain), mk(short)


@pytest.mark.parametrize("kind,name", [("cells", "delaunay3d_5"), ("facets", "delaunay3d_7")])
def test_forty_eight_registers_and_125_points(edges, kind, name):
    """KNP_MAX_PROG_REGS = 48 registers are 48 KiB of dynamic LDS next to up to 4 KiB of static LDS, with KNP_FUNCTIONAL_MAX_Q = 125
    points and three outputs: create and eval return 0, the values are the reference's and those of the program on three registers"""
    from cgx_hip import _lib
    from cgx_hip.functionals import quadrature
    from cgx_hip.mesh import facet_quadrature
    E = edges(kind, name)
    if kind == "cells":
        qp, qw = quadrature(3, 9)
        rule = dict(q_bary=qp, q_w=qw)
    else:      # the largest facet rule has 11 x 11 points: four more of weight zero at the centroid
        qp, qw = facet_quadrature(3, 20)
        qp = np.ascontiguousarray(np.vstack([qp, np.full((4, 3), 1.0 / 3.0)]))
        qw = np.ascontiguousarray(np.r_[qw, np.zeros(4)])
        rule = dict(q_pts=qp, q_w=qw)
    assert len(qw) == _lib.KNP_FUNCTIONAL_MAX_Q == 125
    chain, short = _register_programs()
    assert chain["code"][:, 1:].max() == 47 and set(chain["code"][:48, 1]) == set(range(48)) and short["code"][:, 1:].max() == 2
    seg_ptr, items = np.array([0, E.n_items], dtype=np.int32), np.arange(E.n_items, dtype=np.int32)
    big = E.plan(seg_ptr, items, n_q=125, **rule, **chain)
    small = E.plan(seg_ptr, items, n_q=125, **rule, **short)
    try:
        got = E.eval(big, 1, 3)
        low = E.eval(small, 1, 3)
        r = E.reference(items, [E.P.user * E.P.user, E.P.user, 1.0], rule=(qp, qw))
        _check(got, [[a for a, _ in r]], [[b for _, b in r]], f"{kind} {name}: 48 registers, 125 points")
        assert got.tobytes() == low.tobytes()
    finally:
        assert E.raw.destroy(big) == 0 and E.raw.destroy(small) == 0


# ================================================================================================ the rest of the device path, det < 0 in 2D
@pytest.mark.parametrize("name", FI.CW)
def test_assembly_and_diagnostics_on_clockwise_cells(name, tmp_path):
    """knp_assemble_matrix / _rhs / _precond against the oracle with the bars of
    test_gpu_irregular.test_layout_operators_and_launch_path, the launch choices of the counter-clockwise parent (the graph is the
    same), and the per-tag diagnostics as test_per_tag_diagnostics_on_cells_and_facets_of_many_sizes holds them"""
    from phim_ref import phim_ref
    from test_gpu_fluxes import _close, _random_fields, _reference
    from test_gpu_ion_budget import _host_budget
    from test_gpu_irregular import _context, _maxdiff, _rel, _set_time
    from test_gpu_membrane_potential import _check_device
    p, be, o = _context(tmp_path, name)
    lm = p.local_mesh
    E = lm.coords[lm.cells][:, 1:, :] - lm.coords[lm.cells][:, :1, :]
    assert 0.3 <= (np.linalg.det(E) < 0).mean() <= 0.7
    info = be.launch_info()
    IM.check_launch(info, IM.PARENT[name])
    assert be.n_dof_owned == o.n_dof and np.array_equal(be.node_i, o.lay.node_i.astype(np.int32))
    _set_time(p, o)
    be.assemble_matrix()
    A, Ao = be.csr(), o.assemble_A()
    print(name, "A", _maxdiff(A, Ao) / np.abs(Ao.data).max())
    assert A.shape == Ao.shape and _maxdiff(A, Ao) <= 1e-12 * np.abs(Ao.data).max()
    be.assemble_rhs()
    b, bo = be.b.cpu().numpy(), o.assemble_b()
    print(name, "b", _rel(b, bo), [_rel(b[f::4], bo[f::4]) for f in range(4)])
    assert _rel(b, bo) <= 1e-12
    for f in range(4):
        assert _rel(b[f::4], bo[f::4]) <= 1e-10, f
    be.assemble_precond()
    Pm, Po = be.precond_csr(), o.assemble_P()
    print(name, "P", _maxdiff(Pm, Po) / np.abs(Po.data).max())
    assert _maxdiff(Pm, Po) <= 1e-12 * np.abs(Po.data).max()
    # the per-tag diagnostics on random fields
    _random_fields(p, 11)
    tags = [int(t) for t in p.gamma_tags]
    ctags, host = _host_budget(p)
    assert np.array_equal(be.budget_layout().tags, ctags)
    got = be.ion_amounts().cpu().numpy()
    print(name, "ion amounts: max rel. difference", np.abs(got / host - 1.0).max())
    assert np.allclose(got, host, rtol=1e-12, atol=0)
    out = p.membrane_fluxes()
    ref, S, cover = _reference(p, [[t] for t in tags], False)
    assert list(out["tag"]) == tags and min(len(c) for c in cover) >= 20 and np.all(S > 0) and np.all(np.abs(ref) > 0)
    assert _close(out["flux_i"], ref[:, 0], S[:, 0]) and _close(out["flux_e"], ref[:, 1], S[:, 1])
    phi = p.phi_m_prev.numpy().copy()
    pot = p.membrane_potential()
    pref = phim_ref(p, phi, [[t] for t in tags])
    assert list(pot["tag"]) == tags and np.all(pref[4] > 0)
    _check_device(be.membrane_potential().cpu().numpy(), pref, name)
    assert np.allclose(pot["area"], pref[1], rtol=1e-13, atol=0)
    assert np.array_equal(pot["min"], pref[2]) and np.array_equal(pot["max"], pref[3])
