"""Derived fields on the device (cgx_hip/fields.py, csrc/knp_fields.inc): per-cell and per-facet means of user expressions against
the NumPy reference of tests/derived_field_ref.py on the irregular meshes of tests/irregular_meshes.py, their consistency with the
functionals, the raw ABI at the edges of the 128-item blocks, the projection onto vertices on synthetic item lists (every lane width,
lists around the split threshold) and on the hub meshes, and a run that records fields into fields.xdmf / fields.h5.

Tolerances.  Per-item means: |device - reference| <= tol * scale with scale = sum_q |q_w f| of the item; tol is
``functional_ref.TOL`` (1e-12) for integrands of values only and ``functionals_irregular.tolerance(floor)`` = max(TOL, 8 floor) for a
case that reads a derivative, the floor being the distance of the fp64 reference from its long-double-geometry twin
(tests/test_derived_fields_host.py holds every floor below 1e-10).  Projection: 1e-12 of sum |measure value| / sum measure."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import derived_field_ref as DR
import functional_ref
import functionals_irregular as FI
import irregular_meshes as IM
import membrane_functional_ref as mref
from functional_raw import RawMembrane, RawVolume
from functional_ref import TOL

pytestmark = pytest.mark.gpu
CANARY = -123.25      # the fill of functional_raw's evaluation buffers
PAD = 64


@pytest.fixture(scope="module")
def probs(tmp_path_factory):
    """one problem with its backend per mesh, random fields; shared by the tests, none of which writes a field"""
    cache = {}
    tmp = tmp_path_factory.mktemp("derived_fields")

    def get(name):
        if name not in cache:
            if name in FI.SEEDS or IM.PARENT.get(name) in FI.SEEDS:
                cache[name] = FI.Prob(tmp, name, backend=True)
            else:      # a mesh the functional tests do not use: the same recipe with a seed of its own
                FI.SEEDS[name] = 31
                try:
                    cache[name] = FI.Prob(tmp, name, backend=True)
                finally:
                    del FI.SEEDS[name]
        return cache[name]
    return get


def _check(got, want, scale, what, tol=TOL):
    got, want, scale = (np.asarray(a, dtype=np.float64) for a in (got, want, scale))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    print(f"{what}: max |device - host| / scale = {np.max(err / np.maximum(scale, 1e-300), initial=0.0):.3e} (tol {tol:.1e})")
    assert np.all(np.isfinite(got))
    assert np.all(err <= tol * scale), (what, float(np.max(err / np.maximum(scale, 1e-300))))


# ================================================================================================ per-item values, Python classes
@pytest.mark.parametrize("case", DR.CELL_CASES)
@pytest.mark.parametrize("name", DR.CELL_MESHES)
def test_cell_field_against_the_reference(probs, name, case):
    from cgx_hip.fields import CellField
    P = probs(name)
    p = P.p
    fi, fe, degree = DR.cell_forms(P, case)
    tol = FI.tolerance(DR.cell_floor(P, case)) if case in DR.DERIVATIVE_CASES else TOL
    F = CellField(p, fi, fe, degree=degree)
    cells, side, want, scale = DR.cell_field(p, fi, fe, degree=degree)
    lm = p.local_mesh
    assert F.n_out == (1 if case == "value" else P.dim) and np.array_equal(F.cells, cells) and np.array_equal(F.side, side)
    assert np.array_equal(F.cell_tag, np.asarray(lm.cell_tags)[cells])
    assert np.allclose(F.volume, functional_ref.cell_volumes(lm.coords[np.asarray(lm.cells)[cells]]), rtol=1e-14, atol=0)
    got = F()
    assert got.is_cuda and got.shape == (len(cells), F.n_out)
    _check(got.cpu().numpy(), want, scale, f"{name} {case}", tol)
    full = F.full().cpu().numpy()
    assert full.shape == (int(lm.n_cells_owned), F.n_out) and np.array_equal(full[cells], got.cpu().numpy())
    F.close()
    with pytest.raises(Exception):
        F()


def test_cell_field_of_some_tags_and_one_side(probs):
    from cgx_hip.fields import CellField
    P = probs(FI.TWO_TAG)
    p = P.p
    fi, fe, degree = DR.cell_forms(P, "ion_flux")
    F = CellField(p, fi, None, tags=[3], degree=degree)
    cells, side, want, scale = DR.cell_field(p, fi, None, tags=[3], degree=degree)
    assert len(cells) > 0 and np.array_equal(F.cells, cells) and set(F.cell_tag.tolist()) == {3} and set(F.side.tolist()) == {0}
    got = F.value()
    _check(got, want, scale, "tag 3 only", FI.tolerance(DR.cell_floor(P, "ion_flux")))
    full = F.full(fill=-5.0).cpu().numpy()
    rest = np.setdiff1d(np.arange(full.shape[0]), cells)
    assert np.array_equal(full[cells], got) and np.all(full[rest] == -5.0)
    ti, te = F.to_nodes()
    assert torch.isnan(te).all() and not torch.isnan(ti).all()
    with pytest.raises(ValueError):
        CellField(p, fi, None, tags=[1])            # an extracellular tag without expr_e: the functionals' refusal
    with pytest.raises(ValueError):
        CellField(p, [1.0, 1.0, 1.0, 1.0], None)    # more than three outputs


@pytest.mark.parametrize("case", DR.FACET_CASES)
@pytest.mark.parametrize("name", DR.FACET_MESHES)
def test_facet_field_against_the_reference(probs, name, case):
    from cgx_hip.fields import FacetField
    P = probs(name)
    p = P.p
    expr, degree = DR.facet_forms(P, case)
    tol = FI.tolerance(DR.facet_floor(P, case)) if case in DR.DERIVATIVE_CASES else TOL
    F = FacetField(p, expr, degree=degree)
    facets, want, scale = DR.facet_field(p, expr, degree=degree)
    assert F.n_out == {"value": 1, "I_ch": 3}.get(case, 2) and np.array_equal(F.facets, facets)
    assert np.array_equal(F.vertices, np.asarray(p._fv)[facets]) and np.array_equal(F.area, np.asarray(p._fmeas)[facets])
    assert np.array_equal(F.facet_tag, np.asarray(p.gamma_facet_tags)[facets])
    got = F()
    assert got.is_cuda and got.shape == (len(facets), F.n_out)
    _check(got.cpu().numpy(), want, scale, f"{name} {case}", tol)
    # nodal: every listed facet's vertices carry a value, every other vertex the fill
    u = F.to_nodes(fill=-9.0).cpu().numpy()
    ref, rscale, _ = DR.project(F.n_vertices, F.vertices, F.area, got.cpu().numpy(), fill=-9.0)
    _check(u, ref, rscale, f"{name} {case} to_nodes")
    on = np.zeros(F.n_vertices, dtype=bool)
    on[F.vertices.ravel()] = True
    assert np.all(u[:, ~on] == -9.0)


def test_fields_on_an_emi_problem(tmp_path):
    from cgx_hip.fields import CellField, FacetField
    p = FI.emi_problem(tmp_path, backend=True)
    fi, fe, degree = DR.emi_cell_forms(p)
    F = p.cell_field(fi, fe, degree=degree)
    assert isinstance(F, CellField) and F.n_out == 3
    cells, side, want, scale = DR.cell_field(p, fi, fe, degree=degree)
    fl = DR.floor(lambda ld: DR.cell_field(p, fi, fe, degree=degree, longdouble=ld)[2:])
    assert fl <= FI.BOUND and np.array_equal(F.cells, cells)
    _check(F.value(), want, scale, "EMI current density", FI.tolerance(fl))
    outs = FI.emi_outs(p)
    M = p.facet_field(outs, degree=2)
    assert isinstance(M, FacetField)
    facets, mwant, mscale = DR.facet_field(p, outs, degree=2)
    mfl = DR.floor(lambda ld: DR.facet_field(p, outs, degree=2, longdouble=ld)[1:])
    assert mfl <= FI.BOUND
    _check(M.value(), mwant, mscale, "EMI membrane outputs", FI.tolerance(mfl))
    ti, te = F.to_nodes()
    both = ~torch.isnan(ti[0]) & ~torch.isnan(te[0])
    assert int(both.sum()) == len(np.unique(np.asarray(p._fv)))      # the membrane vertices, and only they, have both


# ================================================================================================ consistency with the functionals
@pytest.mark.parametrize("name", DR.CELL_MESHES)
def test_cell_means_times_volume_sum_to_the_volume_functional(probs, name):
    from cgx_hip.fields import CellField
    from cgx_hip.functionals import VolumeFunctional
    P = probs(name)
    fi, fe, degree = DR.cell_forms(P, "ion_flux_degree3")
    F, V = CellField(P.p, fi, fe, degree=degree), VolumeFunctional(P.p, fi, fe, degree=degree)
    mean, integral = F.value(), V.value()
    tags, _, _, scale = functional_ref.reference(P.p, fi, fe, degree=degree)
    assert np.array_equal(tags, V.tags)
    got = np.array([[math.fsum(F.volume[F.cell_tag == t] * mean[F.cell_tag == t, j]) for j in range(F.n_out)] for t in tags])
    _check(got, integral, scale, f"{name}: sum |T| mean against VolumeFunctional")


@pytest.mark.parametrize("name", DR.FACET_MESHES)
def test_facet_means_times_area_sum_to_the_membrane_functional(probs, name):
    from cgx_hip.fields import FacetField
    from cgx_hip.functionals import MembraneFunctional
    P = probs(name)
    expr, degree = DR.facet_forms(P, "flux_dn_degree3")
    F, M = FacetField(P.p, expr, degree=degree), MembraneFunctional(P.p, expr, degree=degree)
    mean, integral = F.value(), M.value()
    tags, _, scale = mref.reference(P.p, expr, degree=degree)
    assert np.array_equal(tags, M.tags)
    got = np.array([[math.fsum(F.area[F.facet_tag == t] * mean[F.facet_tag == t, j]) for j in range(F.n_out)] for t in tags])
    _check(got, integral, scale, f"{name}: sum |F| mean against MembraneFunctional")


# ================================================================================================ the raw ABI
def _eval_items(raw, fid, fields, n_items, n_out=1, out=True):
    """(return code, [n_items, n_out], the canary past the end): one knp_*_eval_items into a buffer that held the canary"""
    buf = torch.full((n_items * n_out + PAD,), CANARY, dtype=torch.float64, device=raw.be.device)
    rc = getattr(raw.be.lib, raw.ABI + "_eval_items")(raw.be.ctx, fid, C.byref(fields) if fields is not None else None,
                                                      C.c_void_p(buf.data_ptr()) if out else None)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    return rc, h[:n_items * n_out].reshape(n_items, n_out), h[n_items * n_out:]


class _Raw:
    def __init__(self, P, kind):
        from cgx_hip import _lib
        p = P.p
        lm = p.local_mesh
        self.P, self.kind = P, kind
        self.fields = _lib.Fields()
        self.fields.aux[0] = P.user.data_ptr()
        if kind == "cells":
            self.n = int(lm.n_cells_owned)
            self.raw = RawVolume(P.be, self.n, P.dim)
            self.rule = (self.raw.args["q_bary"], self.raw.args["q_w"])
        else:
            self.fv = np.asarray(p._fv)
            self.n = len(self.fv)
            self.raw = RawMembrane(P.be, self.n, P.dim)
            self.rule = (self.raw.args["q_pts"], self.raw.args["q_w"])
            self.opp = mref.opposite_vertices(np.asarray(lm.cells), np.asarray(lm.gamma), self.fv)

    def reference(self, items):
        lm = self.P.p.local_mesh
        e = [self.P.user * self.P.user]
        if self.kind == "cells":
            return DR.cell_means(lm.coords, np.asarray(lm.cells)[items], e, *self.rule)
        return DR.facet_means(lm.coords, self.fv[items], self.opp[items], e, *self.rule)

    def create(self, seg_ptr, items):
        rc, fid = self.raw.create(n_tags=len(seg_ptr) - 1, seg_ptr=np.asarray(seg_ptr, dtype=np.int32),
                                  **{self.raw.ITEMS: np.ascontiguousarray(items, dtype=np.int32)})
        assert rc == 0, self.raw.error()
        return fid


@pytest.mark.parametrize("kind,name", [("cells", "hub2d_12_300"), ("facets", "delaunay3d_7")])
def test_eval_items_at_the_block_edges(probs, kind, name):
    R = _Raw(probs(name), kind)
    rng = np.random.default_rng(3)
    for n in (1, 127, 128, 129, 257):
        n = min(n, R.n)
        items = rng.permutation(R.n)[:n]
        fid = R.create([0, n], items)
        rc, got, tail = _eval_items(R.raw, fid, R.fields, n)
        assert rc == 0, R.raw.error()
        want, scale = R.reference(items)
        _check(got, want, scale, f"{kind} n = {n}")
        assert np.all(tail == CANARY)
        assert R.raw.destroy(fid) == 0
    assert R.n >= (257 if kind == "cells" else 129)


@pytest.mark.parametrize("kind,name", [("cells", "delaunay2d_12_cw"), ("facets", "hub2d_12_48m_cw")])
def test_eval_items_keeps_the_plans_order_and_refuses_bad_calls(probs, kind, name):
    from cgx_hip import _lib
    R = _Raw(probs(name), kind)
    items = np.array([5, 1, 9, 2, 8, 0, 4])          # two tags, neither in item order
    fid = R.create([0, 3, 7], items)
    rc, got, tail = _eval_items(R.raw, fid, R.fields, 7)
    want, scale = R.reference(items)
    assert rc == 0 and np.all(tail == CANARY)
    _check(got, want, scale, f"{kind}: rows in the plan's order")
    # the functional of the same plan: its two rows are the measure-weighted sums of those means
    rc, tot = R.raw.eval(fid, R.fields, 2)
    lm = R.P.p.local_mesh
    meas = (functional_ref.cell_volumes(lm.coords[np.asarray(lm.cells)[items]]) if kind == "cells" else np.asarray(R.P.p._fmeas)[items])
    assert rc == 0
    for t, (a, b) in enumerate(((0, 3), (3, 7))):
        assert abs(tot[t, 0] - math.fsum(meas[a:b] * got[a:b, 0])) <= TOL * np.sum(meas[a:b] * scale[a:b, 0])
    # refusals: nothing is launched, the buffer keeps the canary
    empty = _lib.Fields()
    for what, args in (("unknown id", dict(fid=fid + 1000)), ("unknown id (negative)", dict(fid=-1)), ("null out", dict(out=False)),
                       ("null fields", dict(fields=None)), ("null pointer of a slot the code reads", dict(fields=empty))):
        kw = dict(fid=fid, fields=R.fields, out=True)
        kw.update(args)
        rc, body, tail = _eval_items(R.raw, kw["fid"], kw["fields"], 7, out=kw["out"])
        assert rc < 0 and np.all(body == CANARY) and np.all(tail == CANARY), what
        assert R.raw.error(), what
    assert R.raw.destroy(fid) == 0
    rc, body, _ = _eval_items(R.raw, fid, R.fields, 7)
    assert rc < 0 and np.all(body == CANARY)         # a destroyed plan
    # a plan without items: a successful no-op, whatever else is passed
    rc0, f0 = R.raw.create(n_tags=1, seg_ptr=np.array([0, 0], dtype=np.int32))
    assert rc0 == 0
    rc, body, tail = _eval_items(R.raw, f0, None, 7, out=False)
    assert rc == 0
    rc, body, tail = _eval_items(R.raw, f0, R.fields, 7)
    assert rc == 0 and np.all(body == CANARY)
    assert R.raw.destroy(f0) == 0


# ================================================================================================ the projection, synthetic lists
class RawProjection:
    """knp_project_* through ctypes"""

    def __init__(self, be, n_vertices):
        self.be, self.n_vertices = be, n_vertices

    def create(self, iv, meas, nv=None, id=True, null=()):
        from cgx_hip import _lib
        iv = np.ascontiguousarray(iv, dtype=np.int32)
        meas = np.ascontiguousarray(meas, dtype=np.float64)
        pid = C.c_int32(-1)
        rc = self.be.lib.knp_project_create(self.be.ctx, len(meas), iv.shape[1] if nv is None else nv,
                                            None if "iv" in null else iv.ctypes.data_as(_lib.i32p),
                                            None if "meas" in null else meas.ctypes.data_as(_lib.f64p), C.byref(pid) if id else None)
        return rc, int(pid.value)

    def apply(self, pid, values, n_out, fill, null=()):
        """(return code, out [n_out, n_vertices], canary tail)"""
        v = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(self.be.device)
        buf = torch.full((n_out * self.n_vertices + PAD,), CANARY, dtype=torch.float64, device=self.be.device)
        rc = self.be.lib.knp_project_apply(self.be.ctx, pid, None if "values" in null else C.c_void_p(v.data_ptr()), n_out, float(fill),
                                           None if "out" in null else C.c_void_p(buf.data_ptr()))
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        return rc, h[:n_out * self.n_vertices].reshape(n_out, self.n_vertices), h[n_out * self.n_vertices:]

    def info(self, pid):
        from cgx_hip import _lib
        from cgx_hip.fields import PROJECT_INFO
        v = np.full(len(PROJECT_INFO), -1, dtype=np.int32)
        assert self.be.lib.knp_project_get_info(self.be.ctx, pid, v.ctypes.data_as(_lib.i32p), len(v)) == 0
        return dict(zip(PROJECT_INFO, (int(x) for x in v)))

    def destroy(self, pid):
        return self.be.lib.knp_project_destroy(self.be.ctx, pid)

    def error(self):
        return (self.be.lib.knp_last_error(self.be.ctx) or b"").decode()


def _hubs(lengths, nv, n_pool, rng):
    """items of ``nv`` vertices: hub k (vertex 1 + k; vertex 0 stays empty) is held by ``lengths[k]`` items whose other vertices cycle
    through a pool of ``n_pool`` vertices behind the hubs; shuffled"""
    first = 1 + len(lengths)
    iv, t = [], 0
    for k, ln in enumerate(lengths):
        for _ in range(ln):
            iv.append([1 + k] + [first + (t + a) % n_pool for a in range(nv - 1)])
            t += 1
    iv = np.array(iv, dtype=np.int32).reshape(-1, nv)
    return iv[rng.permutation(len(iv))]


def _project_case(R, iv, n_out, fill, rng, what):
    meas = 10.0 ** rng.uniform(-3.0, 3.0, len(iv))                     # spread over 1e6
    values = rng.uniform(-2.0, 3.0, (len(iv), n_out)) * 10.0 ** rng.uniform(-2.0, 2.0, (len(iv), 1))      # mixed sign
    rc, pid = R.create(iv, meas)
    assert rc == 0, R.error()
    want, scale, ptr = DR.project(R.n_vertices, iv, meas, values, fill=fill)
    info = R.info(pid)
    assert info == DR.plan_info(ptr), (what, info, DR.plan_info(ptr))
    rc, got, tail = R.apply(pid, values, n_out, fill)
    rc2, again, _ = R.apply(pid, values, n_out, fill)
    assert rc == 0 and rc2 == 0 and np.all(tail == CANARY)
    assert np.array_equal(got.view(np.int64), again.view(np.int64)), what      # the same bits, NaN fill included
    empty = np.diff(ptr) == 0
    assert empty[0] and (np.all(np.isnan(got[:, empty])) if math.isnan(fill) else np.all(got[:, empty] == fill)), what
    _check(got[:, ~empty], want[:, ~empty], scale[:, ~empty], what)
    assert R.destroy(pid) == 0
    return info, ptr


@pytest.mark.parametrize("L", DR.LANES)
def test_projection_star_lists_at_every_lane_width(probs, L):
    be = probs("delaunay2d_12_cw").be
    R = RawProjection(be, probs("delaunay2d_12_cw").p.local_mesh.coords.shape[0])
    rng = np.random.default_rng(40 + L)
    lengths = [1, L - 1, L, L + 1] if L > 2 else [1, 1, 2, 3]
    for n_out, fill in ((1, float("nan")), (2, 4.5), (3, float("nan"))):
        info, ptr = _project_case(R, _hubs(lengths, 2, 3, rng), n_out, fill, rng, f"L = {L}, n_out = {n_out}")
        assert info["lanes"] == L and info["n_split"] == 0
        assert sorted(np.diff(ptr)[1:1 + len(lengths)].tolist()) == sorted(lengths) and np.diff(ptr)[0] == 0


def test_projection_lists_around_the_split_threshold(probs):
    be = probs("delaunay2d_12_cw").be
    n_v = probs("delaunay2d_12_cw").p.local_mesh.coords.shape[0]
    R = RawProjection(be, n_v)
    rng = np.random.default_rng(77)
    S = DR.SPLIT
    lengths = [S - 1, S, S + 1, 3 * S + 7]
    assert n_v >= 1 + len(lengths) + 40
    for nv, n_out, fill in ((3, 1, float("nan")), (2, 3, -1.5), (4, 2, float("nan"))):
        info, ptr = _project_case(R, _hubs(lengths, nv, 40, rng), n_out, fill, rng, f"split, nv = {nv}, n_out = {n_out}")
        assert info["split"] == S and info["n_split"] == 2 and info["longest"] == 3 * S + 7
        assert info["n_units"] == n_v - 2 + 2 + 4      # every vertex one unit, the two long lists 2 and 4


def test_projection_refusals(probs):
    P = probs("delaunay2d_12_cw")
    n_v = P.p.local_mesh.coords.shape[0]
    R = RawProjection(P.be, n_v)
    iv, meas = np.array([[0, 1, 2], [2, 3, 4]]), np.array([1.0, 2.0])
    bad = [("null id", dict(id=False)), ("null item_vertices", dict(null=("iv",))), ("null measure", dict(null=("meas",))),
           ("nv = 1", dict(nv=1)), ("nv = 5", dict(nv=5))]
    for what, kw in bad:
        rc, pid = R.create(iv, meas, **kw)
        assert rc < 0 and pid == -1 and R.error(), what
    for what, biv, bm in (("vertex -1", [[0, 1, -1], [2, 3, 4]], meas), ("vertex n_vertices", [[0, 1, 2], [2, 3, n_v]], meas),
                          ("a vertex twice", [[0, 1, 2], [3, 4, 3]], meas), ("measure 0", iv, [1.0, 0.0]), ("measure < 0", iv, [-1.0, 1.0]),
                          ("measure NaN", iv, [1.0, float("nan")]), ("measure inf", iv, [float("inf"), 1.0])):
        rc, pid = R.create(np.array(biv), np.array(bm))
        assert rc < 0 and pid == -1 and R.error(), what
    rc, pid = R.create(iv, meas)
    assert rc == 0
    vals = np.array([[1.0], [2.0]])
    for what, kw in (("unknown id", dict(pid=pid + 1000)), ("n_out = 0", dict(n_out=0)), ("n_out = 4", dict(n_out=4)),
                     ("null values", dict(null=("values",))), ("null out", dict(null=("out",)))):
        a = dict(pid=pid, n_out=1, null=())
        a.update(kw)
        rc, body, tail = R.apply(a["pid"], vals, a["n_out"], 0.0, a["null"])
        assert rc < 0 and np.all(body == CANARY) and np.all(tail == CANARY) and R.error(), what
    rc, got, _ = R.apply(pid, vals, 1, 0.0)
    assert rc == 0 and abs(got[0, 2] - 5.0 / 3.0) <= 1e-15 and got[0, 0] == 1.0 and got[0, 4] == 2.0 and got[0, 5] == 0.0
    assert R.be.lib.knp_project_get_info(R.be.ctx, pid + 1000, (C.c_int32 * 5)(), 5) < 0
    assert R.be.lib.knp_project_get_info(None, pid, (C.c_int32 * 5)(), 5) < 0
    assert R.destroy(pid) == 0 and R.destroy(pid) < 0
    rc2, pid2 = R.create(iv, meas)
    assert rc2 == 0 and pid2 == pid and R.destroy(pid2) == 0      # a destroyed id is reused


# ================================================================================================ the projection on meshes
@pytest.mark.parametrize("name", ["hub2d_12_300", "hub3d_5_140"])
def test_projection_on_hub_meshes(probs, name):
    from cgx_hip.fields import CellField
    P = probs(name)
    p = P.p
    lm = p.local_mesh
    d = P.dim
    fi, fe, degree = DR.cell_forms(P, "ion_flux")
    F = CellField(p, fi, fe, degree=degree)
    vals = F()
    ti, te = F.to_nodes(values=vals)
    h = vals.cpu().numpy()
    cells = np.asarray(lm.cells)
    hub = IM.hub_vertex(np.asarray(IM.mesh(name)[0]), (0.5,) * d)
    lhs, seen_hub = 0.0, False
    for s, t in enumerate((ti, te)):
        sel = F.side == s
        want, scale, ptr = DR.project(F.n_vertices, cells[F.cells[sel]], F.volume[sel], h[sel])
        got = t.cpu().numpy()
        empty = np.diff(ptr) == 0
        assert np.all(np.isnan(got[:, empty])) and empty.any()
        _check(got[:, ~empty], want[:, ~empty], scale[:, ~empty], f"{name}: side {s} projection")
        info = F._proj[s].info()
        assert info == DR.plan_info(ptr)
        if not empty[hub]:
            assert np.diff(ptr)[hub] >= int(name.rsplit("_", 1)[1]) and info["longest"] == np.diff(ptr)[hub]
            _check(got[:, hub], want[:, hub], scale[:, hub], f"{name}: the hub vertex ({np.diff(ptr)[hub]} cells)")
            seen_hub = True
        lump = np.zeros(F.n_vertices)
        np.add.at(lump, cells[F.cells[sel]].ravel(), np.repeat(F.volume[sel], d + 1))
        lhs = lhs + np.array([math.fsum(np.nan_to_num(got[j]) * lump / (d + 1)) for j in range(F.n_out)])
    assert seen_hub
    rhs = np.array([math.fsum(F.volume * h[:, j]) for j in range(F.n_out)])
    _check(lhs, rhs, np.abs(F.volume[:, None] * h).sum(axis=0), f"{name}: sum_v u(v) lump(v) / (d + 1) = sum_T |T| mean_T")
    # a membrane vertex carries both values, each from its own side's cells
    both = np.nonzero(~np.isnan(ti[0].cpu().numpy()) & ~np.isnan(te[0].cpu().numpy()))[0]
    assert set(both.tolist()) == set(np.unique(np.asarray(p._fv)).tolist())
    assert np.all(ti.cpu().numpy()[:, both] != te.cpu().numpy()[:, both])
    fi_, fe_ = F.functions()
    assert len(fi_) == d and torch.equal(torch.nan_to_num(fi_[1].x.array), torch.nan_to_num(ti[1]))
    from cgx_hip.sampling import FieldSampler
    pts = lm.coords[cells[:5]].mean(axis=1)
    smp = FieldSampler(p, pts)(fi_, fe_).cpu().numpy()      # the sampler takes the projections
    assert smp.shape[-1] == 5 and np.all(np.isfinite(smp))


# ================================================================================================ a run that records fields
def _run(tmp_path, sub, with_fields):
    from parity_utils import ci_config, make_problem
    from cgx_hip import fem
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    cfg = ci_config(N=8, steps=3, rtol=1e-11)
    cfg["quiet"] = True
    cfg["output_dir"] = str(tmp_path / sub) + os.sep
    cfg["solver"]["output"].update({"save_xdmf": True, "save_interval": 1})
    p = make_problem(cfg, "ci")
    p.solver_config["view_ksp"] = False
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    F = {}
    if with_fields:
        phi = [p.wh[k][p.N_ions] for k in range(2)]
        F["J"] = p.cell_field([-g for g in fem.grad(phi[0])], [-g for g in fem.grad(phi[1])])
        F["rho"] = p.cell_field(p.wh[0][0] + p.wh[0][1] - p.wh[0][2], p.wh[1][0] + p.wh[1][1] - p.wh[1][2], degree=1)
        F["I"] = p.facet_field(p.ion_list[0]["I_ch"][p.gamma_tags[0]], degree=2)
        s.add_field("J", F["J"])
        s.add_field("rho", F["rho"], interval=2, nodal=True)
        s.add_field("I", F["I"], interval=3)
        with pytest.raises(ValueError):
            s.add_field("J", F["J"])
        with pytest.raises(ValueError):
            s.add_field("other", object())
        with pytest.raises(ValueError):
            s.add_field("zero", F["J"], interval=0)
    s.solve()
    if with_fields:
        with pytest.raises(RuntimeError):
            s.add_field("late", F["J"])
    return cfg["output_dir"], p, F


def test_a_run_records_fields_and_leaves_the_solution_files_alone(tmp_path):
    import xml.etree.ElementTree as ET
    from cgx_hip import hdf5_min
    plain, _, _ = _run(tmp_path, "plain", False)
    out, p, F = _run(tmp_path, "fields", True)
    assert not os.path.exists(plain + "fields.xdmf") and not os.path.exists(plain + "fields.h5")
    for f in ("solution.h5", "solution.xdmf"):
        assert open(plain + f, "rb").read() == open(out + f, "rb").read(), f
    lm = p.local_mesh
    nc, nv = int(lm.n_cells_owned), lm.coords.shape[0]
    h = hdf5_min.Hdf5File(out + "fields.h5")
    assert h.keys("/Field/J") == ["0", "1", "2", "3"] and h.keys("/Field/rho_i") == ["0", "1"] and h.keys("/Field/I") == ["0", "1"]
    J = h.read("/Field/J/3")
    assert J.shape == (nc, 3) and np.array_equal(J[:, :2], F["J"].full().cpu().numpy()) and np.all(J[:, 2] == 0.0)
    assert np.array_equal(h.read("/Field/I/1"), F["I"]().cpu().numpy()) and h.read("/Field/I/1").shape == (len(F["I"].facets), 1)
    assert np.array_equal(h.read("/Mesh/membrane/topology"), F["I"].vertices)
    ri = h.read("/Field/rho_i/1")                  # recorded at step 2; the state has moved on since
    assert ri.shape == (nv, 1) and np.isnan(ri).any() and not np.isnan(ri).all()
    root = ET.parse(out + "fields.xdmf").getroot()
    steps = [g for g in root.iter("Grid") if g.get("CollectionType") == "Spatial"]
    assert len(steps) == 4 and len(list(root.iter("Time"))) == 4
    names = [[a.get("Name") for a in g.iter("Attribute")] for g in steps]
    assert names == [["J", "rho_i", "rho_e", "I"], ["J"], ["J", "rho_i", "rho_e"], ["J", "I"]]
    cen = {a.get("Name"): (a.get("Center"), a.get("AttributeType")) for a in root.iter("Attribute")}
    assert cen == {"J": ("Cell", "Vector"), "rho_i": ("Node", "Scalar"), "rho_e": ("Node", "Scalar"), "I": ("Cell", "Scalar")}
    assert [g.get("Name") for g in steps[0].findall("Grid")] == ["mesh", "membrane"]
    assert 'TopologyType="Polyline"' in open(out + "fields.xdmf").read()
