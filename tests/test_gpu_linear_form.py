"""Linear forms on the device (cgx_hip/linear_forms.py, csrc/knp_fields.inc): ``int f v dx`` / ``int g v dS`` per vertex against the
NumPy reference of tests/linear_form_ref.py on the irregular meshes of tests/irregular_meshes.py, bit-identical repeats, the raw ABI
of the load end at the edges of the 128-item blocks, the sum-only gather on synthetic item lists (every lane width, lists around the
split threshold), the refusals of the new entry points, ``knp_rhs_add_load`` row by row, and sources in a step.

Tolerances.  A vertex's entry: |device - reference| <= tol * scale with scale = the sum over the vertex's entries of
meas sum_q |q_w lambda_a f|; tol = ``functionals_irregular.tolerance(floor)`` = max(1e-12, 8 floor), the floor being the distance of
the fp64 reference from its long-double-geometry twin (tests/test_linear_form_host.py holds every floor below 1e-10).  The gather
alone: 1e-12 of the sum of |values| of the list.  A vertex without a listed item is exactly 0.

The step tests run on the tissue lattice (``tissue_config(2, 20, 2)``), not on the CI square: at N = 8 the square has no cell inside
the reference's injection cube, and on finer squares the cube lies inside the one cell, where the extracellular nodal source of
``source_terms: ion_injection`` acts on no node.  On the lattice the cube covers the gap between the four cells.  In (a) both
problems' nodal sources are scaled by 1e10 before the assembly: the row's scale dt sum_b |M_ab f_b| is then the size of the whole
row, so that the rounding of the far larger term M k_prev that shares the row (1e5 .. 1e7 times the unscaled source) does not
count against the 1e-12 of the source's own scale.

Measured on MI355X (step (b), K summed over all tags, 3 steps at rtol 1e-11): see DESIGN.md section 14."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import derived_field_ref as DR
import functionals_irregular as FI
import linear_form_ref as LR
import membrane_functional_ref as mref
from functional_raw import RawMembrane, RawVolume
from functional_ref import TOL

pytestmark = pytest.mark.gpu
CANARY = -123.25
PAD = 64


@pytest.fixture(scope="module")
def probs(tmp_path_factory):
    """one problem with its backend per mesh, random fields; shared by the tests, none of which writes a field"""
    cache = {}
    tmp = tmp_path_factory.mktemp("linear_forms")

    def get(name):
        if name not in cache:
            cache[name] = FI.Prob(tmp, name, backend=True)
        return cache[name]
    return get


def _check(got, want, scale, what, tol=TOL):
    got, want, scale = (np.asarray(a, dtype=np.float64) for a in (got, want, scale))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    pos = scale > 0
    print(f"{what}: max |device - host| / scale = {np.max(err[pos] / scale[pos], initial=0.0):.3e} (tol {tol:.1e})")
    assert np.all(np.isfinite(got))
    assert np.all(err <= tol * scale), (what, float(np.max(err[pos] / scale[pos], initial=0.0)), float(np.max(err[~pos], initial=0.0)))


# ================================================================================================ 1. forms against the reference
@pytest.mark.parametrize("case", FI.VOLUME_CASES)
@pytest.mark.parametrize("name", FI.VOLUME_MESHES)
def test_volume_form_against_the_reference(probs, name, case):
    from cgx_hip.linear_forms import VolumeLinearForm
    P = probs(name)
    fi, fe, degree = LR.volume_case(P, case)
    tol = FI.tolerance(LR.volume_floor(P, case))
    F = VolumeLinearForm(P.p, fi, fe, degree=degree)
    want, scale, on = LR.volume_form(P.p, fi, fe, degree=degree)
    got = F()
    assert got.is_cuda and tuple(got.shape) == (2, F.n_out, F.n_vertices) == want.shape
    h = got.cpu().numpy()
    _check(h, want, scale, f"{name} {case}", tol)
    for s in range(2):
        assert on[s].any() and not on[s].all() and np.all(h[s][:, ~on[s]] == 0.0)
        assert F._scatter[s].info() == DR.plan_info(LR.entries(F.n_vertices, np.asarray(P.p.local_mesh.cells)[F.cells[s]])[0])
    assert np.array_equal(F.value(), h)
    F.close()
    with pytest.raises(Exception):
        F()


@pytest.mark.parametrize("case", FI.MEMBRANE_CASES)
@pytest.mark.parametrize("name", FI.MEMBRANE_MESHES)
def test_membrane_form_against_the_reference(probs, name, case):
    """the closed cases run over the pooled group of all membrane tags (two tags pooled on the two-tag mesh)"""
    from cgx_hip.linear_forms import MembraneLinearForm
    P = probs(name)
    outs, tags, degree = LR.membrane_case(P, case)
    tol = FI.tolerance(LR.membrane_floor(P, case))
    F = MembraneLinearForm(P.p, outs, tags, degree=degree)
    want, scale, on = LR.membrane_form(P.p, outs, tags, degree=degree)
    assert np.array_equal(F.facets, LR.membrane_facets(P.p, tags))
    got = F()
    assert got.is_cuda and tuple(got.shape) == (F.n_out, F.n_vertices) == want.shape
    h = got.cpu().numpy()
    _check(h, want, scale, f"{name} {case}", tol)
    assert on.any() and not on.all() and np.all(h[:, ~on] == 0.0)


def test_forms_of_some_tags_one_side_and_the_one_shot_calls(probs):
    from cgx_hip.linear_forms import VolumeLinearForm
    P = probs(FI.TWO_TAG)
    p = P.p
    fi, fe, degree = LR.volume_case(P, "nonlinear")
    tol = FI.tolerance(LR.volume_floor(P, "nonlinear"))
    F = VolumeLinearForm(p, fi, None, tags=[3], degree=degree)
    want, scale, on = LR.volume_form(p, fi, None, tags=[3], degree=degree)
    h = F.value()
    _check(h, want, scale, "tag 3 only, intracellular only", tol)
    assert np.all(h[1] == 0.0) and on[0].any() and np.all(h[0][:, ~on[0]] == 0.0)
    out = torch.full((2 * 3 * F.n_vertices,), CANARY, dtype=torch.float64, device=P.be.device)
    assert F(out=out).data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy().reshape(h.shape), h)
    with pytest.raises(ValueError):
        F(out=out[:-1])
    with pytest.raises(ValueError):
        VolumeLinearForm(p, fi, None, tags=[1])            # an extracellular tag without integrand_e: the functionals' refusal
    with pytest.raises(ValueError):
        VolumeLinearForm(p, [1.0, 1.0, 1.0, 1.0], None)    # more than three outputs
    full = p.assemble_vector(fi, fe, degree=degree)
    wfull, sfull, _ = LR.volume_form(p, fi, fe, degree=degree)
    _check(full, wfull, sfull, "assemble_vector", tol)
    outs, tags, mdeg = LR.membrane_case(P, "random_minus")
    one = [int(p.gamma_tags[0])]
    mv = p.assemble_vector_membrane(outs, tags=one, degree=mdeg)
    mw, ms, mon = LR.membrane_form(p, outs, one, degree=mdeg)
    _check(mv, mw, ms, "assemble_vector_membrane, one tag of two", FI.tolerance(LR.membrane_floor(P, "random_minus")))
    assert mon.any() and np.all(mv[:, ~mon] == 0.0)


def test_forms_on_an_emi_problem(tmp_path):
    p = FI.emi_problem(tmp_path, backend=True)
    fi, fe = [p.wh[0] * p.n, -p.sigma_i * p.wh[0]], [p.wh[1], p.sigma_e * p.wh[1] * p.wh[1]]
    got = p.assemble_vector(fi, fe, degree=3)
    want, scale, _ = LR.volume_form(p, fi, fe, degree=3)
    _check(got, want, scale, "EMI volume form")
    outs = FI.emi_outs(p)
    fl = LR.floor(lambda ld: LR.membrane_form(p, outs, degree=3, longdouble=ld))
    assert fl <= FI.BOUND
    mw, ms, _ = LR.membrane_form(p, outs, degree=3)
    _check(p.assemble_vector_membrane(outs, degree=3), mw, ms, "EMI membrane form", FI.tolerance(fl))
    assert not hasattr(p, "add_source")


# ================================================================================================ 2. bit-identical runs
@pytest.mark.parametrize("name", ["hub2d_12_300", FI.TWO_TAG])
def test_repeated_calls_give_the_same_bits(probs, name):
    from cgx_hip.linear_forms import MembraneLinearForm, VolumeLinearForm
    P = probs(name)
    fi, fe, degree = LR.volume_case(P, "nonlinear")
    F = VolumeLinearForm(P.p, fi, fe, degree=degree)
    a, b = F(), F()
    outs, tags, mdeg = LR.membrane_case(P, "flux_i")
    M = MembraneLinearForm(P.p, outs, tags, degree=mdeg)
    ma = M()
    G = VolumeLinearForm(P.p, P.user, P.lin, degree=2)      # another form in between
    G()
    c, mb = F(), M()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(ma, mb)
    assert not torch.equal(a[:, :1], G())


# ================================================================================================ 3. block edges of the load end
def _three_outputs():
    """OUT_0 = aux_0 ^ 2, OUT_1 = aux_0, OUT_2 = aux_0 ^ 3"""
    from cgx_hip._lib import OPS
    return np.array([[OPS["AUX"], 0, 0, 0], [OPS["MUL"], 1, 0, 0], [OPS["MUL"], 2, 0, 1], [OPS["OUT"], 0, 0, 1], [OPS["OUT"], 0, 1, 0],
                     [OPS["OUT"], 0, 2, 2]], dtype=np.int32)


class _Raw:
    def __init__(self, P, kind):
        from cgx_hip import _lib
        p = P.p
        lm = p.local_mesh
        self.P, self.kind = P, kind
        self.fields = _lib.Fields()
        self.fields.aux[0] = P.user.data_ptr()
        if kind == "cells":
            self.n, self.nv = int(lm.n_cells_owned), P.dim + 1
            self.raw = RawVolume(P.be, self.n, P.dim)
            self.rule = (self.raw.args["q_bary"], self.raw.args["q_w"])
        else:
            self.fv = np.asarray(p._fv)
            self.n, self.nv = len(self.fv), P.dim
            self.raw = RawMembrane(P.be, self.n, P.dim)
            self.rule = (self.raw.args["q_pts"], self.raw.args["q_w"])
            self.opp = mref.opposite_vertices(np.asarray(lm.cells), np.asarray(lm.gamma), self.fv)

    def reference(self, items, n_out):
        lm = self.P.p.local_mesh
        u = self.P.user
        e = [u * u] if n_out == 1 else [u * u, u, u * u * u]
        if self.kind == "cells":
            return LR.cell_loads(lm.coords, np.asarray(lm.cells)[items], e, *self.rule)
        return LR.facet_loads(lm.coords, self.fv[items], self.opp[items], np.asarray(self.P.p._fmeas)[items], e, *self.rule)

    def create(self, items, n_out=1):
        kw = {} if n_out == 1 else dict(n_out=3, n_instr=6, code=_three_outputs())
        rc, fid = self.raw.create(n_tags=1, seg_ptr=np.array([0, len(items)], dtype=np.int32),
                                  **{self.raw.ITEMS: np.ascontiguousarray(items, dtype=np.int32)}, **kw)
        assert rc == 0, self.raw.error()
        return fid

    def eval_load(self, fid, n_items, n_out=1, fields=True, out=True):
        """(return code, [n_items, nv, n_out], the guard of nv * n_out doubles past the end, the padding behind it)"""
        size, guard = n_items * self.nv * n_out, self.nv * n_out
        buf = torch.full((size + guard + PAD,), CANARY, dtype=torch.float64, device=self.raw.be.device)
        f = self.fields if fields is True else fields
        rc = getattr(self.raw.be.lib, self.raw.ABI + "_eval_load")(self.raw.be.ctx, fid, C.byref(f) if f is not None else None,
                                                                   C.c_void_p(buf.data_ptr()) if out else None)
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        return rc, h[:size].reshape(n_items, self.nv, n_out), h[size:]


@pytest.mark.parametrize("kind,name", [("cells", "hub2d_12_300"), ("cells", "delaunay3d_5"), ("facets", "delaunay2d_92"), ("facets", "delaunay3d_7")])
def test_eval_load_at_the_block_edges(probs, kind, name):
    R = _Raw(probs(name), kind)
    rng = np.random.default_rng(7)
    assert R.n >= (257 if kind == "cells" else 129)
    for n_out in (1, 3):
        for n in (1, 127, 128, 129, 257):
            n = min(n, R.n)
            items = rng.permutation(R.n)[:n]
            fid = R.create(items, n_out)
            rc, got, tail = R.eval_load(fid, n, n_out)
            assert rc == 0, R.raw.error()
            want, scale = R.reference(items, n_out)
            _check(got, want, scale, f"{kind} {name} n = {n}, n_out = {n_out}")
            assert np.all(tail == CANARY)
            assert R.raw.destroy(fid) == 0


# ================================================================================================ 4. the gather, synthetic lists
class RawScatter:
    """knp_scatter_* through ctypes"""

    def __init__(self, be, n_vertices):
        self.be, self.n_vertices = be, n_vertices

    def create(self, iv, nv=None, id=True, null=False):
        from cgx_hip import _lib
        iv = np.ascontiguousarray(iv, dtype=np.int32)
        sid = C.c_int32(-1)
        rc = self.be.lib.knp_scatter_create(self.be.ctx, len(iv), iv.shape[1] if nv is None else nv,
                                            None if null else iv.ctypes.data_as(_lib.i32p), C.byref(sid) if id else None)
        return rc, int(sid.value)

    def apply(self, sid, values, n_out, null=()):
        """(return code, out [n_out, n_vertices], canary tail)"""
        v = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(self.be.device)
        buf = torch.full((max(n_out, 1) * self.n_vertices + PAD,), CANARY, dtype=torch.float64, device=self.be.device)
        rc = self.be.lib.knp_scatter_apply(self.be.ctx, sid, None if "values" in null else C.c_void_p(v.data_ptr()), n_out,
                                           None if "out" in null else C.c_void_p(buf.data_ptr()))
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        k = max(n_out, 1) * self.n_vertices
        return rc, h[:k].reshape(max(n_out, 1), self.n_vertices), h[k:]

    def info(self, sid):
        from cgx_hip import _lib
        from cgx_hip.fields import PROJECT_INFO
        v = np.full(len(PROJECT_INFO), -1, dtype=np.int32)
        assert self.be.lib.knp_scatter_get_info(self.be.ctx, sid, v.ctypes.data_as(_lib.i32p), len(v)) == 0
        return dict(zip(PROJECT_INFO, (int(x) for x in v)))

    def destroy(self, sid):
        return self.be.lib.knp_scatter_destroy(self.be.ctx, sid)

    def error(self):
        return (self.be.lib.knp_last_error(self.be.ctx) or b"").decode()


def _scatter_case(R, iv, n_out, rng, what):
    nv = iv.shape[1]
    values = rng.uniform(-2.0, 3.0, (len(iv), nv, n_out)) * 10.0 ** rng.uniform(-3.0, 3.0, (len(iv), 1, 1))      # mixed sign, spread 1e6
    rc, sid = R.create(iv)
    assert rc == 0, R.error()
    want, ptr = LR.gather(R.n_vertices, iv, values)
    scale, _ = LR.gather(R.n_vertices, iv, np.abs(values))
    info = R.info(sid)
    assert info == DR.plan_info(ptr), (what, info, DR.plan_info(ptr))
    rc, got, tail = R.apply(sid, values, n_out)
    rc2, again, _ = R.apply(sid, values, n_out)
    assert rc == 0 and rc2 == 0 and np.all(tail == CANARY)
    assert np.array_equal(got.view(np.int64), again.view(np.int64)), what
    empty = np.diff(ptr) == 0
    assert empty[0] and np.all(got[:, empty] == 0.0), what
    _check(got, want, scale, what)
    assert R.destroy(sid) == 0
    return info, ptr


@pytest.mark.parametrize("L", DR.LANES)
def test_gather_star_lists_at_every_lane_width(probs, L):
    from test_gpu_derived_fields import _hubs
    P = probs("delaunay2d_12_cw")
    R = RawScatter(P.be, P.p.local_mesh.coords.shape[0])
    rng = np.random.default_rng(140 + L)
    lengths = [1, L - 1, L, L + 1] if L > 2 else [1, 1, 2, 3]      # vertex 0 keeps the empty list
    for nv, n_out in ((2, 1), (2, 2), (2, 3), (3, 2), (4, 3)):
        info, ptr = _scatter_case(R, _hubs(lengths, nv, 3, rng), n_out, rng, f"L = {L}, nv = {nv}, n_out = {n_out}")
        assert info["n_split"] == 0 and (info["lanes"] == L or nv > 2)
        assert sorted(np.diff(ptr)[1:1 + len(lengths)].tolist()) == sorted(lengths) and np.diff(ptr)[0] == 0


def test_gather_lists_around_the_split_threshold(probs):
    from test_gpu_derived_fields import _hubs
    P = probs("delaunay2d_12_cw")
    n_v = P.p.local_mesh.coords.shape[0]
    R = RawScatter(P.be, n_v)
    rng = np.random.default_rng(177)
    S = DR.SPLIT
    lengths = [S - 1, S, S + 1, 2 * S + 1]      # 511, 512, 513, 1025
    assert S == 512 and n_v >= 1 + len(lengths) + 40
    for nv, n_out in ((3, 1), (2, 3), (4, 2)):
        info, ptr = _scatter_case(R, _hubs(lengths, nv, 40, rng), n_out, rng, f"split, nv = {nv}, n_out = {n_out}")
        assert info["split"] == S and info["n_split"] == 2 and info["longest"] == 2 * S + 1
        assert info["n_units"] == n_v - 2 + 2 + 3      # every vertex one unit, the two long lists 2 and 3


# ================================================================================================ 5. refusals
def test_refusals_of_the_new_entry_points(probs):
    from cgx_hip import _lib
    P = probs("delaunay2d_12_cw")
    be = P.be
    n_v = P.p.local_mesh.coords.shape[0]
    # ---- the load end: the codes and the nothing-launched rule of *_eval_items
    for kind in ("cells", "facets"):
        R = _Raw(P, kind)
        fid = R.create(np.array([5, 1, 9, 2, 8, 0, 4]))
        empty = _lib.Fields()
        for what, kw in (("unknown id", dict(fid=fid + 1000)), ("negative id", dict(fid=-1)), ("null out", dict(out=False)),
                         ("null fields", dict(fields=None)), ("null pointer of a slot the code reads", dict(fields=empty))):
            a = dict(fid=fid, fields=True, out=True)
            a.update(kw)
            rc, body, tail = R.eval_load(a["fid"], 7, fields=a["fields"], out=a["out"])
            assert rc == -1 and np.all(body == CANARY) and np.all(tail == CANARY) and R.raw.error(), (kind, what)
        assert R.raw.destroy(fid) == 0
        rc, body, _ = R.eval_load(fid, 7)
        assert rc == -1 and np.all(body == CANARY) and "unknown" in R.raw.error()
        rc0, f0 = R.raw.create(n_tags=1, seg_ptr=np.array([0, 0], dtype=np.int32))      # a plan without items: a successful no-op
        assert rc0 == 0
        assert R.eval_load(f0, 7, fields=None, out=False)[0] == 0
        rc, body, tail = R.eval_load(f0, 7)
        assert rc == 0 and np.all(body == CANARY) and np.all(tail == CANARY)
        assert R.raw.destroy(f0) == 0
    # ---- the gather: the refusals of knp_project_create without the measure
    S = RawScatter(be, n_v)
    iv = np.array([[0, 1, 2], [2, 3, 4]])
    for what, kw in (("null id", dict(id=False)), ("null item_vertices", dict(null=True)), ("nv = 1", dict(nv=1)), ("nv = 5", dict(nv=5))):
        rc, sid = S.create(iv, **kw)
        assert rc == -1 and sid == -1 and "scatter" in S.error(), what
    for what, biv in (("vertex -1", [[0, 1, -1], [2, 3, 4]]), ("vertex n_vertices", [[0, 1, 2], [2, 3, n_v]]), ("a vertex twice", [[0, 1, 2], [3, 4, 3]])):
        rc, sid = S.create(np.array(biv))
        assert rc == -1 and sid == -1 and "scatter" in S.error(), what
    rc, sid = S.create(iv)
    assert rc == 0
    vals = np.array([[[1.0], [2.0], [4.0]], [[8.0], [16.0], [32.0]]])
    for what, kw in (("unknown id", dict(sid=sid + 1000)), ("n_out = 0", dict(n_out=0)), ("n_out = 4", dict(n_out=4)),
                     ("null values", dict(null=("values",))), ("null out", dict(null=("out",)))):
        a = dict(sid=sid, n_out=1, null=())
        a.update(kw)
        rc, body, tail = S.apply(a["sid"], vals, a["n_out"], a["null"])
        assert rc == -1 and np.all(body == CANARY) and np.all(tail == CANARY) and S.error(), what
    rc, got, _ = S.apply(sid, vals, 1)
    assert rc == 0 and got[0, :6].tolist() == [1.0, 2.0, 12.0, 16.0, 32.0, 0.0]
    assert be.lib.knp_scatter_get_info(be.ctx, sid + 1000, (C.c_int32 * 5)(), 5) < 0 and be.lib.knp_scatter_get_info(None, sid, (C.c_int32 * 5)(), 5) < 0
    assert S.destroy(sid) == 0 and S.destroy(sid) == -1
    rc2, sid2 = S.create(iv)
    assert rc2 == 0 and sid2 == sid and S.destroy(sid2) == 0      # a destroyed id is reused
    # ---- knp_rhs_add_load
    b = torch.full((be.n_dof_local + PAD,), CANARY, dtype=torch.float64, device=be.device)
    load = torch.ones(n_v, dtype=torch.float64, device=be.device)
    bp, lp = C.c_void_p(b.data_ptr()), C.c_void_p(load.data_ptr())
    for what, args in (("field -1", (-1, 0, 1.0, lp, bp)), ("field 4", (4, 0, 1.0, lp, bp)), ("side -1", (0, -1, 1.0, lp, bp)),
                       ("side 2", (0, 2, 1.0, lp, bp)), ("null load", (0, 0, 1.0, None, bp)), ("null b", (0, 0, 1.0, lp, None))):
        assert be.lib.knp_rhs_add_load(be.ctx, *args) == -1, what
        assert "rhs_add_load" in (be.lib.knp_last_error(be.ctx) or b"").decode(), what
    torch.cuda.synchronize()
    assert torch.all(b == CANARY)


def test_rhs_add_load_refuses_a_context_with_ghost_nodes(tmp_path):
    import irregular_meshes as IM
    import rank_pieces as RP
    from parity_utils import make_problem
    lm = RP.cut_piece("hub2d_12_48m", 0)
    p = make_problem(IM.config(tmp_path, "hub2d_12_48m"), "ci", lm)
    be = p.create_backend()
    assert be.n_nodes > be.n_nodes_owned
    b = torch.full((be.n_dof_local,), CANARY, dtype=torch.float64, device=be.device)
    load = torch.ones(lm.coords.shape[0], dtype=torch.float64, device=be.device)
    assert be.lib.knp_rhs_add_load(be.ctx, 0, 0, 1.0, C.c_void_p(load.data_ptr()), C.c_void_p(b.data_ptr())) == -3      # KNP_E_STATE
    assert "ghost" in (be.lib.knp_last_error(be.ctx) or b"").decode()
    torch.cuda.synchronize()
    assert torch.all(b == CANARY)


# ================================================================================================ 6. knp_rhs_add_load
@pytest.mark.parametrize("name", ["delaunay2d_12_cw", "delaunay3d_5"])
def test_rhs_add_load_changes_the_rows_of_one_field_and_side_only(probs, name):
    P = probs(name)
    be = P.be
    n_v = P.p.local_mesh.coords.shape[0]
    rng = np.random.default_rng(61)
    b0 = rng.uniform(-3.0, 3.0, be.n_dof_local) * 10.0 ** rng.uniform(-4.0, 4.0, be.n_dof_local)
    load = rng.uniform(-2.0, 2.0, n_v) * 10.0 ** rng.uniform(-4.0, 4.0, n_v)
    scale = -0.37
    node_of = [np.asarray(be.node_i), np.asarray(be.node_e)]
    ld = torch.from_numpy(load).to(be.device)
    for side in range(2):
        verts = np.nonzero((node_of[side] >= 0) & (node_of[side] < be.n_nodes_owned))[0]
        assert len(verts) > 0
        for field in range(4):
            b = torch.from_numpy(np.concatenate([b0, np.full(PAD, CANARY)])).to(be.device)
            assert be.lib.knp_rhs_add_load(be.ctx, field, side, scale, C.c_void_p(ld.data_ptr()), C.c_void_p(b.data_ptr())) == 0
            torch.cuda.synchronize()
            h = b.cpu().numpy()
            rows = 4 * node_of[side][verts] + field
            exact = b0[rows].astype(np.longdouble) + np.longdouble(scale) * load[verts].astype(np.longdouble)
            err = np.abs(h[rows].astype(np.longdouble) - exact)
            # one rounding of the sum, with or without one of the product (fused or not)
            assert np.all(err <= 2.0 ** -52 * (np.abs(b0[rows]) + np.abs(scale * load[verts]))), (side, field)
            assert np.any(h[rows] != b0[rows])
            rest = np.ones(be.n_dof_local, dtype=bool)
            rest[rows] = False
            assert np.array_equal(h[:be.n_dof_local][rest].view(np.int64), b0[rest].view(np.int64)) and np.all(h[be.n_dof_local:] == CANARY)


# ================================================================================================ 7. the step
def _solver(p):
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    p.solver_config["view_ksp"] = False
    return SolverKNPEMI(p, solver_config=p.solver_config)


def _assembled(s):
    """prepare and the first assembly of a run, without a solve: ``be.b`` behind ``SolverKNPEMI.assemble()``"""
    s.prepare()
    s.problem.t.value += float(s.problem.dt.value)
    s._b_is_final = False
    s.assemble()
    torch.cuda.synchronize()
    return s.backend.b.cpu().numpy().copy()


def test_the_form_path_equals_the_nodal_path(tmp_path):
    from cgx_hip import fem
    src, plain = LR.step_problems(tmp_path, steps=1)
    amp = 1e10      # see the module docstring: the source's scale becomes the row's
    f_nodal = {}
    for idx in (1, 2):
        fn = src.ion_list[idx]["f_e"]
        fn.x.array.mul_(amp)
        f_nodal[idx] = fn.numpy().copy()
    s1, s2 = _solver(src), _solver(plain)
    b_nodal = _assembled(s1)
    handles = []
    for idx, name in ((1, "K"), (2, "Cl")):
        f = fem.Function(plain.V, f"f_copy_{name}")
        FI.write(f, f_nodal[idx])
        handles.append(plain.add_source(name, expr_e=f, degree=2))
    b_form = _assembled(s2)
    be = s2.backend
    dt = float(plain.dt.value)
    node_e = np.asarray(be.node_e)
    worst = 0.0
    expected_same = np.ones(be.n_dof_local, dtype=bool)
    for idx in (1, 2):
        nodal, form, scale = LR.nodal_and_form(plain, f_nodal[idx])
        on = scale > 0
        floor = float(np.max(np.abs(nodal - form)[on] / scale[on]))
        tol = max(TOL, 8.0 * floor)
        verts = np.nonzero((node_e >= 0) & on)[0]
        rows = 4 * node_e[verts] + idx
        expected_same[rows] = False
        err = np.abs(b_nodal[rows] - b_form[rows])
        worst = max(worst, float(np.max(err / (dt * scale[verts]))))
        print(f"ion {idx}: floor {floor:.2e}, tol {tol:.1e}, {len(rows)} rows, max |b_nodal - b_form| / (dt sum |M f|) = {np.max(err / (dt * scale[verts])):.3e}")
        assert len(rows) > 0 and np.all(err <= tol * dt * scale[verts])
        assert np.all(np.abs(b_form[rows]) >= 0.5 * dt * np.abs(nodal[verts]))      # the source is in the rows, not lost beside them
    # every other row is the same assembly of the same state
    assert np.array_equal(b_nodal[expected_same].view(np.int64), b_form[expected_same].view(np.int64))
    # (c) disabling and removing restore the right-hand side of a run that never registered a source
    b_never = _assembled(_solver(LR.step_problems(tmp_path, steps=1)[1]))
    for h in handles:
        h.enabled = False
    s2._b_is_final = False
    s2.assemble()
    torch.cuda.synchronize()
    assert np.array_equal(be.b.cpu().numpy().view(np.int64), b_never.view(np.int64))
    handles[0].enabled = True
    s2.assemble()
    torch.cuda.synchronize()
    again = be.b.cpu().numpy()
    rows_k = 4 * node_e[node_e >= 0] + 1
    assert np.array_equal(again[rows_k].view(np.int64), b_form[rows_k].view(np.int64)) and not np.array_equal(again, b_form)
    for h in handles:
        h.remove()
    assert not plain._sources
    s2.assemble()
    torch.cuda.synchronize()
    assert np.array_equal(be.b.cpu().numpy().view(np.int64), b_never.view(np.int64))


def _total_k(p):
    return math.fsum(p.ion_budget()["K"])


def test_a_time_switched_source_is_conserved(tmp_path):
    """K summed over all tags rises by R dt per step with the source on and not before; the defect is held to 10 x the defect of
    the nodal ``ion_injection`` run over the same steps (both are bounded by the linear solve's residual).

    The rise is taken against a third run of the same steps without any source.  The KNP-EMI scheme does not conserve one ion
    on its own: the capacitive current is split among the ions with each side's own fractions alpha_k, so while phi_m moves the
    total of K drifts (here by -3.1e-16 mol per step, 240 times R dt, the same in all three runs); only what a source adds to
    that is R dt.  Measured on MI355X: see DESIGN.md section 14."""
    from cgx_hip import fem
    src, plain = LR.step_problems(tmp_path, steps=3)
    none = LR.step_problems(tmp_path, steps=3)[1]
    dt = float(plain.dt.value)
    # the rate of the nodal run: int over the extracellular cells of the P1 function f_e, from the host restatement
    nodal, _, _ = LR.nodal_and_form(plain, src.ion_list[1]["f_e"].numpy())
    R = math.fsum(nodal)
    assert R > 0
    rise = {}
    for key, p in (("none", none), ("nodal", src), ("form", plain)):
        s = _solver(p)
        s.prepare()
        if key == "form":
            budget = p.ion_budget()
            ext = np.nonzero(budget["side"] == 1)[0]
            assert len(ext) == 1
            V = float(budget["volume"][ext[0]])
            t_on = 1.5 * dt      # between the steps 1 and 2
            h = p.add_source("K", expr_e=fem.conditional(fem.ge(p.t, t_on), R / V, 0.0), tags=[int(budget["tag"][ext[0]])], degree=1)
        k0 = _total_k(p)
        r = []
        for i in (1, 2, 3):
            assert s.step(i) is not False
            r.append(_total_k(p) - k0)
        rise[key] = np.array(r)
        assert all(x > 0 for x in s.reasons)
    added_n, added_f = rise["nodal"] - rise["none"], rise["form"] - rise["none"]
    want_n = R * dt * np.array([1.0, 2.0, 3.0])
    want_f = R * dt * np.array([0.0, 1.0, 2.0])
    defect_n, defect_f = float(np.max(np.abs(added_n - want_n))), float(np.max(np.abs(added_f - want_f)))
    print(f"K total {k0:.6e} mol, drift without a source {rise['none']}, R dt = {R * dt:.6e} mol per step; defect nodal {defect_n:.3e}, "
          f"defect form {defect_f:.3e} mol (relative to R dt: {defect_n / (R * dt):.3e}, {defect_f / (R * dt):.3e}); added form {added_f}, "
          f"nodal {added_n}")
    assert defect_n < 0.01 * R * dt                              # today's path does add R dt per step: the yardstick measures something
    assert abs(added_f[0]) <= 10.0 * defect_n                    # not before
    assert added_f[1] > 0.5 * R * dt and added_f[2] > 1.5 * R * dt
    assert defect_f <= 10.0 * defect_n
    h.remove()


def test_a_membrane_source_adds_dt_c_times_the_facets_share(tmp_path):
    from cgx_hip import fem
    plain = LR.step_problems(tmp_path, steps=1)[1]
    s = _solver(plain)
    b0 = _assembled(s)
    c = -3.25e-3
    tags = [int(plain.gamma_tags[0]), int(plain.gamma_tags[2])]
    h = plain.add_membrane_source("phi", "i", fem.Constant(plain.mesh, c), tags=tags)
    s.assemble()
    torch.cuda.synchronize()
    be = s.backend
    b1 = be.b.cpu().numpy()
    dt, d = float(plain.dt.value), plain.local_mesh.coords.shape[1]
    fv, meas = np.asarray(plain._fv), np.asarray(plain._fmeas)
    sel = np.isin(np.asarray(plain.gamma_facet_tags), tags)
    share = np.zeros(plain.local_mesh.coords.shape[0])
    np.add.at(share, fv[sel].ravel(), np.repeat(meas[sel] / d, d))
    verts = np.nonzero(share > 0)[0]
    node_i = np.asarray(be.node_i)
    assert len(verts) > 0 and np.all(node_i[verts] >= 0) and 0 < sel.sum() < len(sel)
    rows = 4 * node_i[verts] + 3
    want = dt * c * share[verts]
    # to the tolerance of item 1 (a constant: TOL) of the source's scale, and one rounding of the row it is added to
    err = np.abs((b1[rows] - b0[rows]) - want)
    print(f"membrane source: max |delta b - dt c |F| / d| / scale = {np.max(err / np.abs(want)):.3e}; rounding of the row {np.max(2.0 ** -52 * np.abs(b1[rows]) / np.abs(want)):.3e}")
    assert np.all(err <= TOL * np.abs(want) + 2.0 ** -52 * (np.abs(b0[rows]) + np.abs(b1[rows])))
    rest = np.ones(len(b0), dtype=bool)
    rest[rows] = False
    assert np.array_equal(b1[rest].view(np.int64), b0[rest].view(np.int64)) and np.all(b1[rows] != b0[rows])
    h.remove()
