"""The owned/ghost paths of the kernels, operator by operator, on rank pieces of the irregular meshes (tests/rank_pieces.py; the
preconditions, with the teeth, in tests/test_rank_pieces_host.py).  Every other operator-level GPU test runs where
``n_nodes_owned == n_nodes``; the code that tells owned from ghost ran only in multi-process end-to-end solves checked at 1e-6.

ONE process builds the context of one rank's piece (``make_problem(cfg, models, local_mesh)``; ``Backend`` installs communication hooks
only when ``comm.size > 1``) and every operator is compared with the oracle on the WHOLE mesh through ``l2g``.  Where a kernel needs
an exchange the test installs its own hooks with ``knp_set_comm``: a halo hook that writes the ghost entries, an identity all-reduce.

Tolerances are those of the test of the same operator on whole meshes, named at each test.  MEASURED lists what the MI355X gave.

MEASURED on an MI355X (largest over the cases; tolerance; the test it is borrowed from)
  a. layout: exact.  max_node_pairs is the maximum over the owned nodes of the piece's graph.
  b. A 4.3e-15, second assembly 4.0e-15, P 4.3e-15, owned block of P 4.3e-15 of the largest entry (1e-12); b 2.4e-15, per field block
     2.4e-15 (1e-12, 1e-10; test_gpu_irregular.test_layout_operators_and_launch_path).  knp_assemble_rhs leaves b[n_dof_owned:] untouched
     (now said in the header).  Assembly variants on a 2D and a 3D piece: the bits of the default, unstaged 8.2e-17 (1e-15;
     test_assembly_variants_write_the_same_bits).
  c. SpMV 6.4e-15 of (|A||x|)_i at the library's width and at 4, 8, 16, 32 lanes (1e-12;
     test_spmv_rowwise_at_every_lane_width); y[n_dof_owned:] keeps the sentinel; through a halo hook: one call, the same bits.
  d. knp_l2_norms: the pieces' squared norms against the whole mesh 2.7e-15 (1e-12; test_gpu_functionals.
     test_against_the_norm_and_budget_kernels).  knp_nullspace_test 6.9e-25 where 1e-10 max|A| = 1.1e-18, and with
     zeroed ghosts 1.9e-17 of the row-wise bound against NumPy with the owned count (1e-12); knp_project_nullspace 3.6e-17
     (1e-13; test_spmv_rowwise_at_every_lane_width).  Never read, poisoned with NaN, results finite: knp_l2_norms -- the potentials at
     vertices of no owned cell; knp_project_nullspace -- v[n_dof_owned:] (still NaN afterwards); knp_pc_apply with vertex-block
     Jacobi -- r[n_dof_owned:]; knp_spmv reads x[n_dof_owned:] after the hook (NaN before it).  knp_nullspace_test builds its own vector.
  e. knp_unpack / knp_pack: NumPy indexing bit for bit, ghost vertices and ghost nodes included.  With the unpack target registered
     and a last cycle of at most 8 columns (restart 8; and 98 = 3 * 32 + 2 in g) fused_tails is 1 on the whole mesh and 0 on the piece,
     where the fields are untouched by the solve and knp_unpack then writes them, ghost vertices included, bit for bit.
  f. vertex-block Jacobi: worst block residual 2.7e-12 (rtol 1e-9; test_pc_apply_vbjacobi_inverts_vertex_blocks_at_the_hub), on the piece
     that owns the hub and on the one that sees it as a ghost.  hypre and btcc on piece 0 of delaunay2d_24 cut in 2 (hierarchies of
     4 levels, btcc 4 and 3, from own_block; the pieces of the other cuts are too small for three): hypre 6.1e-16, btcc 2.7e-15 of the NumPy
     cycle with fp64 and fused fp32 storage, btcc level by level with fp32 storage 1.4e-10 (1e-10, 2e-6; test_pc_apply_against_the_numpy_cycle), fused, KNP_BLOCKED=0, KNP_FUSED=0, library width and 16 lanes.
     z[n_dof_owned:] is never written.
  g. gmres / fgmres on A_oo x = b_o, restart 32, 98 / 80 and 60 / 52 iterations: against sparse LU concentrations 6.7e-10 (1e-7), potential
     2.8e-9 (1e-6; test_two_steps_match_direct_solves); true residual of the flexible solve 9.9e-10 (1.05e-9;
     test_flexible_gmres_reaches_the_true_residual).  With hooks: 1.05 halo calls and 1.05 all-reduce calls per iteration, equal to the
     library's counters; without: the same counts, and the flexible driver folds the first reduction stage into 27 / 18 of its SpMVs.
  h. two-tag mesh cut in 2: ion amounts 1.8e-15 (rtol 1e-12), fluxes 1.0e-16 of S, membrane potential 3.5e-17 of S (1e-12;
     test_per_tag_diagnostics_on_cells_and_facets_of_many_sizes), stimulus integral 1.1e-16 (rtol 1e-12); sums over the pieces against the
     host and against the GPU on the whole mesh 6.7e-16, 5.4e-17, 3.5e-17, 0.  Piece 1, tag 2: ten facets seen, none owned: zeros and
     (0, +inf, -inf).
  i. two ranks, native exchange with and without the row split, hooks: 4.9e-15 of (|A||x|)_i each (1e-12), per rank the same bits.  The library does not
     export its row lists: that the split launch ran is inferred from p2p_on, from ghost entries of x that were NaN before the call,
     and from the host's restatement of the rule of knp_create (108 / 104 interior, 15 / 15 boundary nodes); agreement of the legs alone
     would also be seen if every leg took the unsplit path.  Wall time 11.3 s for the three legs, test_ranks_on_one_gpu_match_oracle[2-p2p] 5.7 s.
"""
import dataclasses
import os

import numpy as np
import pytest
import torch

import irregular_meshes as IM
import rank_pieces as RP

pytestmark = pytest.mark.gpu

WIDTHS = [4, 8, 16, 32]
SENTINEL = -7.25e300
# forced lane widths and hooks: the piece that owns the hub, the one that sees it as a ghost, a 3D piece, the piece with more ghosts than owned
FOUR = [("hub2d_12_48m", 1), ("hub2d_12_48m", 0), ("delaunay3d_5", 1), ("hub3d_5_60", 0)]


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _maxdiff(A, B):
    D = (A - B).tocoo()
    return np.abs(D.data).max() if D.nnz else 0.0


@dataclasses.dataclass
class Piece:
    name: str
    rank: int
    lm: object
    og: object          # oracle on the whole mesh
    ol: object          # oracle on the piece (layout, local pattern)
    p: object
    be: object
    l2gd: np.ndarray    # global dof of every local dof
    n_own: int

    @property
    def own(self):
        return self.l2gd[:self.n_own]

    def dev(self, a):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=self.be.device)


def _piece(tmp_path, name, rank, og=None, cfg=None):
    lm = RP.cut_piece(name, rank)
    og = og or RP.global_oracle(name)
    ol = RP.piece_oracle(lm, og)
    p = RP.make_piece_problem(tmp_path, name, lm, og, cfg=cfg)
    be = p.create_backend()
    assert p.comm.size == 1 and not hasattr(be, "_halo_cb")
    return Piece(name, rank, lm, og, ol, p, be, RP.global_maps(lm, ol, og), 4 * RP.n_nodes_owned(lm, ol))


@pytest.fixture(scope="module")
def globals_():
    """A, b, P of the whole mesh, once per mesh"""
    cache = {}

    def get(name):
        if name not in cache:
            og = RP.global_oracle(name)
            cache[name] = (og.assemble_A().tocsr(), og.assemble_b(), og.assemble_P().tocsr())
        return cache[name]
    return get


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """One context per (cut, rank) with the library's own launch choices and the matrix assembled.  Shared by the tests that only
    read: none of them assembles again, writes a field or installs a hook."""
    cache = {}
    tmp = tmp_path_factory.mktemp("pieces")

    def get(name, rank):
        if (name, rank) not in cache:
            assert not [k for k in os.environ if k.startswith(("KNP_SPMV", "KNP_ASM", "KNP_PC_GROUP"))], "a shared context is built without switches"
            c = _piece(tmp, name, rank)
            c.be.assemble_matrix()
            cache[(name, rank)] = c
        return cache[(name, rank)]
    return get


class Hooks:
    """``knp_set_comm`` on a piece's context: the halo hook writes ``ghost`` (a device tensor, or None: leave them) into the ghost
    entries on the context's stream, the all-reduce is the identity.  Calls are counted; the ctypes callbacks live as long as this."""

    def __init__(self, be, ghost=None):
        from cgx_hip import _lib
        from cgx_hip.parallel import guarded
        self.halo_calls = self.ar_calls = 0
        self.ghost = ghost
        idx = torch.arange(be.n_dof_owned, be.n_dof_local, device=be.device)

        def halo(user, xptr):
            self.halo_calls += 1
            if self.ghost is not None:
                be._view(xptr, be.n_dof_local).index_copy_(0, idx, self.ghost)

        def allreduce(user, ptr, n):
            self.ar_calls += 1
        self._cb = (_lib.HALO_FN(guarded(halo)), _lib.ALLREDUCE_FN(guarded(allreduce)))
        be.check(be.lib.knp_set_comm(be.ctx, self._cb[0], self._cb[1], None))
        be._test_hooks = self


# ---- a, b. layout, matrix, right-hand side, P ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rank", RP.PIECES)
def test_layout_and_operators_of_a_piece(name, rank, tmp_path, globals_):
    """test_gpu_irregular.test_layout_operators_and_launch_path on a piece: owned rows, local columns, against the rows of the whole
    mesh (A, P: 1e-12 of the largest entry; b: 1e-12, per field block 1e-10), stimulus on, and again after other fields."""
    c = _piece(tmp_path, name, rank)
    be, ol, og = c.be, c.ol, c.og
    Ag, bg, Pg = globals_(name)
    no = c.n_own // 4
    # layout: owned nodes first, the numbering of the oracle on the piece
    assert be.n_nodes_owned == no and be.n_dof_owned == c.n_own < be.n_dof_local == ol.n_dof and be.n_nodes == ol.lay.n_nodes
    assert np.array_equal(be.node_i, ol.lay.node_i.astype(np.int32)) and np.array_equal(be.node_e, ol.lay.node_e.astype(np.int32))
    nvo = c.lm.n_vertices_owned
    for nodes in (be.node_i, be.node_e):
        assert nodes[:nvo].max() < no and (nodes[nvo:][nodes[nvo:] >= 0] >= no).all()
    info = be.launch_info()
    assert info["max_node_pairs"] == IM.graph_stats(ol)["pairs"][:no].max(), info
    be.assemble_matrix()
    A = be.csr()
    assert A.shape == (c.n_own, ol.n_dof)
    dA = _maxdiff(RP.to_global_columns(A, c.l2gd, og.n_dof), Ag[c.own]) / np.abs(Ag.data).max()
    be.b.fill_(SENTINEL)
    be.assemble_rhs()
    b = be.b.cpu().numpy()
    assert np.all(b[c.n_own:] == SENTINEL)                              # knp_assemble_rhs: the ghost entries of b are not written
    b, bo = b[:c.n_own], bg[c.own]
    db = [_rel(b[f::4], bo[f::4]) for f in range(4)]
    be.assemble_precond()
    P = be.precond_csr()
    dP = _maxdiff(RP.to_global_columns(P, c.l2gd, og.n_dof), Pg[c.own]) / np.abs(Pg.data).max()
    dPo = _maxdiff(P[:, :c.n_own].tocsr(), Pg[c.own][:, c.own]) / np.abs(Pg.data).max()      # own_block of solver.py
    print(f"ERR a/b {name} piece {rank}: A {dA:.2e}  b {_rel(b, bo):.2e} {db}  P {dP:.2e}  own block {dPo:.2e}")
    assert dA <= 1e-12 and dP <= 1e-12 and dPo <= 1e-12
    assert _rel(b, bo) <= 1e-12 and all(d <= 1e-10 for d in db)
    # second assembly, other fields (the second state of test_layout_operators_and_launch_path, on the whole mesh, through l2g)
    o2 = IM.oracle(name)
    IM.perturb(o2)
    X = o2.coords / o2.coords.max()
    s2 = 1.0 + 0.08 * np.cos(2.0 * X[:, 0] - 0.3) * np.sin(3.0 * X[:, 1] + 0.2)
    for side in range(2):
        for j in range(3):
            o2.k[side][j] = o2.k[side][j] * (s2 if (side + j) % 2 else 2.0 - s2)
            c.p.wh[side][j].x.array[:] = c.dev(o2.k[side][j][c.lm.l2g])
    be.assemble_matrix()
    A2g = o2.assemble_A().tocsr()
    dA2 = _maxdiff(RP.to_global_columns(be.csr(), c.l2gd, og.n_dof), A2g[c.own]) / np.abs(A2g.data).max()
    print(f"ERR b {name} piece {rank}: A second {dA2:.2e}")
    assert dA2 <= 1e-12 and _maxdiff(A2g, Ag) > 1e-6 * np.abs(Ag.data).max()


@pytest.mark.parametrize("name", ["hub2d_12_48m", "delaunay3d_5", "hub3d_5_60", "hub2d_12_48m_cw"])
def test_owned_unknowns_of_a_cut_add_up(name, cases):
    size, _ = RP.CUTS[name]
    assert sum(cases(name, r).be.n_dof_owned for r in range(size)) == RP.global_oracle(name).n_dof


def _assembled(tmp_path, name, rank):
    c = _piece(tmp_path, name, rank)
    c.be.assemble_matrix()
    c.be.assemble_precond()
    return c.be.csr(), c.be.precond_csr(), c.be.launch_info()


@pytest.mark.parametrize("name,rank", [("hub2d_12_48m", 1), ("delaunay3d_5", 0)])
def test_assembly_variants_write_the_same_bits_on_a_piece(name, rank, tmp_path, monkeypatch):
    """the switches and assertions of test_gpu_irregular.test_assembly_variants_write_the_same_bits"""
    A1, P1, i1 = _assembled(tmp_path, name, rank)
    monkeypatch.setenv("KNP_ASM_FUSED_MEANS", "0")
    Af, Pf, inf = _assembled(tmp_path, name, rank)
    monkeypatch.delenv("KNP_ASM_FUSED_MEANS")
    assert i1["asm_dmax"] > 0 and inf["asm_dmax"] == 0 and inf["asm_variant"] == i1["asm_variant"], (i1, inf)
    monkeypatch.setenv("KNP_ASM_TRANSPOSED", "0")
    A2, P2, i2 = _assembled(tmp_path, name, rank)
    monkeypatch.setenv("KNP_ASM_STAGE", "0")
    A3, P3, i3 = _assembled(tmp_path, name, rank)
    assert i2["asm_variant"] == 1 and i3["asm_variant"] == 0 and i3["asm_stage"] == 0
    print(f"ERR b {name} piece {rank} {i1}: plain vs staged: A", np.abs(A3.data - A1.data).max() / np.abs(A1.data).max(),
          "P", np.abs(P3.data - P1.data).max() / np.abs(P1.data).max())
    for M, M1 in ((Af, A1), (Pf, P1), (A2, A1), (P2, P1)):
        assert np.array_equal(M.indices, M1.indices) and np.array_equal(M.data, M1.data)
    assert np.array_equal(A3.indices, A1.indices) and np.abs(A3.data - A1.data).max() <= 1e-15 * np.abs(A1.data).max()
    assert np.array_equal(P3.indices, P1.indices) and np.abs(P3.data - P1.data).max() <= 1e-15 * np.abs(P1.data).max()


# ---- c. SpMV -------------------------------------------------------------------------------------------------------------------------
def _spmv(c, Ag, what, x_ghost="global"):
    """row by row, |y - (A_g x_g)[owned]|_i <= 1e-12 (|A_g| |x_g|)_i (the bound of test_spmv_rowwise_at_every_lane_width); the ghost
    entries of y keep what they held.  Returns y (owned) as the device wrote it."""
    xg = np.random.default_rng(0).standard_normal(c.og.n_dof)
    x = xg[c.l2gd].copy()
    if x_ghost == "nan":
        x[c.n_own:] = np.nan
    xt = c.dev(x)
    yt = torch.full_like(xt, SENTINEL)
    c.be.spmv(xt, yt)
    y = yt.cpu().numpy()
    assert np.all(y[c.n_own:] == SENTINEL)
    err = np.abs(y[:c.n_own] - (Ag @ xg)[c.own])
    bound = (abs(Ag) @ np.abs(xg))[c.own]
    print(f"ERR c {what}: SpMV max err / bound = {(err / bound).max():.3e}")
    assert np.all(np.isfinite(y[:c.n_own])) and np.all(err <= 1e-12 * bound)
    return y[:c.n_own], xg


@pytest.mark.parametrize("name,rank", RP.PIECES)
def test_spmv_rowwise_on_a_piece(name, rank, cases, globals_):
    c = cases(name, rank)
    info = c.be.launch_info()
    _spmv(c, globals_(name)[0], f"{name} piece {rank} G={info['spmv_group']} trips={-(-info['max_node_pairs'] // (2 * info['spmv_group']))}")


@pytest.mark.parametrize("G", WIDTHS)
@pytest.mark.parametrize("name,rank", FOUR)
def test_spmv_rowwise_on_a_piece_at_every_lane_width(name, rank, G, tmp_path, monkeypatch, globals_):
    monkeypatch.setenv("KNP_SPMV", str(G))
    c = _piece(tmp_path, name, rank)
    c.be.assemble_matrix()
    info = c.be.launch_info()
    assert info["spmv_group"] == G and info["spmv_unroll"] == 2
    _spmv(c, globals_(name)[0], f"{name} piece {rank} G={G} trips={-(-info['max_node_pairs'] // (2 * G))}")


@pytest.mark.parametrize("name,rank", FOUR)
def test_spmv_calls_the_halo_hook_once_and_reads_what_it_wrote(name, rank, tmp_path, globals_):
    """ghost entries NaN until the hook fills them on the context's stream: one call per knp_spmv, the bits of the pre-filled run"""
    c = _piece(tmp_path, name, rank)
    c.be.assemble_matrix()
    y0, xg = _spmv(c, globals_(name)[0], f"{name} piece {rank} pre-filled")
    h = Hooks(c.be, ghost=c.dev(xg[c.l2gd[c.n_own:]]))
    halos0 = c.be.stats()["halos"]
    y1, _ = _spmv(c, globals_(name)[0], f"{name} piece {rank} through the hook", x_ghost="nan")
    assert h.halo_calls == 1 == c.be.stats()["halos"] - halos0 and h.ar_calls == 0
    assert np.array_equal(y0, y1)


# ---- d, e. reductions over owned entries; pack and unpack with ghosts -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["hub2d_12_48m", "delaunay3d_5"])
def test_l2_norms_of_the_pieces_add_up_and_fields_round_trip(name, tmp_path):
    """knp_l2_norms (k_l2 over the owned cells): the pieces' squared norms sum to the P1 formula on the whole mesh, 1e-12 (TOL of
    test_gpu_functionals.test_against_the_norm_and_budget_kernels); vertices of no owned cell are never read (NaN there).
    knp_unpack / knp_pack against NumPy indexing, bit for bit, ghost vertices and ghost nodes included."""
    size, _ = RP.CUTS[name]
    og = RP.global_oracle(name)
    X = og.coords / og.coords.max()
    phi = [np.cos(3.0 * X[:, 0]) + 0.5 * X[:, 1], np.sin(2.0 * X[:, 1]) - 0.7 * X[:, 0] + 2.0]
    want = [og.l2_norm(phi[s], s) ** 2 for s in range(2)]
    got = np.zeros(2)
    for r in range(size):
        c = _piece(tmp_path, name, r)
        be, p, lm = c.be, c.p, c.lm
        # e. unpack a local vector with other values in the ghost entries than anywhere else, pack it back
        x = np.random.default_rng(4).standard_normal(be.n_dof_local)
        be.x.copy_(c.dev(x))
        be.unpack()
        for side, nodes in ((0, be.node_i), (1, be.node_e)):
            has = nodes >= 0
            for f in range(4):
                expect = np.where(has, x[4 * np.maximum(nodes, 0) + f], 0.0)
                assert np.array_equal(p.wh[side][f].numpy(), expect), (r, side, f)
        pi, pe = p.wh[0][3].numpy(), p.wh[1][3].numpy()
        assert np.array_equal(p.phi_m_prev.numpy(), pi - pe)
        assert (be.node_i[lm.n_vertices_owned:] >= 0).any() or (be.node_e[lm.n_vertices_owned:] >= 0).any()
        be.x.fill_(SENTINEL)
        be.pack()
        assert np.array_equal(be.x.cpu().numpy(), x)
        # d. the norms: potentials of the whole mesh through l2g, NaN at the vertices no owned cell has
        seen = np.zeros(lm.coords.shape[0], dtype=bool)
        seen[lm.cells[:lm.n_cells_owned].ravel()] = True
        assert not seen.all()
        for s in range(2):
            v = phi[s][lm.l2g].copy()
            v[~seen] = np.nan
            p.wh[s][3].x.array[:] = c.dev(v)
        ni, ne = be.l2_norms_sq()
        assert np.isfinite(ni) and np.isfinite(ne)
        ref = [RP.l2_sq(c.ol, np.nan_to_num(phi[s][lm.l2g]), s, lm.n_cells_owned) for s in range(2)]
        assert abs(ni - ref[0]) <= 1e-12 * ref[0] and abs(ne - ref[1]) <= 1e-12 * ref[1]
        got += (ni, ne)
    d = np.abs(got / want - 1.0)
    print(f"ERR d {name}: sum of the pieces' squared norms against the whole mesh {d}")
    assert np.all(d <= 1e-12)


def test_n_cells_owned_outside_its_range_means_all_cells():
    """include/knpemi_hip.h, knp_mesh_desc, through the raw ABI (a ``MeshDesc`` built by hand, as
    test_gpu_parity.test_mesh_validation_in_knp_create): n_cells_owned <= 0 or > n_cells reads as n_cells.  The same piece described with
    its count integrates its owned cells in knp_l2_norms, described with 0, -1 or n_cells + 1 its ghost cells too (1e-12, as in d)."""
    import ctypes as C
    from cgx_hip import _lib
    from cgx_hip import mesh as meshmod
    from cgx_hip._lib import MeshDesc
    lib = _lib.load()
    name, rank = "hub2d_12_48m", 1
    lm = RP.cut_piece(name, rank)
    og = RP.global_oracle(name)
    ol = RP.piece_oracle(lm, og)
    coords = np.ascontiguousarray(lm.coords, dtype=np.float64)
    cells = np.ascontiguousarray(lm.cells, dtype=np.int32)
    side = np.ascontiguousarray(ol.cell_side, dtype=np.uint8)
    qp, qw = meshmod.facet_quadrature(2, 10)
    qp, qw = np.ascontiguousarray(qp, dtype=np.float64), np.ascontiguousarray(qw, dtype=np.float64)
    X = og.coords / og.coords.max()
    phi = [np.cos(3.0 * X[:, 0])[lm.l2g] + 2.0, np.sin(2.0 * X[:, 1])[lm.l2g] + 2.0]
    dev = torch.device("cuda", torch.cuda.current_device())
    pt = [torch.as_tensor(v, device=dev) for v in phi]
    torch.cuda.synchronize()
    nc, nco = cells.shape[0], int(lm.n_cells_owned)
    assert 0 < nco < nc
    got = {}
    for given in (nco, 0, -1, nc + 1, nc):
        d = MeshDesc(dim=2, n_vertices=coords.shape[0], n_vertices_owned=lm.n_vertices_owned, n_cells=nc, n_cells_owned=given,
                     cells=cells.ctypes.data_as(_lib.i32p), coords=coords.ctypes.data_as(_lib.f64p),
                     cell_side=side.ctypes.data_as(_lib.u8p), n_gamma=0, gamma=None, gamma_prog=None,
                     n_q=qw.shape[0], q_pts=qp.ctypes.data_as(_lib.f64p), q_w=qw.ctypes.data_as(_lib.f64p))
        ctx = C.c_void_p()
        rc = lib.knp_create(C.byref(ctx), C.byref(d))
        assert rc == 0, lib.knp_last_error(ctx)
        out = (C.c_double * 2)()
        rc = lib.knp_l2_norms(ctx, C.c_void_p(pt[0].data_ptr()), C.c_void_p(pt[1].data_ptr()), out)
        assert rc == 0, lib.knp_last_error(ctx)
        got[given] = (out[0], out[1])
        lib.knp_destroy(ctx)
    for given, n_ref in ((nco, nco), (0, nc), (-1, nc), (nc + 1, nc), (nc, nc)):
        for s in range(2):
            ref = RP.l2_sq(ol, phi[s], s, n_ref)
            assert abs(got[given][s] - ref) <= 1e-12 * ref, (given, s, got[given][s], ref)
    assert got[0][0] > (1 + 1e-6) * got[nco][0] and got[0][1] > (1 + 1e-6) * got[nco][1]


@pytest.mark.parametrize("name,rank", FOUR)
def test_nullspace_kernels_reduce_over_owned_nodes(name, rank, tmp_path):
    """knp_nullspace_test and knp_project_nullspace with an identity all-reduce (test_spmv_rowwise_at_every_lane_width: 1e-10 of the
    largest entry; 1e-13): the count and the sum run over the owned potential unknowns, the ghost entries of v are neither read nor
    written (NaN before and after).  ||A ns|| with the ghosts in place is rounding noise whatever the normalisation, so the test runs
    once more with a halo hook that zeroes the ghost entries: then ||A ns|| = ||A[:, owned] ns_owned|| is of the size of the entries
    of A, and it is compared with NumPy on the exported rows with ns = 1 / sqrt(owned potential unknowns), within the row-wise SpMV
    bound 1e-12 || |A| |ns| ||."""
    c = _piece(tmp_path, name, rank)
    be = c.be
    be.assemble_matrix()
    h = Hooks(be)
    A = be.csr()
    no = c.n_own // 4
    ns = np.zeros(be.n_dof_local)
    ns[3::4] = 1.0 / np.sqrt(no)
    t = be.nullspace_test()
    ref = np.linalg.norm(A @ ns)
    print(f"ERR d {name} piece {rank}: nullspace test {t:.3e} (NumPy on the exported rows {ref:.3e}), 1e-10 max|A| = {1e-10 * np.abs(A.data).max():.3e}")
    assert t <= 1e-10 * np.abs(A.data).max() and h.halo_calls == 1 and h.ar_calls >= 1
    h.ghost = torch.zeros(be.n_dof_local - c.n_own, dtype=torch.float64, device=be.device)
    t0 = be.nullspace_test()
    ns0 = ns.copy()
    ns0[c.n_own:] = 0.0
    ref0, bound0 = np.linalg.norm(A @ ns0), np.linalg.norm(abs(A) @ np.abs(ns0))
    wrong = ref0 * np.sqrt(no / (be.n_dof_local // 4))                   # what a count over the local potential unknowns would give
    print(f"ERR d {name} piece {rank}: nullspace test with zeroed ghosts {t0:.6e}, NumPy {ref0:.6e}, |diff| / bound {abs(t0 - ref0) / bound0:.2e}; "
          f"with the local count it would be {wrong:.6e}")
    assert ref0 > 1e-3 * np.abs(A.data).max() and abs(wrong - ref0) > 1e-2 * ref0
    assert abs(t0 - ref0) <= 1e-12 * bound0 and h.halo_calls == 2
    h.ghost = None
    v = np.random.default_rng(2).standard_normal(be.n_dof_local)
    v[c.n_own:] = np.nan
    vt = c.dev(v)
    be.project_nullspace(vt)
    out = vt.cpu().numpy()
    want = v[:c.n_own].copy()
    want[3::4] -= v[:c.n_own][3::4].sum() / no
    d = _rel(out[:c.n_own], want)
    print(f"ERR d {name} piece {rank}: projection {d:.2e}")
    assert np.all(np.isnan(out[c.n_own:])) and np.all(np.isfinite(out[:c.n_own])) and d <= 1e-13
    assert np.array_equal(out[:c.n_own].reshape(-1, 4)[:, :3], v[:c.n_own].reshape(-1, 4)[:, :3])


# ---- f. preconditioner application on a piece -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rank", [("hub2d_12_48m", 1), ("hub2d_12_48m", 0), ("hub3d_5_60", 0)])
def test_pc_apply_vbjacobi_inverts_the_owned_vertex_blocks(name, rank, tmp_path):
    """test_gpu_irregular.test_pc_apply_vbjacobi_inverts_vertex_blocks_at_the_hub on the piece that owns the hub and on one that sees it
    as a ghost: z solves the owned vertex blocks of A; the ghost entries of r are never read (NaN), those of z never written."""
    c = _piece(tmp_path, name, rank)
    be, ol = c.be, c.ol
    be.assemble_matrix()
    be.pc_setup(1)
    A = be.csr().tocsr()
    no = c.n_own // 4
    r = np.random.default_rng(1).standard_normal(be.n_dof_local)
    r[c.n_own:] = np.nan
    zt = torch.full((be.n_dof_local,), SENTINEL, dtype=torch.float64, device=be.device)
    be.pc_apply(c.dev(r), zt)
    z = zt.cpu().numpy()
    assert np.all(z[c.n_own:] == SENTINEL) and np.all(np.isfinite(z[:c.n_own]))
    grp = ol.lay.node_vertex[:no]
    assert grp.max() < c.lm.n_vertices_owned
    starts = np.nonzero(np.r_[True, grp[1:] != grp[:-1]])[0]
    sizes = np.diff(np.r_[starts, no])
    assert sizes.max() == 2
    hub = np.nonzero(c.lm.l2g == IM.hub_vertex(IM.mesh(name)[0], RP.HUB[name]))[0][0]
    assert (hub < c.lm.n_vertices_owned) == ((name, rank) != ("hub2d_12_48m", 0))      # piece 0 of the 2D cut sees the hub as a ghost
    worst = 0.0
    for s, sz in zip(starts, sizes):
        idx = np.arange(4 * s, 4 * (s + sz))
        blk = A[idx][:, idx].toarray()
        worst = max(worst, np.abs(blk @ z[idx] - r[idx]).max() / np.abs(r[idx]).max())
        assert np.allclose(blk @ z[idx], r[idx], rtol=1e-9, atol=1e-12 * np.nanmax(np.abs(r)))
    print(f"ERR f {name} piece {rank}: vbjacobi worst block residual {worst:.2e}")


# ---- g. both Krylov drivers with n != ldv -----------------------------------------------------------------------------------------------
RESTART = 32        # krylov_cases.MS


@pytest.mark.parametrize("hooks", [True, False])
@pytest.mark.parametrize("name,rank", [("hub2d_12_48m", 1), ("hub3d_5_60", 0)])
def test_krylov_drivers_solve_the_owned_block(name, rank, hooks, tmp_path):
    """gmres and fgmres on a piece whose ghost entries stay zero solve A_oo x = b_o (n = n_dof_owned, ldv = n_dof_local in every Krylov
    kernel), null-space projection off, vertex-block Jacobi.  With hooks (a halo hook that zeroes the ghosts, an identity all-reduce)
    the reductions finish in k_reduce_partials + all-reduce, without them in the single-block finish.  Against the host sparse LU of
    the exported block: concentrations rtol 1e-7, potential 1e-6 of its largest entry (test_gpu_irregular.test_two_steps_match_direct_solves,
    solved to its rtol 1e-13); the true residual of the flexible solve at rtol 1e-9 within MARGIN
    (test_flexible_gmres_reaches_the_true_residual)."""
    import scipy.sparse.linalg as spla
    import krylov_cases as KC
    from test_gpu_fgmres import MARGIN
    assert RESTART in KC.MS
    c = _piece(tmp_path, name, rank)
    be, n = c.be, c.n_own
    be.assemble_matrix()
    be.assemble_rhs()
    be.b[n:] = 0.0
    be.set_nullspace(False)
    be.pc_setup(1)
    be.fields_out()                                                        # registers the unpack target, as Backend.unpack() does
    h = Hooks(be, ghost=torch.zeros(be.n_dof_local - n, dtype=torch.float64, device=be.device)) if hooks else None
    Aoo = be.csr()[:, :n].tocsc()
    b = be.b.cpu().numpy()[:n]
    xlu = spla.splu(Aoo).solve(b)
    assert np.linalg.norm(b - Aoo @ xlu) <= 1e-12 * np.linalg.norm(b)
    for driver, rtol in (("gmres", 1e-13), ("fgmres", 1e-9)):
        be.x.zero_()
        st0 = be.stats()
        calls0 = (h.halo_calls, h.ar_calls) if hooks else (0, 0)
        its, rn, reason = getattr(be, driver)(rtol, 1e-50, 5000, RESTART)
        if driver == "gmres":
            its_left = its
        st = be.stats()
        x = be.x.cpu().numpy()
        assert np.all(x[n:] == 0.0) and np.all(be.b.cpu().numpy()[n:] == 0.0)
        x = x[:n]
        true = np.linalg.norm(b - Aoo @ x) / np.linalg.norm(b)
        dk = max(np.max(np.abs(x[f::4] / xlu[f::4] - 1.0)) for f in range(3))
        dphi = np.abs(x[3::4] - xlu[3::4]).max() / np.abs(xlu[3::4]).max()
        halos, ars = st["halos"] - st0["halos"], st["allreduces"] - st0["allreduces"]
        folded = st["spmv_dots"] - st0["spmv_dots"]      # flexible GMRES without hooks: SpMVs with the reduction's first stage (k_spmv_node_dots)
        print(f"ERR g {name} piece {rank} {driver} hooks={hooks}: its {its} reason {reason} true residual {true:.2e} k {dk:.2e} phi {dphi:.2e}; "
              f"halo exchanges {halos} ({halos / its:.3f} per iteration), reductions {ars} ({ars / its:.3f} per iteration), SpMVs with folded dots {folded}")
        assert reason == 2 and its > RESTART                               # at least two cycles
        if driver == "gmres":
            assert dk <= 1e-7 and dphi <= 1e-6
        else:
            assert true <= MARGIN * rtol
        assert halos + folded >= its and (folded > 0) == (driver == "fgmres" and not hooks)
        if hooks:
            assert (h.halo_calls - calls0[0], h.ar_calls - calls0[1]) == (halos, ars)
        assert be.stats()["fused_tails"] == 0
        _check_unpacked(c)                                                 # the fields after the solve: those of the unfused unpack
    if (name, rank, hooks) == ("hub2d_12_48m", 1, False):
        assert its_left % RESTART <= 8, its_left                           # a last cycle the fused tail would take (see the next test)


def _check_unpacked(c, poison=True):
    """``be.unpack()`` into fields that hold a sentinel, then every field against NumPy indexing of ``be.x``, bit for bit, at every
    local vertex -- ghost vertices from the ghost entries of x.  ``poison=False`` after a fused tail: the library cannot see the
    caller write the target, and ``knp_unpack`` of fields it holds as current returns at once (include/knpemi_hip.h)."""
    be, p = c.be, c.p
    for fn in [*p.wh[0][:4], *p.wh[1][:4], p.phi_m_prev] if poison else []:
        fn.x.array.fill_(SENTINEL)
    be.unpack()
    x = be.x.cpu().numpy()
    for side, nodes in ((0, be.node_i), (1, be.node_e)):
        for f in range(4):
            expect = np.where(nodes >= 0, x[4 * np.maximum(nodes, 0) + f], 0.0)
            assert np.array_equal(p.wh[side][f].numpy(), expect), (side, f)
    assert np.array_equal(p.phi_m_prev.numpy(), p.wh[0][3].numpy() - p.wh[1][3].numpy())


@pytest.mark.parametrize("where", ["piece", "whole"])
def test_fused_tail_runs_on_a_whole_mesh_and_not_on_a_piece(where, tmp_path):
    """The same calls on hub2d_12_48m and on its piece 1: target registered (``fields_out``), no hooks, no null space, vertex-block
    Jacobi, ``knp_gmres_solve`` with restart 8 and a budget of 40 iterations -- every cycle has at most 8 columns, so the update after
    which the solve returns is one the fused tail takes (knp_krylov.inc: ``stop && tail_ok && jd <= 8``).  On the whole mesh it runs
    (``fused_tails`` 1) and ``knp_unpack`` finds the fields current; on the piece ``knp_create`` has switched it off (ghost nodes):
    ``fused_tails`` stays 0, the fields still hold the sentinel after the solve, and ``knp_unpack`` writes every local vertex, the
    ghost vertices from the ghost entries of x, which the solve has left as they were.  Fields against NumPy indexing of x, bit for bit
    (e)."""
    name, rank = "hub2d_12_48m", 1
    if where == "piece":
        c = _piece(tmp_path, name, rank)
    else:
        from parity_utils import make_problem
        p = make_problem(IM.config(tmp_path, name))
        o = IM.oracle(name)
        IM.perturb(o, p)
        be = p.create_backend()
        c = Piece(name, -1, p.local_mesh, o, o, p, be, np.arange(o.n_dof), o.n_dof)
    be, p, n = c.be, c.p, c.n_own
    assert (be.n_dof_local > be.n_dof_owned) == (where == "piece")
    be.assemble_matrix()
    be.assemble_rhs()
    be.set_nullspace(False)
    be.pc_setup(1)
    be.fields_out()
    x0 = np.random.default_rng(6).standard_normal(be.n_dof_local) * 1e-3
    be.x.copy_(c.dev(x0))
    for fn in (p.wh[0][3], p.wh[1][3]):                                    # the potentials: no assembly reads them
        fn.x.array.fill_(SENTINEL)
    st0 = be.stats()
    its, rn, reason = be.gmres(1e-8, 1e-50, 40, 8)
    tails = be.stats()["fused_tails"] - st0["fused_tails"]
    x = be.x.cpu().numpy()
    print(f"ERR e {where}: its {its} reason {reason} fused tails {tails}")
    assert 0 < its <= 40 and np.all(np.isfinite(x)) and np.array_equal(x[n:], x0[n:])
    touched = not np.all(p.wh[0][3].numpy() == SENTINEL)
    assert tails == (1 if where == "whole" else 0) and touched == (where == "whole")
    if where == "whole":                                                   # what the tail wrote is what knp_unpack writes
        for side, nodes in ((0, be.node_i), (1, be.node_e)):
            for f in range(4):
                assert np.array_equal(p.wh[side][f].numpy(), np.where(nodes >= 0, x[4 * np.maximum(nodes, 0) + f], 0.0)), (side, f)
    _check_unpacked(c, poison=where == "piece")


# ---- f (continued). the AMG cycle on the owned block of P: the route of KNP_DIST_PC=bj -------------------------------------------------
AMG_PIECE = ("delaunay2d_24", 0)
AMG_COARSE = 12                     # test_gpu_irregular.COARSE["delaunay2d_24"]


def _pc_solver(tmp_path, fp32, pc="hypre"):
    """test_gpu_irregular._pc_solver on a piece, one process: ``assemble_preconditioner`` builds the hierarchy on ``own_block`` of P"""
    from CGx.KNPEMI.KNPEMIx_solver import SolverKNPEMI
    name, rank = AMG_PIECE
    lm = RP.cut_piece(name, rank)
    og = RP.global_oracle(name)
    cfg = IM.config(tmp_path, name, pc=pc)
    ks = cfg["solver"]["ksp_settings"]
    ks["amg_coarse_size"], ks["amg_fp32"], ks["amg_setup"] = AMG_COARSE, fp32, "host"
    p = RP.make_piece_problem(tmp_path, name, lm, og, cfg=cfg)
    s = SolverKNPEMI(p, solver_config=p.solver_config)
    s.btcc_coupled_phi = False      # what a rank of a multi-rank run gets: the coupled potential block is for whole meshes on one GPU
    s.setup_solver()
    RP.set_piece_state(p, lm, og)
    p.setup_preconditioner(s.use_block_Jacobi)
    s.assemble_preconditioner()
    be = s.backend
    be.assemble_rhs()
    be.assemble_matrix()
    be.pc_setup(s._pc_kind)
    return s, be, lm, og


@pytest.mark.parametrize("G", [None, 16])
@pytest.mark.parametrize("fp32", [False, True])
def test_pc_apply_hypre_on_the_owned_block_against_the_numpy_cycle(fp32, G, tmp_path, monkeypatch):
    """test_gpu_irregular.test_pc_apply_against_the_numpy_cycle on a piece of delaunay2d_24 (the pieces of the other cuts hold 320 to
    548 unknowns: too few for three levels): ``pc_apply`` against knpemi_oracle.pc_amg_vcycle on the hierarchy that was uploaded, per
    field block 1e-10 with fp64 storage, 2e-6 with fp32; the fused cycle, KNP_BLOCKED=0 and the level-by-level cycle (KNP_FUSED=0:
    k_pnode, which skips the ghost columns of P).  The ghost entries of r hold other numbers and must not matter; those of z keep what
    they held."""
    import knpemi_oracle as K
    from parity_utils import fp32_stored
    if G is not None:
        monkeypatch.setenv("KNP_PC_GROUP", str(G))
    s, be, lm, og = _pc_solver(tmp_path, fp32)
    n = be.n_dof_owned
    info = be.launch_info()
    levels = [len(h.levels) for h in s.hierarchies]
    assert info["pc_group"] == (G or IM.EXPECT[AMG_PIECE[0]]["asm_group"] // 2) and n < be.n_dof_local
    assert s.hierarchy.levels[0].A.shape == (n, n) and all(k >= 3 for k in levels), levels
    bg = og.assemble_b()
    ol = RP.piece_oracle(lm, og)
    own = RP.global_maps(lm, ol, og)[:n]
    b = be.b.cpu().numpy()[:n]
    assert _rel(b, bg[own]) <= 1e-12 and all(_rel(b[f::4], bg[own][f::4]) <= 1e-10 for f in range(4))      # k_rhs<G>, the same switch
    r = np.random.default_rng(3).standard_normal(be.n_dof_local)
    rt = torch.as_tensor(r, device=be.device)
    tol = 2e-6 if fp32 else 1e-10
    seen = []
    for switch in (None, "KNP_BLOCKED", "KNP_FUSED"):
        if switch:
            monkeypatch.setenv(switch, "0")
            be.pc_setup(s._pc_kind)
        st = be.stats()
        seen.append((st["fused"], st["blocked"]))
        z = torch.full_like(rt, SENTINEL)
        be.pc_apply(rt, z)
        z = z.cpu().numpy()
        assert np.all(z[n:] == SENTINEL) and np.array_equal(rt.cpu().numpy(), r)
        h = fp32_stored(s.hierarchy) if fp32 else s.hierarchy
        zo = K.pc_amg_vcycle(h.levels, h.coarse_inv, s.amg_pre, s.amg_post, s.amg_cheby_degree, fused=bool(st["fused"]))(r[:n].copy())
        d = [np.max(np.abs(z[:n][f::4] - zo[f::4])) / np.max(np.abs(zo[f::4])) for f in range(4)]
        print(f"ERR f hypre piece {AMG_PIECE} levels {levels} fp32={fp32} G={info['pc_group']} fused={st['fused']} blocked={st['blocked']}: {d}")
        for f in range(4):
            assert d[f] <= tol, (switch, f, d)
    assert seen[0][0] > 0 and (seen[0][1] > 0) == fp32 and seen[1] == (seen[0][0], 0) and seen[2][0] == 0, seen


def _btcc_on_a_piece(ol, n, hk, hp, pre, post, deg, fused, ghost_z):
    """knpemi_oracle.pc_btcc for the owned block of a piece: the hierarchies act on the owned unknowns, the mass-matrix row of an
    owned node reaches ghost nodes, whose ion corrections are ``ghost_z`` ([n_dof_local - n])"""
    import knpemi_oracle as K
    import scipy.sparse as sp
    Vk = K.pc_amg_vcycle(hk.levels, hk.coarse_inv, pre, post, deg, fused=fused)
    Vp = K.pc_amg_vcycle(hp.levels, hp.coarse_inv, pre, post, deg, fused=fused)
    nn, no = ol.lay.n_nodes, n // 4
    Mn = sp.coo_matrix((ol.Mloc.ravel(), (ol.rowsA.ravel(), ol.colsA.ravel())), shape=(nn, nn)).tocsr()
    ML = np.asarray(Mn.sum(axis=1)).ravel()
    zz = np.array(ol.p.z)
    s = np.zeros(nn)
    for side, nodes in ((0, ol.lay.node_i), (1, ol.lay.node_e)):
        v = np.nonzero(nodes >= 0)[0]
        s[nodes[v]] = sum(ol.p.z[j] ** 2 * ol.k[side][j][v] for j in range(3))
    cc = (ol.p.psi / (s * ML))[:no]
    pidx = np.arange(3, n, 4)

    def apply(r):
        z = Vk(r)
        z[pidx] = 0.0
        zl = np.concatenate([z, ghost_z])
        zr = sum(zz[j] * r[j::4] for j in range(3))
        zk = sum(zz[j] * zl[j::4] for j in range(3))
        t = np.zeros_like(r)
        t[pidx] = r[pidx] - zr + (Mn @ zk)[:no]
        w = Vp(t)
        z[pidx] = w[pidx] + cc * t[pidx]
        return z
    return apply


@pytest.mark.parametrize("G", [None, 16])
@pytest.mark.parametrize("fp32", [False, True])
def test_pc_apply_btcc_on_the_owned_block_against_the_numpy_cycle(fp32, G, tmp_path, monkeypatch):
    """The same for the block-triangular preconditioner, both hierarchies on the owned block.  The potential right-hand side
    t_phi = r_phi - sum_j z_j r_kj + M (sum_j z_j z_kj) is the one place where a row of an owned node reaches ghost unknowns: the
    level-by-level cycle reads them from z after the halo exchange (here: what z holds there), the fused cycle forms the ion charge at
    the owned nodes only and reads zeros at the ghost nodes -- per-GPU blocks either way, and the same numbers at every application."""
    from parity_utils import fp32_stored
    if G is not None:
        monkeypatch.setenv("KNP_PC_GROUP", str(G))
    s, be, lm, og = _pc_solver(tmp_path, fp32, "btcc")
    n = be.n_dof_owned
    ol = RP.piece_oracle(lm, og)
    levels = [len(h.levels) for h in s.hierarchies]
    assert len(levels) == 2 and all(k >= 3 for k in levels), levels
    rng = np.random.default_rng(3)
    r = rng.standard_normal(be.n_dof_local)
    ghost = rng.standard_normal(be.n_dof_local - n)
    rt = torch.as_tensor(r, device=be.device)
    tol = 2e-6 if fp32 else 1e-10
    seen = []
    for switch in (None, "KNP_BLOCKED", "KNP_FUSED"):
        if switch:
            monkeypatch.setenv(switch, "0")
            be.pc_setup(s._pc_kind)
        st = be.stats()
        fused = bool(st["fused"])
        seen.append(st["fused"])
        z = torch.as_tensor(np.concatenate([np.full(n, SENTINEL), ghost]), device=be.device)
        be.pc_apply(rt, z)
        z = z.cpu().numpy()
        assert np.array_equal(z[n:], ghost) and np.array_equal(rt.cpu().numpy(), r)
        hk, hp = s.hierarchies
        if fp32:
            hk, hp = fp32_stored(hk, coarse=fused), fp32_stored(hp, level0_uploaded=s._coupled_phi)
        zo = _btcc_on_a_piece(ol, n, hk, hp, s.amg_pre, s.amg_post, s.amg_cheby_degree, fused, np.zeros_like(ghost) if fused else ghost)(r[:n].copy())
        d = [np.max(np.abs(z[:n][f::4] - zo[f::4])) / np.max(np.abs(zo[f::4])) for f in range(4)]
        print(f"ERR f btcc piece {AMG_PIECE} levels {levels} fp32={fp32} G={be.launch_info()['pc_group']} fused={st['fused']} blocked={st['blocked']}: {d}")
        for f in range(4):
            assert d[f] <= tol, (switch, f, d)
    assert seen[0] > 0 and seen[1] == seen[0] and seen[2] == 0, seen


# ---- h. per-tag diagnostics summed over the pieces --------------------------------------------------------------------------------------
def test_per_tag_diagnostics_of_the_pieces_add_up(tmp_path):
    """test_gpu_irregular.test_per_tag_diagnostics_on_cells_and_facets_of_many_sizes per piece of the two-tag mesh cut in 2, with its
    tolerances (ion amounts rtol 1e-12, fluxes and membrane potential 1e-12 of the magnitude sums S, the membrane integral of the
    stimulus current rtol 1e-12 as test_membrane_integral_of_a_group_longer_than_a_wave_matches_host_quadrature): each piece against
    the host integrals over what it owns, the sum of the pieces against the host integrals and against the GPU on the whole mesh.
    Piece 1 sees ten facets of tag 2 and owns none: an empty segment, zeros, (0, +inf, -inf)."""
    from cgx_hip.diagnostics import membrane_program
    from flux_ref import TOL
    from phim_ref import phim_ref
    from test_gpu_fluxes import _reference
    from test_gpu_ion_budget import _host_budget, _host_stimulus
    from test_gpu_membrane_potential import _check_device
    p0 = RP.two_tag_problem(tmp_path)
    nv = p0.local_mesh.coords.shape[0]
    rng = np.random.default_rng(11)
    fields = {(s, j): rng.uniform(1.0, 150.0, nv) for s in range(2) for j in range(3)}
    fields.update({(s, 3): rng.uniform(-0.1, 0.1, nv) for s in range(2)})
    tags = [int(t) for t in p0.gamma_tags]
    groups = [[t] for t in tags]
    assert tags == [2, 3]

    def run(p, l2g):
        be = p.create_backend()
        for (s, j), v in fields.items():
            p.wh[s][j].x.array[:] = torch.as_tensor(v[l2g], device=be.device)
        p.phi_m_prev.x.array[:] = torch.as_tensor((fields[(0, 3)] - fields[(1, 3)])[l2g], device=be.device)
        out = {}
        ctags, host = _host_budget(p)
        out["ions"], out["ions_host"] = be.ion_amounts().cpu().numpy(), host
        assert np.array_equal(be.budget_layout().tags, ctags)
        fl = p.membrane_fluxes()
        ref, S, cover = _reference(p, groups, False)
        out["flux"], out["flux_ref"], out["flux_S"] = np.stack([fl["flux_i"], fl["flux_e"]], axis=1), ref, S
        out["area"], out["n_facets"] = fl["area"], [len(cv) for cv in cover]
        p.membrane_potential()
        out["phim"] = be.membrane_potential().cpu().numpy()
        out["phim_ref"] = phim_ref(p, p.phi_m_prev.numpy().copy(), groups)
        be.set_diag_program(membrane_program(p, p.stim_ufl_expr))
        be.set_facet_groups(groups)
        out["stim"] = be.membrane_integral(torch.full((2,), SENTINEL, dtype=torch.float64, device=be.device)).cpu().numpy()
        be.set_facet_groups([p.stimulus_tags])
        out["stim_all"] = be.membrane_integral(torch.full((1,), SENTINEL, dtype=torch.float64, device=be.device)).cpu().numpy()[0]
        out["stim_host"] = _host_stimulus(p)
        return out
    whole = run(p0, np.arange(nv))
    parts = []
    for r in range(RP.TWO_TAG_CUT[0]):
        lm = RP.two_tag_piece(r)
        parts.append(run(RP.two_tag_problem(tmp_path, lm, p0.stimulus_area), lm.l2g))
    for r, o in enumerate([whole] + parts):
        what = "whole mesh" if r == 0 else f"piece {r - 1}"
        d_ions = np.abs(o["ions"] / o["ions_host"] - 1.0).max()
        d_flux = (np.abs(o["flux"] - o["flux_ref"]) / np.maximum(o["flux_S"], 1e-300)).max()
        print(f"ERR h {what}: ions {d_ions:.2e}  fluxes / S {d_flux:.2e}  owned facets per tag {o['n_facets']}  stimulus "
              f"{abs(o['stim_all'] / o['stim_host'] - 1.0):.2e}")
        assert np.allclose(o["ions"], o["ions_host"], rtol=1e-12, atol=0)
        assert np.all(np.abs(o["flux"] - o["flux_ref"]) <= TOL * o["flux_S"])
        _check_device(o["phim"], o["phim_ref"], what)
        assert np.isclose(o["stim_all"], o["stim_host"], rtol=1e-12, atol=0) and np.isclose(o["stim"].sum(), o["stim_host"], rtol=1e-12, atol=0)
    # the tag piece 1 owns no facet of: zeros, not what the output held
    assert parts[1]["n_facets"][0] == 0 and (np.asarray(RP.two_tag_piece(1).gamma_tags) == 2).sum() > 0
    assert np.all(parts[1]["flux"][0] == 0.0) and parts[1]["area"][0] == 0.0 and parts[1]["stim"][0] == 0.0
    assert parts[1]["phim"][0].tolist() == [0.0, np.inf, -np.inf]
    # sums over the pieces: against the host on the whole mesh and against the GPU on the whole mesh
    S = whole["flux_S"]
    ions, flux = sum(o["ions"] for o in parts), sum(o["flux"] for o in parts)
    stim = sum(o["stim"] for o in parts)
    I = sum(o["phim"][:, 0] for o in parts)
    lo, hi = np.min([o["phim"][:, 1] for o in parts], axis=0), np.max([o["phim"][:, 2] for o in parts], axis=0)
    I0, _, lo0, hi0, S0, _ = whole["phim_ref"]
    print("ERR h sums: ions", np.abs(ions / whole["ions_host"] - 1.0).max(), np.abs(ions / whole["ions"] - 1.0).max(),
          "fluxes / S", (np.abs(flux - whole["flux_ref"]) / S).max(), (np.abs(flux - whole["flux"]) / S).max(),
          "phi_m / S", (np.abs(I - I0) / S0).max(), (np.abs(I - whole["phim"][:, 0]) / S0).max(),
          "stimulus", np.abs(stim / whole["stim"] - 1.0).max(), abs(stim.sum() / whole["stim_host"] - 1.0))
    for ref in (whole["ions_host"], whole["ions"]):
        assert np.allclose(ions, ref, rtol=1e-12, atol=0)
    for ref in (whole["flux_ref"], whole["flux"]):
        assert np.all(np.abs(flux - ref) <= TOL * S)
    for ref in (I0, whole["phim"][:, 0]):
        assert np.all(np.abs(I - ref) <= TOL * S0)
    assert np.array_equal(lo, lo0) and np.array_equal(hi, hi0)
    assert np.allclose(sum(o["area"] for o in parts), whole["area"], rtol=1e-13, atol=0)
    assert np.allclose(stim, whole["stim"], rtol=1e-12, atol=0) and np.isclose(stim.sum(), whole["stim_host"], rtol=1e-12, atol=0)


# ---- i. the interior / boundary row split, which only runs with the native exchange: two ranks on the one GPU ---------------------------
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spmv_worker(rank, size, port, q, comm, split, tmp):
    """the spawn harness of test_gpu_distributed.py: one knp_spmv on this rank's slice of a vector of the whole mesh"""
    try:
        os.environ["KNP_COMM"] = comm
        os.environ.setdefault("KNP_P2P_TIMEOUT", "10")
        if not split:
            os.environ["KNP_SPMV_SPLIT"] = "0"
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=size)
        from parity_utils import make_problem
        name = "hub2d_12_48m"
        mine = os.path.join(tmp, f"{comm}{int(split)}_{rank}")
        os.makedirs(mine)
        p = make_problem(IM.config(mine, name))                # read from a file: cut by kway
        lm = p.local_mesh
        og = RP.global_oracle(name)
        ol = RP.piece_oracle(lm, og)
        l2gd, n = RP.global_maps(lm, ol, og), 4 * RP.n_nodes_owned(lm, ol)
        assert p.comm.size == size and abs(p.stimulus_area - og.stimulus_area) <= 1e-12 * og.stimulus_area
        RP.set_piece_state(p, lm, og)
        be = p.create_backend()
        assert be.n_dof_owned == n < be.n_dof_local and be.n_dof_global == og.n_dof
        be.assemble_matrix()
        interior, boundary = RP.interior_boundary(lm, ol, ol.assemble_A().tocsr())
        xg = np.random.default_rng(0).standard_normal(og.n_dof)
        x = np.full(be.n_dof_local, np.nan)                    # the exchange fills the ghost entries
        x[:n] = xg[l2gd[:n]]
        xt = torch.as_tensor(x, device=be.device)
        yt = torch.full_like(xt, SENTINEL)
        be.spmv(xt, yt)
        y = yt.cpu().numpy()
        ghosts_filled = bool(np.array_equal(xt.cpu().numpy(), xg[l2gd]))
        q.put((rank, "ok", y[:n].copy(), l2gd[:n].copy(), bool(getattr(be, "p2p_on", False)), len(interior), len(boundary),
               bool(np.all(y[n:] == SENTINEL)), ghosts_filled))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:      # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


def _spmv_leg(size, comm, split, tmp):
    """one leg; raises -- so that no later leg starts -- when a rank reports an error or ends abnormally"""
    import queue
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_spmv_worker, args=(r, size, port, q, comm, split, str(tmp))) for r in range(size)]
    for p in procs:
        p.start()
    res, waited = [], 0.0
    while len(res) < size:
        try:
            res.append(q.get(timeout=1.0))
        except queue.Empty:
            waited += 1.0
            dead = [(p.pid, p.exitcode) for p in procs if p.exitcode not in (None, 0)]
            assert not dead, f"leg {comm} split={split}: a rank ended abnormally: {dead}"
            assert waited < 300.0, f"leg {comm} split={split}: no answer"
    for p in procs:
        p.join(timeout=60)
    assert [p.exitcode for p in procs] == [0] * size, [p.exitcode for p in procs]
    for r in res:
        assert r[1] == "ok", f"rank {r[0]}:\n{r[1]}"
        assert r[4] == (comm == "p2p"), "the requested exchange path is not the one that ran"
    return {r[0]: r for r in res}


def test_split_spmv_computes_the_rows_of_the_unsplit_one(tmp_path, globals_):
    """knp_spmv over 2 ranks on hub2d_12_48m cut by kway: with the native exchange (interior rows while the halo travels, boundary rows
    after it), with the native exchange and KNP_SPMV_SPLIT=0, and through the hooks.  The gathered y against the product on the whole
    mesh, row by row with the bound of (c); the three legs bit for bit per rank: the split changes which launch computes a row, not the
    row's arithmetic.  The library does not export its row lists (``n_int``, ``n_bnd``): that the split launch ran in the first leg
    is inferred from ``p2p_on``, from ghost entries of x that were NaN before the call, and from the host's restatement of
    ``knp_create``'s rule giving both lists non-empty; the agreement of the legs alone would not show it."""
    import time
    t0 = time.perf_counter()
    size = 2
    legs = {}
    for comm, split in (("p2p", True), ("p2p", False), ("hooks", True)):
        legs[(comm, split)] = _spmv_leg(size, comm, split, tmp_path)
    Ag = globals_("hub2d_12_48m")[0]
    xg = np.random.default_rng(0).standard_normal(Ag.shape[0])
    want, bound = Ag @ xg, abs(Ag) @ np.abs(xg)
    for key, leg in legs.items():
        y = np.full(Ag.shape[0], np.nan)
        for r in range(size):
            _, _, yr, own, _, n_int, n_bnd, y_ghost_kept, ghosts_filled = leg[r]
            assert n_int > 0 and n_bnd > 0 and y_ghost_kept and ghosts_filled, (key, r, n_int, n_bnd, y_ghost_kept, ghosts_filled)
            assert np.all(np.isnan(y[own]))
            y[own] = yr
        err = np.abs(y - want)
        print(f"ERR i {key}: SpMV max err / bound = {(err / bound).max():.3e}; interior / boundary nodes {[(leg[r][5], leg[r][6]) for r in range(size)]}")
        assert np.all(err <= 1e-12 * bound)
    first = legs[("p2p", True)]
    for key, leg in legs.items():
        for r in range(size):
            assert np.array_equal(leg[r][2], first[r][2]), (key, r)
    print(f"ERR i wall time of the three legs: {time.perf_counter() - t0:.1f} s")
