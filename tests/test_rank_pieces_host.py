"""Preconditions of tests/test_gpu_rank_pieces.py, on the host: the cuts of tests/rank_pieces.py do have what the owned/ghost paths
of the kernels need (ghost nodes, facets a piece sees but does not own, the hub owned here and a ghost there, interior and boundary
rows), the oracle on a piece reproduces the owned rows of the oracle on the whole mesh far below the 1e-12 of the GPU comparisons,
and each mistake a kernel could make about ownership moves the result by more than 1e-6 (the teeth)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import irregular_meshes as IM
import rank_pieces as RP

ALL = [(name, r) for name, (size, _) in RP.CUTS.items() for r in range(size)]


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


@pytest.fixture(scope="module")
def built():
    """per piece: LocalMesh, whole-mesh oracle, piece oracle, dof map, owned dofs, A of the piece"""
    cache = {}

    def get(name, rank):
        if (name, rank) not in cache:
            lm = RP.cut_piece(name, rank)
            og = RP.global_oracle(name)
            ol = RP.piece_oracle(lm, og)
            cache[(name, rank)] = (lm, og, ol, RP.global_maps(lm, ol, og), 4 * RP.n_nodes_owned(lm, ol), ol.assemble_A().tocsr())
        return cache[(name, rank)]
    return get


@pytest.fixture(scope="module")
def global_ops():
    cache = {}

    def get(name):
        if name not in cache:
            og = RP.global_oracle(name)
            cache[name] = (og.assemble_A().tocsr(), og.assemble_b(), og.assemble_P().tocsr())
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(RP.CUTS))
def test_every_cell_facet_and_vertex_has_one_owner(name, built):
    size, _ = RP.CUTS[name]
    coords, cells, _ = IM.mesh(name)
    gamma, _ = RP.gamma_of(name)
    pieces = [built(name, r) for r in range(size)]
    assert sum(lm.n_cells_owned for lm, *_ in pieces) == cells.shape[0]
    owned_cells = np.concatenate([np.sort(lm.l2g[lm.cells[:lm.n_cells_owned]], axis=1) for lm, *_ in pieces])
    assert len({tuple(c) for c in owned_cells.tolist()}) == cells.shape[0]
    facets = np.concatenate([np.sort(lm.l2g[ol.fv[RP.owned_facets(lm, ol)]], axis=1) for lm, _, ol, *_ in pieces])
    assert facets.shape[0] == gamma.shape[0] and len({tuple(f) for f in facets.tolist()}) == gamma.shape[0]
    verts = np.concatenate([lm.l2g[:lm.n_vertices_owned] for lm, *_ in pieces])
    assert np.array_equal(np.sort(verts), np.arange(coords.shape[0]))
    og = pieces[0][1]
    assert sum(n_own for *_, n_own, _ in pieces) == og.n_dof
    # ghosts everywhere; facets seen but not owned somewhere; the hub owned by one piece and a ghost of another
    assert all(lm.coords.shape[0] > lm.n_vertices_owned and ol.n_dof > n_own for lm, _, ol, _, n_own, _ in pieces)
    assert any((~RP.owned_facets(lm, ol)).any() for lm, _, ol, *_ in pieces)
    if name in RP.HUB:
        hub = IM.hub_vertex(coords, RP.HUB[name])
        where = [np.nonzero(lm.l2g == hub)[0] for lm, *_ in pieces]
        assert sum(1 for (lm, *_), w in zip(pieces, where) if len(w) and w[0] < lm.n_vertices_owned) == 1
        assert any(len(w) and w[0] >= lm.n_vertices_owned for (lm, *_), w in zip(pieces, where))
    print(name, [(lm.n_vertices_owned, lm.coords.shape[0] - lm.n_vertices_owned, ol.fv.shape[0], int(RP.owned_facets(lm, ol).sum()))
                 for lm, _, ol, *_ in pieces])


def test_the_pieces_of_the_gpu_tests_see_facets_they_do_not_own(built):
    for name, r in RP.PIECES:
        lm, _, ol, *_ = built(name, r)
        assert (~RP.owned_facets(lm, ol)).any(), (name, r)


@pytest.mark.parametrize("name,rank", ALL)
def test_interior_and_boundary_rows_exist(name, rank, built):
    lm, og, ol, l2gd, n_own, A = built(name, rank)
    interior, boundary = RP.interior_boundary(lm, ol, A)
    print(name, rank, "interior", len(interior), "boundary", len(boundary))
    assert len(interior) > 0 and len(boundary) > 0 and len(interior) + len(boundary) == n_own // 4


@pytest.mark.parametrize("name,rank", ALL)
def test_owned_rows_of_the_piece_oracle_are_the_global_rows(name, rank, built, global_ops):
    lm, og, ol, l2gd, n_own, A = built(name, rank)
    Ag, bg, Pg = global_ops(name)
    own = l2gd[:n_own]
    assert np.array_equal(np.sort(l2gd), np.unique(l2gd))
    dA = abs(RP.to_global_columns(A[:n_own], l2gd, og.n_dof) - Ag[own]).max() / abs(Ag).max()
    dP = abs(RP.to_global_columns(ol.assemble_P().tocsr()[:n_own], l2gd, og.n_dof) - Pg[own]).max() / abs(Pg).max()
    b = ol.assemble_b()[:n_own]
    db = max(_rel(b[f::4], bg[own][f::4]) for f in range(4))
    print(f"{name} piece {rank}: A {dA:.2e}  b {db:.2e}  P {dP:.2e}")
    assert dA <= 1e-14 and dP <= 1e-14 and db <= 1e-14


@pytest.mark.parametrize("name,rank", ALL)
def test_teeth(name, rank, built, global_ops):
    """what each ownership mistake would change, relative to the right result: all far above the 1e-6 of the end-to-end tests"""
    lm, og, ol, l2gd, n_own, A = built(name, rank)
    Ag, bg, _ = global_ops(name)
    xg = np.random.default_rng(0).standard_normal(og.n_dof)
    x = xg[l2gd]
    y = A[:n_own] @ x
    assert _rel(y, (Ag @ xg)[l2gd[:n_own]]) <= 1e-13
    x0 = x.copy()
    x0[n_own:] = 0.0
    a = _rel(A[:n_own] @ x0, y)                                         # (a) ghost entries of x not exchanged
    mine = RP.owned_facets(lm, ol)
    b_teeth = None
    if (~mine).any():
        b_own = RP.piece_oracle(lm, og, facets=mine).assemble_b()[:n_own]
        b_teeth = _rel(b_own, ol.assemble_b()[:n_own])                  # (b) b without the facets of other ranks
    nco, nc = lm.n_cells_owned, lm.cells.shape[0]
    phi = [np.cos(3e6 * ol.coords[:, 0]) + 2.0, np.sin(2e6 * ol.coords[:, 1]) + 2.0]
    # (c) the L2 norm over all local cells, on every side that has a ghost cell (a side without one has no such mistake to make)
    ghost_sides = [s for s in range(2) if (ol.cell_side[nco:] == s).any()]
    c = {s: RP.l2_sq(ol, phi[s], s, nc) / RP.l2_sq(ol, phi[s], s, nco) - 1.0 for s in ghost_sides}
    d = abs(x @ x / (x[:n_own] @ x[:n_own]) - 1.0)                      # (d) dot over n_dof_local
    print(f"{name} piece {rank}: (a) {a:.2e}  (b) {b_teeth if b_teeth is not None else 'no facet of another rank here: does not apply'}  "
          f"(c) {c}  (d) {d:.2e}")
    assert a > 1e-6 and d > 1e-6 and ghost_sides and all(v > 1e-6 for v in c.values())
    assert b_teeth is None or b_teeth > 1e-6
    if (name, rank) in RP.PIECES + [("delaunay2d_24", 0)]:              # every piece whose right-hand side a GPU test compares
        assert b_teeth is not None


@pytest.mark.parametrize("name,rank", ALL)
def test_owned_block_is_solvable(name, rank, built):
    """the owned x owned block of A (what a piece's Krylov solve with zeroed ghosts inverts): sparse LU residual and a condition
    estimate (1-norm, from the LU factors)"""
    lm, og, ol, l2gd, n_own, A = built(name, rank)
    Aoo = A[:n_own][:, :n_own].tocsc()
    b = ol.assemble_b()[:n_own]
    lu = spla.splu(Aoo)
    x = lu.solve(b)
    res = np.linalg.norm(b - Aoo @ x) / np.linalg.norm(b)
    inv1 = spla.onenormest(spla.LinearOperator(Aoo.shape, matvec=lu.solve, rmatvec=lambda v: lu.solve(v, trans="T")))
    print(f"{name} piece {rank}: n = {n_own}, LU residual {res:.2e}, cond_1 estimate {inv1 * spla.onenormest(Aoo):.2e}")
    assert res <= 1e-12


@pytest.mark.parametrize("name,rank", [("hub2d_12_48m", 1), ("delaunay3d_5", 0)])
def test_native_problem_on_a_piece(name, rank, built, tmp_path):
    """``make_piece_problem``: one process, the piece's mesh, the whole mesh's stimulus area and state"""
    lm, og, ol, *_ = built(name, rank)
    p = RP.make_piece_problem(tmp_path, name, lm, og)
    assert p.comm.size == 1 and p.local_mesh.n_vertices_owned < p.local_mesh.coords.shape[0]
    assert p.stimulus_area == og.stimulus_area != ol.fmeas[RP.owned_facets(lm, ol)].sum()
    assert np.array_equal(p.wh[0][0].numpy(), ol.k[0][0]) and np.array_equal(p.phi_m_prev.numpy(), ol.phi_m)
