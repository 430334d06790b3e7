"""Rank pieces of the irregular meshes (tests/irregular_meshes.py) for the owned/ghost paths of the kernels: ``partition_mesh`` cuts
a mesh for ``size`` ranks and hands back one rank's ``LocalMesh`` -- owned vertices first, one layer of ghost cells -- and ONE process
builds the context of that piece (``Backend`` installs communication hooks only when ``comm.size > 1``), so every operator can be
driven alone and compared with the oracle on the WHOLE mesh through ``l2g``.  Host only; preconditions in test_rank_pieces_host.py.

The previous state is the one of ``IM.perturb`` on the whole mesh, carried to a piece through ``l2g`` (``perturb`` scales by the
largest coordinate, which a piece does not share).  The stimulus area is a global integral: a piece takes it from the whole mesh.
"""
from __future__ import annotations

import numpy as np

import irregular_meshes as IM

# name -> (ranks, method): the smallest meshes of the suite, cut so that every piece has ghosts and the hub is owned by one piece
# and a ghost of another; the reoriented twin for the det < 0 branch on a piece.  The twin is cut in 3 by rcb: in 2, by rcb, slab or
# kway, the cut runs near x = 0.5 and the hub at x = 0.25 is a ghost of nobody (and in 3 by kway it is the parent's cut again).
CUTS = {
    "hub2d_12_48m": (3, "kway"),
    "delaunay3d_5": (2, "rcb"),
    "hub3d_5_60": (4, "rcb"),
    "hub2d_12_48m_cw": (3, "rcb"),
    "delaunay2d_24": (2, "rcb"),        # preconditioner cases only: three AMG levels need the unknowns
}
HUB = {"hub2d_12_48m": IM.MEMBRANE_HUB, "hub2d_12_48m_cw": IM.MEMBRANE_HUB, "hub3d_5_60": (0.5, 0.5, 0.5)}
# the (cut, rank) pieces the GPU tests build a context of
PIECES = [("hub2d_12_48m", 0), ("hub2d_12_48m", 1), ("hub2d_12_48m", 2), ("delaunay3d_5", 0), ("delaunay3d_5", 1), ("hub3d_5_60", 0),
          ("hub2d_12_48m_cw", 0), ("hub2d_12_48m_cw", 2)]
_CACHE = {}


def gamma_of(name):
    from cgx_hip import mesh as meshmod
    coords, cells, tags = IM.mesh(name)
    gamma, gtags, _ = meshmod.gamma_integration_entities(cells, tags, (1,), (2,))
    return gamma, gtags


def piece(name, size, rank, method):
    """the ``LocalMesh`` of rank ``rank`` of ``size`` (coordinates in metres, as the oracle's); cached, read only"""
    from cgx_hip.parallel import partition_mesh
    key = ("piece", name, size, rank, method)
    if key not in _CACHE:
        coords, cells, tags = IM.mesh(name)
        gamma, gtags = gamma_of(name)
        _CACHE[key] = partition_mesh(coords * 1e-6, cells.copy(), tags.copy(), gamma, gtags, size, rank, intra_tags=(1,), method=method)
    return _CACHE[key]


def cut_piece(name, rank):
    size, method = CUTS[name]
    return piece(name, size, rank, method)


def global_oracle(name):
    """the oracle on the whole mesh in the ``IM.perturb`` state, stimulus on (t = dt); cached: callers assemble, they do not write"""
    key = ("global", name)
    if key not in _CACHE:
        o = IM.oracle(name)
        IM.perturb(o)
        o.t = o.p.dt
        o.update_t_mod()
        _CACHE[key] = o
    return _CACHE[key]


def piece_oracle(lm, og, facets=None):
    """A new oracle on the piece ``lm`` in the state of the whole-mesh oracle ``og`` (fields through ``l2g``, time, stimulus area).
    ``facets``: a mask over the piece's membrane facets to keep (the wrong right-hand side of the teeth)."""
    import knpemi_oracle as K
    gamma, gtag = lm.gamma, lm.gamma_tags
    if facets is not None:
        gamma, gtag = gamma[facets], gtag[facets]
    ol = K.OracleKNPEMI(lm.coords, lm.cells, lm.cell_tags, gamma=gamma, gamma_tag=gtag, models=K.CI_MODELS(), mesh_conversion_factor=1.0)
    g = lm.l2g
    for side in range(2):
        for j in range(3):
            ol.k[side][j] = og.k[side][j][g].copy()
        ol.phi[side] = og.phi[side][g].copy()
    for nm in ("phi_m", "n", "m", "h"):
        setattr(ol, nm, getattr(og, nm)[g].copy())
    ol.t, ol.t_mod = og.t, og.t_mod
    ol.stimulus_area = og.stimulus_area
    return ol


def global_maps(lm, ol, og):
    """global dof of every local dof (the ``gdof`` of test_distributed_gloo.py)"""
    out = np.empty(ol.n_dof, dtype=np.int64)
    for nodes_l, nodes_g in ((ol.lay.node_i, og.lay.node_i), (ol.lay.node_e, og.lay.node_e)):
        v = np.nonzero(nodes_l >= 0)[0]
        assert (nodes_g[lm.l2g[v]] >= 0).all()
        for f in range(4):
            out[4 * nodes_l[v] + f] = 4 * nodes_g[lm.l2g[v]] + f
    return out


def n_nodes_owned(lm, ol):
    nvo = lm.n_vertices_owned
    return int((ol.lay.node_i[:nvo] >= 0).sum() + (ol.lay.node_e[:nvo] >= 0).sum())


def owned_facets(lm, ol):
    """mask over the piece's membrane facets: counted by the rank that owns the facet's first vertex"""
    return ol.fv[:, 0] < lm.n_vertices_owned


def to_global_columns(M, l2gd, n_glob):
    """rows of ``M`` (local columns) on the columns of the whole mesh"""
    import scipy.sparse as sp
    C = M.tocoo()
    return sp.csr_matrix((C.data, (C.row, l2gd[C.col])), shape=(M.shape[0], n_glob))


def interior_boundary(lm, ol, A):
    """Owned nodes split as ``knp_create`` splits them for the overlapped exchange: a node is boundary when its row of A, or the row of
    the node opposite it across the membrane, has a column in the ghost range."""
    no = n_nodes_owned(lm, ol)
    N = A[:4 * no].tocsr()
    ghost = np.zeros(no, dtype=bool)
    for r in range(4 * no):
        if N.indptr[r + 1] > N.indptr[r] and N.indices[N.indptr[r]:N.indptr[r + 1]].max() >= 4 * no:
            ghost[r // 4] = True
    other = np.full(ol.lay.n_nodes, -1, dtype=np.int64)
    both = np.nonzero((ol.lay.node_i >= 0) & (ol.lay.node_e >= 0))[0]
    other[ol.lay.node_i[both]] = ol.lay.node_e[both]
    other[ol.lay.node_e[both]] = ol.lay.node_i[both]
    bnd = ghost.copy()
    for n in range(no):
        if other[n] >= 0 and other[n] < no and ghost[other[n]]:
            bnd[n] = True
    return np.nonzero(~bnd)[0], np.nonzero(bnd)[0]


def l2_sq(ol, nodal, side, n_cells):
    """sum over the first ``n_cells`` cells of that side of u^T M_loc u (the P1 formula of ``OracleKNPEMI.l2_norm``)"""
    sel = np.nonzero(ol.cell_side[:n_cells] == side)[0]
    u = nodal[ol.cells[sel]]
    return float(np.einsum("ca,cab,cb->", u, ol.Mloc[sel], u))


def make_piece_problem(tmp_path, name, lm, og, pc="hypre", cfg=None):
    """The native problem on the piece ``lm`` (``make_problem`` with a ``LocalMesh``) in the state of ``og``, stimulus on.  The
    stimulus area is integrated over the membrane of ALL ranks: one process on one piece would integrate its own facets only, so the
    whole-mesh value is placed where ``HodgkinHuxley._add_stimulus`` keeps it."""
    from cgx_hip.ionic_models import ATPPump, HodgkinHuxley, NeuronalCotransporters
    from parity_utils import make_problem
    cfg = cfg or IM.config(tmp_path, IM.PARENT.get(name, name), pc=pc)

    def models(problem):
        problem._stimulus_area_cache = {(None, None, tuple(problem.stimulus_tags)): float(og.stimulus_area)}
        return [NeuronalCotransporters(problem), HodgkinHuxley(problem), ATPPump(problem)]
    p = make_problem(cfg, models, lm)
    assert p.stimulus_area == og.stimulus_area and p.local_mesh is lm
    set_piece_state(p, lm, og)
    return p


def set_piece_state(p, lm, og):
    """the fields and the time of the whole-mesh oracle ``og`` on the native problem of the piece ``lm``"""
    import torch
    dev = p.mesh.device
    g = lm.l2g
    for side in range(2):
        for j in range(3):
            p.wh[side][j].x.array[:] = torch.as_tensor(og.k[side][j][g], device=dev)
    p.phi_m_prev.x.array[:] = torch.as_tensor(og.phi_m[g], device=dev)
    for nm in ("n", "m", "h"):
        getattr(p, nm).x.array[:] = torch.as_tensor(getattr(og, nm)[g], device=dev)
    p.t.value = og.t
    for m in p.ionic_models:
        if hasattr(m, "update_t_mod"):
            m.update_t_mod()


# ---- the two-tag variant of delaunay3d(5) (IM.two_tag_config) cut in 2 by rcb, for the per-tag diagnostics: piece 1 sees 10 facets of
# tag 2 and owns none of them
TWO_TAG_CUT = (2, "rcb")


def two_tag_piece(rank):
    from cgx_hip import mesh as meshmod
    from cgx_hip.parallel import partition_mesh
    key = ("two_tag", rank)
    if key not in _CACHE:
        coords, cells, tags = IM.mesh("delaunay3d_5")
        t2 = IM.two_tag(coords, cells, tags)
        gamma, ftags, _ = meshmod.gamma_integration_entities(cells, t2, (2, 3), (1,), "intra")
        size, method = TWO_TAG_CUT
        _CACHE[key] = partition_mesh(coords * 1e-6, cells.copy(), t2, gamma, ftags, size, rank, intra_tags=(2, 3), method=method)
    return _CACHE[key]


def two_tag_problem(tmp_path, lm=None, stimulus_area=None):
    """the problem of ``IM.two_tag_config`` on the whole mesh (``lm`` None) or on a piece with the whole mesh's stimulus area"""
    from cgx_hip.ionic_models import ATPPump, HodgkinHuxley, NeuronalCotransporters
    from parity_utils import make_problem
    cfg = IM.two_tag_config(tmp_path)
    if lm is None:
        return make_problem(cfg, "ci")

    def models(problem):
        problem._stimulus_area_cache = {(None, None, tuple(problem.stimulus_tags)): float(stimulus_area)}
        return [NeuronalCotransporters(problem), HodgkinHuxley(problem), ATPPump(problem)]
    p = make_problem(cfg, models, lm)
    assert p.stimulus_area == stimulus_area and p.local_mesh is lm
    return p
