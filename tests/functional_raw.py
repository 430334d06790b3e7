"""The raw ABI of the two functional kinds through ctypes (``knp_functional_*`` / ``knp_membrane_functional_*`` of
include/knpemi_hip.h): create with valid default arguments, any of them replaced, evaluation into a torch buffer, destroy.  Shared by
tests/test_gpu_functionals.py, tests/test_gpu_membrane_functionals.py and tests/test_gpu_functionals_irregular.py; ``be`` is anything
with ``lib`` and ``ctx`` (and ``device`` for ``eval``)."""
import ctypes as C

import numpy as np


def _i32(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _f64(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def square_program():
    """OUT_0 = aux_0 ^ 2"""
    from cgx_hip._lib import OPS
    return np.array([[OPS["AUX"], 0, 0, 0], [OPS["MUL"], 1, 0, 0], [OPS["OUT"], 0, 0, 1]], dtype=np.int32)


class _RawKind:
    ABI = ITEMS = MODES = None

    def create(self, **kw):
        a = dict(self.args, **kw)
        fid = C.c_int32(-1)
        rc = getattr(self.be.lib, self.ABI + "_create")(self.be.ctx, a["n_tags"], _i32(a["seg_ptr"]), _i32(a[self.ITEMS]), a["n_q"],
                                                        _f64(a[self.POINTS]), _f64(a["q_w"]), a["n_instr"], _i32(a["code"]), a["n_consts"],
                                                        _f64(a["consts"]), a["n_aux"], _i32(a[self.MODES]), a["n_out"],
                                                        C.byref(fid) if a["id"] else None)
        return rc, int(fid.value)

    def eval(self, fid, fields, n_rows, n_out=1, fill=-123.25):
        """(return code, [n_rows, n_out] as NumPy): one evaluation into a new device buffer that held ``fill``"""
        import torch
        out = torch.full((max(n_rows * n_out, 1),), fill, dtype=torch.float64, device=self.be.device)
        rc = getattr(self.be.lib, self.ABI + "_eval")(self.be.ctx, fid, C.byref(fields), C.c_void_p(out.data_ptr()))
        torch.cuda.synchronize()
        return rc, out.cpu().numpy()[:n_rows * n_out].reshape(n_rows, n_out)

    def destroy(self, fid):
        return getattr(self.be.lib, self.ABI + "_destroy")(self.be.ctx, fid)

    def error(self):
        return (self.be.lib.knp_last_error(self.be.ctx) or b"").decode()


class RawVolume(_RawKind):
    """knp_functional_create with valid default arguments (phi^2 of aux 0 over all owned cells as one tag), any of them replaced"""
    ABI, ITEMS, POINTS, MODES = "knp_functional", "cells", "q_bary", "aux_deriv"

    def __init__(self, be, n_cells, dim):
        from cgx_hip.functionals import quadrature
        self.be, self.dim = be, dim
        qb, qw = quadrature(dim, 2)
        self.args = dict(n_tags=1, seg_ptr=np.array([0, n_cells], dtype=np.int32), cells=np.arange(n_cells, dtype=np.int32),
                         n_q=len(qw), q_bary=qb, q_w=qw, n_instr=3, code=square_program(),
                         n_consts=0, consts=None, n_aux=1, aux_deriv=np.array([-1], dtype=np.int32), n_out=1, id=True)


class RawMembrane(_RawKind):
    """knp_membrane_functional_create with valid default arguments (the square of aux 0 over all facets as one tag), any replaced"""
    ABI, ITEMS, POINTS, MODES = "knp_membrane_functional", "facets", "q_pts", "aux_mode"

    def __init__(self, be, n_facets, dim):
        from cgx_hip.mesh import facet_quadrature
        self.be, self.dim = be, dim
        qp, qw = facet_quadrature(dim, 2)
        self.args = dict(n_tags=1, seg_ptr=np.array([0, n_facets], dtype=np.int32), facets=np.arange(n_facets, dtype=np.int32),
                         n_q=len(qw), q_pts=np.ascontiguousarray(qp), q_w=np.ascontiguousarray(qw), n_instr=3, code=square_program(),
                         n_consts=0, consts=None, n_aux=1, aux_mode=np.array([-1], dtype=np.int32), n_out=1, id=True)
