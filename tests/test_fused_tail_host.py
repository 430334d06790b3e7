"""The (data_ptr, _version) bookkeeping with which cgx_hip.backend.Backend decides whether to promise the library that nobody wrote the
fields between an unpack and the next matrix assembly (knp_fields_unchanged): one walk over the tensors per step, compared with the
walk of the previous assembly.  No GPU: CPU tensors and a stub library that records the calls."""
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "knp-emi-cgx_amd"))

from cgx_hip.backend import Backend  # noqa: E402


class _StubLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("knp_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


def _function(n=5):
    t = torch.zeros(n, dtype=torch.float64)
    return types.SimpleNamespace(x=types.SimpleNamespace(array=t), data_ptr=t.data_ptr)


@pytest.fixture()
def be():
    b = Backend.__new__(Backend)
    b.lib = _StubLib()
    b.ctx = None
    b.check = lambda rc: None
    b.p = types.SimpleNamespace(wh=[[_function() for _ in range(4)] for _ in range(2)], phi_m_prev=_function(), aux_functions=[])
    b.x = torch.zeros(40, dtype=torch.float64)
    return b


def _assemble(be):
    be.lib.calls.clear()
    be.assemble_matrix_async()
    return be.lib.calls


def test_fields_out_registers_the_unpack_target(be):
    be.fields_out()
    be.fields_out()      # cached: registered once
    assert be.lib.calls == ["knp_set_unpack_target"]


def _step(be):
    """the assembly of a step and its unpack"""
    _assemble(be)
    be.unpack()


def test_unchanged_fields_give_the_promise_once(be):
    _step(be)
    assert _assemble(be) == ["knp_fields_unchanged", "knp_assemble_matrix_async"]
    assert _assemble(be) == ["knp_assemble_matrix_async"]      # one shot: no unpack in between
    be.unpack()
    assert _assemble(be) == ["knp_fields_unchanged", "knp_assemble_matrix_async"]


def test_no_promise_without_an_earlier_assembly_and_unpack(be):
    assert _assemble(be) == ["knp_assemble_matrix_async"]
    be2_calls = _assemble(be)
    assert be2_calls == ["knp_assemble_matrix_async"]      # marks equal, but nothing was unpacked


def test_inplace_write_withholds_the_promise(be):
    _step(be)
    be.p.wh[0][0].x.array[...] *= 1.01
    assert _assemble(be) == ["knp_assemble_matrix_async"]
    be.unpack()
    be.p.wh[1][2].x.array.add_(1.0)
    be.lib.calls.clear()
    be.assemble_matrix()
    assert be.lib.calls == ["knp_assemble_matrix"]
    be.unpack()
    assert _assemble(be) == ["knp_fields_unchanged", "knp_assemble_matrix_async"]      # and gives it again after a quiet step


def test_write_before_the_unpack_withholds_it_too(be):
    """the marks span assembly to assembly: conservative, never a wrong promise"""
    _assemble(be)
    be.p.wh[0][1].x.array.mul_(2.0)
    be.unpack()
    assert _assemble(be) == ["knp_assemble_matrix_async"]


def test_rebinding_withholds_the_promise(be):
    _step(be)
    be.p.phi_m_prev = _function()
    assert _assemble(be) == ["knp_assemble_matrix_async"]
    be.unpack()
    be.p.wh[1][1] = _function()
    assert _assemble(be) == ["knp_assemble_matrix_async"]
