"""CPU-only checks of the typed multi-scale deformable attention entries (dpft_msda_fwd_typed / dpft_msda_bwd_typed): the C-ABI
surface, the argument errors (reported before any launch, so no GPU is needed and the pointers are never read), the shim's
bindings and the dtype rule of the Python wrappers."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_typed_entries_are_exported_and_have_signatures():
    from dpft_amd.hip.lib import SIGNATURES, lib
    dll = lib.load()
    for name, pointers in (("dpft_msda_fwd_typed", 6), ("dpft_msda_bwd_typed", 10)):
        assert hasattr(dll, name), f"{name} not exported"
        res, args = SIGNATURES[name]
        assert res is C.c_int32
        assert args == [C.c_void_p] * pointers + [C.c_int32] * 9 + [C.c_void_p]     # tensors, 7 sizes + dtype + loc32, stream


def test_typed_entries_report_argument_errors_before_any_launch():
    from dpft_amd.hip.lib import lib
    p = [C.c_void_p(4096 * (i + 1)) for i in range(10)]
    err = lambda: lib.dpft_last_error()
    dims = (1, 4, 2, 8, 3, 1, 1)                       # N, S, M, D, Lq, L, P

    def fwd(tensors=None, dims=dims, dtype=1, loc32=1):
        return lib.dpft_msda_fwd_typed(*(tensors or p[:6]), *dims, dtype, loc32, None)

    def bwd(tensors=None, ws=p[9], dims=dims, dtype=1, loc32=1):
        return lib.dpft_msda_bwd_typed(*(tensors or p[:9]), ws, *dims, dtype, loc32, None)
    for i in range(6):                                 # every tensor of the forward
        t = list(p[:6])
        t[i] = None
        assert fwd(tensors=t) == -1 and err().startswith(b"msda_fwd_typed:") and b"null" in err(), i
    for i in range(9):                                 # every tensor of the backward
        t = list(p[:9])
        t[i] = None
        assert bwd(tensors=t) == -1 and err().startswith(b"msda_bwd_typed:") and b"null" in err(), i
    for call, name in ((fwd, b"msda_fwd_typed:"), (bwd, b"msda_bwd_typed:")):
        assert call(dtype=3) == -1 and err().startswith(name) and b"dtype" in err()
        assert call(dtype=-1) == -1 and err().startswith(name) and b"dtype" in err()
        assert call(loc32=2) == -1 and err().startswith(name) and b"loc32" in err()
        assert call(dims=(1, 4, 2, 0, 3, 1, 1)) == -1 and err().startswith(name) and b"non-positive" in err()      # D = 0
        for k in range(7):
            d = list(dims)
            d[k] = 0
            assert call(dims=tuple(d)) == -1 and err().startswith(name), k
    for dtype in (1, 2):                               # 16-bit storage: the fp32 sums need their workspace
        assert bwd(ws=None, dtype=dtype) == -1 and err().startswith(b"msda_bwd_typed:") and b"workspace" in err()


def _shim():
    spec = importlib.util.spec_from_file_location("MultiScaleDeformableAttention",
                                                  os.path.join(ROOT, "integration", "MultiScaleDeformableAttention.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_shim_binds_the_typed_entries_and_refuses_cpu_half_tensors():
    m = _shim()
    assert m._lib.dpft_msda_fwd_typed.argtypes == [C.c_void_p] * 6 + [C.c_int32] * 9 + [C.c_void_p]
    assert m._lib.dpft_msda_bwd_typed.argtypes == [C.c_void_p] * 10 + [C.c_int32] * 9 + [C.c_void_p]
    assert m._lib.dpft_msda_fwd_typed.restype is C.c_int32 and m._lib.dpft_msda_bwd_typed.restype is C.c_int32
    shapes, lsi = torch.tensor([[2, 2]]), torch.tensor([0])
    for dt in (torch.float16, torch.bfloat16):
        value, attn = torch.zeros(1, 4, 2, 8, dtype=dt), torch.zeros(1, 3, 2, 1, 1, dtype=dt)
        for loc in (torch.zeros(1, 3, 2, 1, 1, 2, dtype=dt), torch.zeros(1, 3, 2, 1, 1, 2)):
            with pytest.raises(RuntimeError):
                m.ms_deform_attn_forward(value, shapes, lsi, loc, attn, 64)
            with pytest.raises(RuntimeError):
                m.ms_deform_attn_backward(value, shapes, lsi, loc, attn, torch.zeros(1, 3, 16, dtype=dt), 64)


@pytest.mark.parametrize("dtype", [torch.float64, torch.int32, torch.int64, torch.uint8])
def test_ops_refuse_other_value_dtypes_without_touching_the_library(dtype, monkeypatch):
    from dpft_amd.hip import ops
    from dpft_amd.hip.lib import HipLibraryError

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(type(ops.lib), "call", no_call)
    monkeypatch.setattr(type(ops.lib), "load", no_call)
    value = torch.zeros(1, 4, 2, 8).to(dtype)
    shapes, lsi = torch.tensor([[2, 2]]), torch.tensor([0])
    loc, attn, go = torch.zeros(1, 3, 2, 1, 1, 2), torch.zeros(1, 3, 2, 1, 1), torch.zeros(1, 3, 16)
    for fn in (ops.msda_fwd, ops.msda_fwd_typed):
        with pytest.raises((HipLibraryError, TypeError)):
            fn(value, shapes, lsi, loc, attn)
    for fn in (ops.msda_bwd, ops.msda_bwd_typed):
        with pytest.raises((HipLibraryError, TypeError)):
            fn(value, shapes, lsi, loc, attn, go)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_ops_refuse_cpu_tensors_without_touching_the_library(dtype, monkeypatch):
    from dpft_amd.hip import ops
    from dpft_amd.hip.lib import HipLibraryError

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(type(ops.lib), "call", no_call)
    monkeypatch.setattr(type(ops.lib), "load", no_call)
    value = torch.zeros(1, 4, 2, 8, dtype=dtype)
    shapes, lsi = torch.tensor([[2, 2]]), torch.tensor([0])
    loc, attn = torch.zeros(1, 3, 2, 1, 1, 2), torch.zeros(1, 3, 2, 1, 1, dtype=dtype)
    with pytest.raises((HipLibraryError, TypeError)):
        ops.msda_fwd(value, shapes, lsi, loc, attn)
    with pytest.raises((HipLibraryError, TypeError)):
        ops.msda_bwd(value, shapes, lsi, loc, attn, torch.zeros(1, 3, 16, dtype=dtype))
