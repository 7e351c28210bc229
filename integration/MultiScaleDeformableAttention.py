"""Drop-in for the reference's only native seam: ``import MultiScaleDeformableAttention as MSDA``
(/root/reference/src/dprt/models/layers/ms_deform_attn.py:24), called as ``MSDA.ms_deform_attn_forward`` (:32-39) and
``MSDA.ms_deform_attn_backward`` (:58-66) -- upstream that is the Deformable-DETR CUDA extension.

Put this directory on PYTHONPATH in place of the CUDA extension and the reference file runs unchanged on MI355X: the two
functions bind ``dpft_msda_fwd_f32`` / ``dpft_msda_bwd_f32`` (float32) and ``dpft_msda_fwd_typed`` / ``dpft_msda_bwd_typed``
(float16 / bfloat16) of libdpft_hip.so (include/dpft_hip.h) through ctypes -- plain pointers and sizes, the caller's current
stream, no torch types in the C signatures.  The library is looked up in $DPFT_HIP_LIB, next to the dpft_amd package of this
checkout, then on the loader path; there is NO fallback: a missing library or a failed launch raises.

Argument meaning and error behaviour follow the extension: CUDA(HIP) tensors, value (N, S, M, D) float32, float16 or bfloat16,
spatial_shapes (L, 2) int64 rows (H, W), level_start_index (L,) int64, sampling_loc (N, Lq, M, L, P, 2) in [0, 1] (x, y),
attn_weight (N, Lq, M, L, P); forward -> (N, Lq, M * D) in value's dtype; backward -> (grad_value, grad_sampling_loc,
grad_attn_weight), each in the dtype of the tensor it belongs to.  ``value`` sets the storage type of the kernels (fp32
arithmetic, every result rounded once).  sampling_loc may be float32 beside a 16-bit value (what ``torch.autocast`` produces;
it is read as it is, not rounded to 16 bits) or have value's dtype; attn_weight and grad_output of another float type are
cast to value's, as upstream's ``type_as``.  CPU tensors, a value of any other dtype and a sampling_loc that is neither
float32 nor value's dtype raise RuntimeError.  Unlike upstream there is no ``im2col_step`` divisibility requirement (the
argument is accepted and ignored).
"""
import ctypes
import os

import torch

_P, _I = ctypes.c_void_p, ctypes.c_int32


def _load():
    here = os.path.dirname(os.path.abspath(__file__))
    cands = [os.environ.get("DPFT_HIP_LIB"), os.path.join(here, "..", "dpft_amd", "libdpft_hip.so"), "libdpft_hip.so"]
    err = None
    for c in cands:
        if not c:
            continue
        try:
            return ctypes.CDLL(c)
        except OSError as e:
            err = e
    raise ImportError(f"MultiScaleDeformableAttention: libdpft_hip.so not found ({err}); build it with "
                      "`make -C dpft_amd/csrc ARCH=gfx950` or point DPFT_HIP_LIB at it")


_lib = _load()
_lib.dpft_msda_fwd_f32.argtypes = [_P] * 6 + [_I] * 7 + [_P]
_lib.dpft_msda_fwd_f32.restype = _I
_lib.dpft_msda_bwd_f32.argtypes = [_P] * 9 + [_I] * 7 + [_P]
_lib.dpft_msda_bwd_f32.restype = _I
_lib.dpft_msda_fwd_typed.argtypes = [_P] * 6 + [_I] * 9 + [_P]
_lib.dpft_msda_fwd_typed.restype = _I
_lib.dpft_msda_bwd_typed.argtypes = [_P] * 10 + [_I] * 9 + [_P]
_lib.dpft_msda_bwd_typed.restype = _I
_lib.dpft_last_error.restype = ctypes.c_char_p

_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}      # the `dtype` argument of the typed entries


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(rc, what):
    if rc:
        raise RuntimeError(f"{what}: {_lib.dpft_last_error().decode('utf-8', 'replace')} (rc={rc})")


def _operands(value, spatial_shapes, level_start_index, sampling_loc, attn_weight):
    for name, t in (("value", value), ("sampling_loc", sampling_loc), ("attn_weight", attn_weight)):
        if not (t.is_cuda and t.is_floating_point()):
            raise RuntimeError(f"MultiScaleDeformableAttention: {name} must be a floating-point GPU tensor (got {t.dtype} on {t.device})")
    if value.dtype not in _DTYPES:
        raise RuntimeError(f"MultiScaleDeformableAttention: value must be float32, float16 or bfloat16 (got {value.dtype})")
    if sampling_loc.dtype not in (torch.float32, value.dtype):
        raise RuntimeError(f"MultiScaleDeformableAttention: sampling_loc must be float32 or value's {value.dtype} (got {sampling_loc.dtype})")
    if value.dim() != 4 or sampling_loc.dim() != 6 or attn_weight.dim() != 5:
        raise RuntimeError("MultiScaleDeformableAttention: value (N,S,M,D), sampling_loc (N,Lq,M,L,P,2), attn_weight (N,Lq,M,L,P)")
    return (value.contiguous(), spatial_shapes.to(device=value.device, dtype=torch.int64).contiguous(),
            level_start_index.to(device=value.device, dtype=torch.int64).contiguous(), sampling_loc.contiguous(),
            attn_weight.to(value.dtype).contiguous())


def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step):
    value, spatial_shapes, level_start_index, sampling_loc, attn_weight = _operands(
        value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = sampling_loc.shape
    out = value.new_empty(N, Lq, M * D)
    if value.dtype == torch.float32:
        rc = _lib.dpft_msda_fwd_f32(_p(value), _p(spatial_shapes), _p(level_start_index), _p(sampling_loc), _p(attn_weight),
                                    _p(out), N, S, M, D, Lq, L, P, _stream())
    else:
        rc = _lib.dpft_msda_fwd_typed(_p(value), _p(spatial_shapes), _p(level_start_index), _p(sampling_loc), _p(attn_weight),
                                      _p(out), N, S, M, D, Lq, L, P, _DTYPES[value.dtype],
                                      int(sampling_loc.dtype == torch.float32), _stream())
    _check(rc, "ms_deform_attn_forward")
    return out


def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step):
    attn_dtype = attn_weight.dtype
    value, spatial_shapes, level_start_index, sampling_loc, attn_weight = _operands(
        value, spatial_shapes, level_start_index, sampling_loc, attn_weight)
    N, S, M, D = value.shape
    _, Lq, _, L, P, _ = sampling_loc.shape
    if not (grad_output.is_cuda and grad_output.is_floating_point()):
        raise RuntimeError(f"MultiScaleDeformableAttention: grad_output must be a floating-point GPU tensor (got {grad_output.dtype} on {grad_output.device})")
    grad_output = grad_output.to(value.dtype).contiguous()
    gl, ga = torch.empty_like(sampling_loc), torch.empty_like(attn_weight)
    if value.dtype == torch.float32:
        gv = torch.zeros_like(value)
        rc = _lib.dpft_msda_bwd_f32(_p(value), _p(spatial_shapes), _p(level_start_index), _p(sampling_loc), _p(attn_weight),
                                    _p(grad_output), _p(gv), _p(gl), _p(ga), N, S, M, D, Lq, L, P, _stream())
    else:
        gv = torch.empty_like(value)
        sums = torch.empty(value.numel(), dtype=torch.float32, device=value.device)      # fp32 sums of grad_value (cleared by the entry)
        rc = _lib.dpft_msda_bwd_typed(_p(value), _p(spatial_shapes), _p(level_start_index), _p(sampling_loc), _p(attn_weight),
                                      _p(grad_output), _p(gv), _p(gl), _p(ga), _p(sums), N, S, M, D, Lq, L, P,
                                      _DTYPES[value.dtype], int(sampling_loc.dtype == torch.float32), _stream())
    _check(rc, "ms_deform_attn_backward")
    return gv, gl, ga.to(attn_dtype)
