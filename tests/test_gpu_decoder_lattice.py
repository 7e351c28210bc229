"""The fused INFERENCE decoder (dpft_amd/csrc/decoder.hip through dpft_amd/models/fusers/fused.py) against the fp64 oracle over the
geometry lattice of tests/decoder_lattice.py: chunk, slice and staging edges of the score kernel, the soft-max fallback, row tails,
one and two iterations, short and mixed slot tables, one-pixel levels, four views, 1 and 16 classes, projection and shape forms.
The CPU half (tests/test_decoder_lattice.py) shows that every case reaches its edge and that its inputs let no error hide.

The rule is the one of test_product_fuser_forward_matches_reference_golden, rtol 1e-4 and atol 1e-5 max|ref|, written as a distance:
max |out - ref| / (rtol |ref| + atol) <= 1.  Should a correct kernel miss it (__expf, exp2, rcp, the one-exp Mish), the yardstick is
the distance of the fp32 CPU evaluation of the same oracle from its fp64 value, recomputed here, with a margin of 4x as in the
self-attention lattice (a different but equally rounded evaluation); both distances are printed for every case."""
import copy
from collections import OrderedDict

import pytest
import torch

from tests import decoder_lattice as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _device_fuser(c):
    """A fresh copy of the case's module on the GPU (its fused decoder packs its weights on the first eval forward)."""
    return copy.deepcopy(L.cached(c)[0]).to(DEV).eval()


def _device_inputs(c):
    inp = L.cached(c)[1]
    return dict(views=[OrderedDict((k, v.to(DEV)) for k, v in lv.items()) for lv in inp["views"]],
                shape=[s.to(DEV) for s in inp["shape"]], projection=[(T.to(DEV), P.to(DEV)) for T, P in inp["projection"]],
                center0=inp["center0"].to(DEV))


def _forward(fuser, dinp, shape=None, projection=None, flags=None):
    """eval + no_grad forward -> dict of CPU tensors with "center" as center - center0."""
    with torch.no_grad():
        out = fuser(batch=dinp["views"], shape=dinp["shape"] if shape is None else shape,
                    projection=dinp["projection"] if projection is None else projection,
                    out=OrderedDict(center=dinp["center0"].clone()), has_transformation=flags)
        res = OrderedDict((k, out[k].clone()) for k in L.KEYS)
        res["center"] = res["center"] - dinp["center0"]
    torch.cuda.synchronize()
    return OrderedDict((k, v.cpu()) for k, v in res.items())


_RUNS = {}


def _fused_run(c):
    """One fused forward per case, shared by the tests below: (module, device inputs, outputs)."""
    if c.name not in _RUNS:
        fuser, dinp = _device_fuser(c), _device_inputs(c)
        out = _forward(fuser, dinp)
        assert fuser.__dict__.get("_fused_decoder"), "the fused inference decoder did not run"
        _RUNS[c.name] = (fuser, dinp, out)
    return _RUNS[c.name]


def _assert_rule(c, what, got, ref64, ref32):
    d, d32 = L.distance(got, ref64), L.distance(ref32, ref64)
    print(f"{c.name:15s} {what:7s} distance {d:8.4f} of the tolerance   fp32 oracle {d32:8.4f}")
    assert torch.isfinite(got).all(), (c.name, what, "NaN / Inf")
    assert d <= max(1.0, 4.0 * d32), (c.name, what, d, d32)


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_outputs_match_fp64_oracle(c):
    """center - center0, size, angle and class of the fused decoder against the fp64 oracle; no NaN / Inf; argmax(class) equal
    wherever the fp64 top-2 margin exceeds ten times the absolute tolerance (at most 5 % of the rows are exempt: CPU half)."""
    out64, out32 = L.cached(c)[2], L.cached(c)[4]
    _, _, out = _fused_run(c)
    for k in L.KEYS:
        _assert_rule(c, k, out[k], out64[k], out32[k])
    rows = L.argmax_rows(out64["class"])
    assert torch.equal(out["class"].argmax(-1)[rows], out64["class"].argmax(-1)[rows]), c.name


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_attn0_matches_fp64_first_layer_attention(c):
    """FusedDecoder.attn0 (dpft_decoder_attn0_f32: the score kernel on the packed rows) against softmax(q k^T / sqrt(2)) v in
    fp64: pins a failure to the score kernel."""
    a64, a32 = L.cached(c)[5], L.cached(c)[6]
    fuser, _, _ = _fused_run(c)
    attn0 = fuser.__dict__["_fused_decoder"].attn0
    assert attn0 is not None
    _assert_rule(c, "attn0", attn0.view(L.n_views(c), c.Q, 16).cpu(), a64, a32)


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_second_launch_is_bit_equal(c):
    """A second launch() on the same descriptor: the tickets are left usable and nothing is accumulated."""
    fuser, dinp, out = _fused_run(c)
    again = fuser.__dict__["_fused_decoder"].launch()
    torch.cuda.synchronize()
    for k in L.KEYS:
        got = again[k] - dinp["center0"] if k == "center" else again[k]
        assert torch.equal(got.cpu(), out[k]), (c.name, k)


@pytest.mark.parametrize("name", ["anchor", "q1"])
def test_first_launch_computing_the_scores_is_bit_equal(name, monkeypatch):
    """DPFT_DEC_ATTN0=0 (read when the weights are packed): the first launch computes the first layer's scores itself -- the
    same block on the same values."""
    c = L.by_name(name)
    _, dinp, out = _fused_run(c)
    monkeypatch.setenv("DPFT_DEC_ATTN0", "0")
    fuser = _device_fuser(c)
    got = _forward(fuser, dinp)
    dec = fuser.__dict__.get("_fused_decoder")
    assert dec and dec.attn0 is None
    for k in L.KEYS:
        assert torch.equal(got[k], out[k]), (name, k)


def test_forms_are_bit_equal():
    """One set of values with `transformation.any()` left to the device (an all-zero T among the views) and given, a (B,3,4) and
    a (B,4,4) projection, shape as int64 (B,2), as int64 rows of a (B,3) tensor read in place, and as int32."""
    c = L.by_name("forms")
    fuser, dinp, out = _fused_run(c)
    inp = L.cached(c)[1]
    for form in L.FORMS:
        shape, projection, flags = L.form_inputs(inp, form)
        shape = [s.to(DEV) for s in shape]
        projection = [(T.to(DEV), P.to(DEV)) for T, P in projection]
        if form == "shape-stride3":
            assert all(s.stride(0) == 3 and s.dtype == torch.int64 for s in shape)
        if form == "p4":
            assert all(P.shape[1] == 4 for _, P in projection)
        got = _forward(fuser, dinp, shape, projection, flags)
        dec = fuser.__dict__["_fused_decoder"]
        assert dec.desc.shape_stride == (3 if form == "shape-stride3" else 2), form
        assert list(dec.desc.has_t)[:3] == ([0, 1, 0] if form == "flags" else [-1, -1, -1]), form
        for k in L.KEYS:
            assert torch.equal(got[k], out[k]), (form, k)


@pytest.mark.parametrize("name", ["anchor", "below-slices"])
def test_eager_decoder_matches_fp64_oracle(name):
    """The eager GPU decoder (use_fused_inference = False) under the same rule: a red test above then says which decoder moved."""
    c = L.by_name(name)
    out64, out32 = L.cached(c)[2], L.cached(c)[4]
    fuser = _device_fuser(c)
    fuser.use_fused_inference = False
    out = _forward(fuser, _device_inputs(c))
    assert not fuser.__dict__.get("_fused_decoder")
    for k in L.KEYS:
        _assert_rule(c, "eager " + k, out[k], out64[k], out32[k])


def test_more_queries_than_the_lds_holds_are_refused():
    """A direct FusedDecoder on a module over the library's limit is refused before anything is packed or launched."""
    from dpft_amd.hip.lib import HipLibraryError
    from dpft_amd.models.fusers import fused
    qmax = L.limits()[3]
    big = L.make_fuser(L.by_name("q1")._replace(name="over", Q=qmax + 1)).to(DEV)
    assert not fused.supported(big)
    with pytest.raises(HipLibraryError, match=f"at most {qmax}"):
        fused.FusedDecoder(big)
