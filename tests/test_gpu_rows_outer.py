"""dpft_rows_outer_f32 (rows_outer_kernel, misc.hip) -- every weight and bias gradient of the training decoder -- element by
element against fp64 over the shape lattice of tests/outer_lattice.py: the compact and the dense grid, the vector loop and the
scalar loop for each of its causes, partial tiles, R on either side of the 64 row groups, gapped output strides, 40 specs.

Exact pass: integer operands, so every summation order gives the fp64 result bit for bit; the output is poisoned with a NaN of a
known bit pattern, and every float the call must not write (gaps, the stride's tail, guard floats on both sides of the buffer)
still holds it afterwards.  Float pass: standard normal operands against a derived rounding bound.  Called through
dpft_amd.hip.lib exactly as train_fused._rows_outer does."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import outer_lattice as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = 0x7FC0DEAD                   # a quiet NaN no arithmetic produces
GUARD = 64                            # guard floats before and after `out`
U = 2.0 ** -24                        # fp32 unit roundoff

_refs = {}


def _reference(c, float_pass):
    """(rows fp32 CPU, fp64 reference, fp64 sum of |a * b|) -- computed once per case and pass, shared, never modified."""
    key = (c.name, float_pass)
    if key not in _refs:
        x = L.operands(c, float_pass)
        _refs[key] = (x, L.reference(x, c), L.reference(x, c, absolute=True) if float_pass else None)
    return _refs[key]


def _rows_on_device(c, x):
    """``x`` at ``ptr_off`` floats past a 16-byte boundary."""
    buf = torch.empty(x.numel() + 8, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    rows = buf[c.ptr_off:c.ptr_off + x.numel()]
    rows.copy_(x.reshape(-1))
    assert rows.data_ptr() % 16 == 4 * c.ptr_off
    return rows


def _poisoned(n):
    return torch.full((GUARD + n + GUARD,), POISON, dtype=torch.int32, device=DEV)


def _call(rows, G, R, W, specs, out_buf, out_gstride, n_specs=None):
    from dpft_amd.hip.lib import OuterSpec, lib, stream
    arr = (OuterSpec * max(len(specs), 1))(*[OuterSpec(*s) for s in specs])
    lib.call("dpft_rows_outer_f32", rows.data_ptr(), G, R, W, C.cast(arr, C.c_void_p), len(specs) if n_specs is None else n_specs,
             out_buf.data_ptr() + 4 * GUARD, out_gstride, stream())


def _run(c, x):
    rows = _rows_on_device(c, x)
    out = _poisoned(c.G * c.out_gstride)
    _call(rows, c.G, c.R, c.W, c.specs, out, c.out_gstride)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_untouched(c, bits):
    n = c.G * c.out_gstride
    covered = L.covered_mask(c)
    assert (bits[:GUARD] == POISON).all() and (bits[GUARD + n:] == POISON).all(), f"{c.name}: guard floats overwritten"
    body = bits[GUARD:GUARD + n]
    bad = np.flatnonzero(body[~covered] != POISON)
    assert bad.size == 0, f"{c.name}: {bad.size} uncovered floats written, first at uncovered index {bad[:5]}"
    return body, covered


@pytest.mark.parametrize("case", L.LATTICE, ids=lambda c: c.name)
def test_rows_outer_integer_operands_equal_fp64_bit_for_bit(case):
    c = case
    x, ref, _ = _reference(c, False)
    bits = _run(c, x)
    body, covered = _check_untouched(c, bits)
    want = ref.float().numpy().view(np.int32)          # exact: the reference is an integer below 2^24
    bad = np.flatnonzero(body[covered] != want[covered])
    if bad.size:
        idx = np.flatnonzero(covered)[bad[:5]]
        got = body.view(np.float32)
        raise AssertionError(f"{c.name} ({L.dispatch(c).mode}): {bad.size} of {int(covered.sum())} covered floats differ from fp64; "
                             f"first at {idx.tolist()}: got {got[idx].tolist()}, want {ref.numpy()[idx].tolist()}")


@pytest.mark.parametrize("case", [c for c in L.LATTICE if c.R >= 63], ids=lambda c: c.name)
def test_rows_outer_normal_operands_within_the_rounding_bound(case):
    """|out - ref64| <= gamma_n * sum_r |a_r * b_r| per element, gamma_n = n u / (1 - n u), u = 2^-24, n = ceil(R / 64) + 18:
    a thread's chain is ceil(R / 64) fused multiply-adds (one rounding each: row groups are 64 apart), then 2 shuffle adds
    (the 4 row groups of a wave) and 16 ordered adds over the waves.  Derived, so no extra factor.  Two calls on the same input
    are bit-identical (fixed summation order)."""
    c = case
    x, ref, absref = _reference(c, True)
    bits = _run(c, x)
    body, covered = _check_untouched(c, bits)
    n = math.ceil(c.R / L.ROW_GROUPS) + 18
    gamma = n * U / (1 - n * U)
    got = body.view(np.float32).astype(np.float64)[covered]
    assert np.isfinite(got).all(), f"{c.name}: non-finite outputs"
    err = np.abs(got - ref.numpy()[covered])
    bound = gamma * absref.numpy()[covered]
    worst = int(np.argmax(err - bound))
    print(f"{c.name}: n = {n}, max err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), (f"{c.name}: {int((err > bound).sum())} elements above the bound; worst at covered index {worst}: "
                                  f"err {err[worst]:.3e} > {bound[worst]:.3e}")
    again = _run(c, x)
    assert np.array_equal(bits, again), f"{c.name}: two calls on the same input differ"


BAD_ARGS = [
    # name, G, R, W, specs, n_specs (None: len(specs))
    ("n_specs 0", 2, 8, 32, [(0, 4, 4, 4, 0)], 0),
    ("n_specs 41", 2, 8, 32, [(0, 1, 1, 1, i) for i in range(41)], None),
    ("col_a + n_a > W", 2, 8, 32, [(0, 4, 4, 4, 0), (17, 16, 0, 4, 16)], None),
    ("col_b + n_b > W", 2, 8, 32, [(0, 4, 29, 4, 0)], None),
    ("col_b < 0 with n_b != 1", 2, 8, 32, [(0, 4, -1, 2, 0)], None),
    ("n_a 0", 2, 8, 32, [(0, 0, 4, 4, 0)], None),
    ("negative out_off", 2, 8, 32, [(0, 4, 4, 4, -1)], None),
    ("G 0", 0, 8, 32, [(0, 4, 4, 4, 0)], None),
    ("R 0", 2, 0, 32, [(0, 4, 4, 4, 0)], None),
    ("W 0", 2, 8, 0, [(0, 4, 4, 4, 0)], None),
]


@pytest.mark.parametrize("bad", BAD_ARGS, ids=lambda b: b[0])
def test_rows_outer_argument_errors_raise_and_write_nothing(bad):
    from dpft_amd.hip.lib import HipLibraryError
    name, G, R, W, specs, n_specs = bad
    rows = torch.ones(2 * 8 * 32, dtype=torch.float32, device=DEV)
    out = _poisoned(4096)
    with pytest.raises(HipLibraryError, match="rows_outer"):
        _call(rows, G, R, W, specs, out, 1024, n_specs)
    torch.cuda.synchronize()
    assert bool((out == POISON).all()), f"{name}: refused call wrote to out"
    # the same buffers with valid arguments compute: the refusal above was about the argument alone
    _call(rows, 2, 8, 32, [(0, 4, 4, 4, 0)], out, 1024)
    torch.cuda.synchronize()
    got = out[GUARD:GUARD + 16].view(torch.float32)
    assert torch.equal(got, torch.full((16,), 8.0, device=DEV))
