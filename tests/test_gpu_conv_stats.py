"""The train-mode BatchNorm statistics every conv forward emits, per tile and per producing form, against fp64
(reference, bounds and the plan restatement: tests/stats_lattice.py; the launches: tests/conv_stats_driver.py).

Per launch: dpft_conv2d_stats_tiles reports the planned tile height, the table (NaN before the launch, guard words around it) is
finite everywhere, y is bit-identical to the launch without statistics and to fp64, the profile names the planned kernel family,
and EVERY tile's mean and M2 of EVERY channel is within the bound derived for its producer: the mean bit for bit where the tile's
column sum is exact (the lattice's integer operands: everywhere in these cases).  The split kind comes from the restated host
plan, which tests/test_stats_lattice.py holds against the library's host queries and which the `sums used` flag confirms on the
device.  The fixed-point column sums go through dpft_conv2d_nhwc_fwd_sums_f32 / dpft_bn_finalize_sums_f32, one launch at a time.

Worst measured error / bound per form (MI355X; mean ratio / M2 ratio, 0 = every mean compared bit for bit):
  pipe, vec (bf16 operands) and x3 (split kernels) alike: unsplit 0 / 0.490, fix-up 0 / 0.290, plain reduction + bn_stats_kernel
  0 / 0.598; generic kernel 0 / 0.057; streaming kernel 0.026 / 0.015; splitk_reduce_stats_kernel (child) 0.969 / 0.580.
  Column sums: sum 1 equal word for word everywhere; sum 2 at 0.500 of its bound on every tiled form (one fp64 ulp: the fused
  form of M2 + cnt mean^2), 0.015 on the streaming kernel.  Finalize of the sums: mean 0.962 (a half ulp), invstd 0.421,
  scale 0.440, running_mean 0.472, running_var 0.393."""
import os
import subprocess
import sys

import pytest

from tests import stats_lattice as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the groups whose launches also go through the column-sums entry (taken unsplit and with the fix-up, on the split kernels and
# the bf16-operand kernel; declined behind a reduction launch)
SUMS_GROUPS = {("fp32+split", None), ("fp32", "128,64,2"), ("bf16x3", "128,128,1"), ("bf16x3", "64,64,3"), ("bf16", None)}


def _report(D):
    print("worst error / bound per form:", D.report())


@pytest.mark.parametrize("mode,tile", S.GROUPS, ids=[f"{m}-{t or 'auto'}" for m, t in S.GROUPS])
def test_tile_table_of_the_vector_path(mode, tile, monkeypatch):
    """Every small C % 64 == 0 case of the geometry lattice, without and with the BatchNorm + ReLU prologue: the unsplit epilogue,
    the in-launch fix-up and the plain reduction + bn_stats_kernel (K % 4 != 0), on the pipelined fp32 kernel, the split
    kernels (bf16x3 with a forced tile) and the bf16-operand kernel."""
    from tests import conv_stats_driver as D
    if tile:
        monkeypatch.setenv("DPFT_FORCE_TILE", tile)
    else:
        monkeypatch.delenv("DPFT_FORCE_TILE", raising=False)
    D.run_group(mode, tile, sums=(mode, tile) in SUMS_GROUPS)
    reached = {S.form_name(S.launch_plan(l)) for l in S.group_launches(mode, tile)}
    assert reached <= set(D.WORST), reached - set(D.WORST)
    _report(D)


def test_tile_table_of_the_generic_and_streaming_kernels(monkeypatch):
    """The generic kernel (C = 3 stem-shaped, generic class, C % 64 == 32) and the streaming 1x1 kernel at its smallest maps
    (a last workgroup with idle waves, a ragged last row block), without and with the prologue; their column sums declined /
    taken; statistics with a bias refused on a streaming shape with nothing written."""
    from tests import conv_stats_driver as D
    monkeypatch.delenv("DPFT_FORCE_TILE", raising=False)
    for l in S.other_launches():
        D.run_group(l.mode, None, sums=True, launches=[l])
    assert {"generic/unsplit", "stream/unsplit", "sums stream/unsplit"} <= set(D.WORST)
    for c in S.STREAM[:2]:
        with D.mode_ctx("fp32+split") as ops:
            D.run_stream_refusal(ops, c, "fp32+split")
    _report(D)


def test_every_form_is_reached():
    """The forms the issue lists, each by at least one launch of this module (the reduction + statistics kernel: in the child)."""
    assert set(S.REQUIRED_FORMS) <= S.forms_reached(), set(S.REQUIRED_FORMS) - S.forms_reached()
    assert set(S.REQUIRED_CHILD_FORMS) <= S.forms_reached(child=True)


def test_reduction_launch_forms_in_a_child_process():
    """DPFT_SK_FIXUP=0 (read once per process) turns the fix-up off: the forced K splits end in splitk_reduce_stats_kernel
    (K % 64 == 0) or in the plain reduction followed by bn_stats_kernel; the column sums are declined there."""
    env = dict(os.environ, DPFT_SK_FIXUP="0")
    env.pop("DPFT_FORCE_TILE", None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "conv_stats_child.py")], env=env, capture_output=True, text=True,
                         timeout=240)
    assert res.returncode == 0, (res.returncode, res.stdout[-1500:], res.stderr[-3000:])
    print(res.stdout[-800:])


@pytest.mark.parametrize("mode,tile", [("fp32+split", None), ("fp32", "64,64,3"), ("bf16x3", "128,64,2"), ("bf16", None)],
                         ids=["fp32+split-auto", "fp32-64,64,3", "bf16x3-128,64,2", "bf16-auto"])
def test_prologue_from_column_sums_is_the_prologue_from_the_finalized_block(mode, tile, monkeypatch):
    """`the same arithmetic everywhere` (common.h): where the plan offers the prologue from sums (pipelined fp32 and split
    kernels, the streaming kernel) the conv is bit-identical to the one given the BN block dpft_bn_finalize_sums_f32 makes of
    the same sums; refused elsewhere (the bf16-operand kernel)."""
    from tests import conv_stats_driver as D
    if tile:
        monkeypatch.setenv("DPFT_FORCE_TILE", tile)
    else:
        monkeypatch.delenv("DPFT_FORCE_TILE", raising=False)
    took = set()
    with D.mode_ctx(mode, tile) as ops:
        cases = S.C64[::3] + (S.STREAM[1:] if tile is None else [])
        for c in cases:
            took.add(D.run_pro_from_sums(ops, S.Launch(c, mode, tile, True)))
    assert took == ({False} if mode == "bf16" else {True}), took


def test_finalize_of_the_column_sums():
    from tests import conv_stats_driver as D
    D.run_finalize_sums()
    _report(D)
