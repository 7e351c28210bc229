"""bn_stats_kernel and bn_finalize_kernel called directly (ops.bn_stats / ops.bn_finalize) at their own edges: K below, at and
above the 256-column slab and off the finalize block's 32 channels, tile heights 64 / 128 / 256, M below a tile and M == 1, ragged
last tiles, 1 / 32 / 33 / 65 tiles (the finalize kernel strides tiles by 32).  Cases, data and bounds: tests/stats_lattice.py.

Exact tier: integer data whose tile means are quarter-integers -- the table equals fp64 bit for bit, and with momentum = 1
running_mean is the mean and running_var the correctly rounded M2 / (M - 1).
Float tier: Gaussian columns offset by up to 200 standard deviations (the stem's raw inputs: the pivot of bn_finalize_kernel must
keep S2 - S1^2 / M from cancelling) -- tile table, mean, invstd, scale and both running statistics within the derived bounds.

Worst measured error / bound (MI355X): bn_stats_kernel tile mean 0.325, tile M2 0.175; bn_finalize_kernel mean 0.966 (a half ulp
of the result), invstd 0.261, scale 0.304, running_mean 0.519, running_var 0.366; exact tier invstd 0.490, scale 0.547."""
import pytest

from tests import stats_lattice as S

pytestmark = pytest.mark.gpu
_id = lambda c: "x".join(map(str, c))


@pytest.mark.parametrize("case", S.EXACT_CASES, ids=_id)
def test_exact_tier_equals_fp64_bit_for_bit(case):
    from tests import conv_stats_driver as D
    D.run_bn_exact(case)


@pytest.mark.parametrize("case", S.FLOAT_CASES, ids=_id)
def test_float_tier_with_offsets_of_200_sigma(case):
    from tests import conv_stats_driver as D
    D.run_bn_float(case)
    print("worst error / bound:", D.report())
