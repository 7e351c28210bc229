"""The BatchNorm passes of bn.hip, one launch at a time through the storage-typed C entries, against the fp64 reference of
tests/bn_lattice.py: every element, mask byte, fp32 copy, parameter gradient and cleared buffer bit for bit in the exact tier, guard
words around every output, and the kernel form the library reports against the dispatch restatement (tests/bn_passes_driver.py).

test_float_tier: Gaussian data, every element within the derived bound c u T (c = 8, tests/bn_lattice.py)."""
import os
import subprocess
import sys

import pytest

from tests import bn_lattice as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SW = L.switches_from_env(os.environ)


@pytest.mark.parametrize("K", L.K_VALUES + L.K_EXTRA + ("trips",))
def test_exact_tier_elementwise_and_reduce(K):
    from tests import bn_passes_driver as D
    for c in L.LATTICE:
        if (c.name.startswith("trips") and K == "trips") or (not c.name.startswith("trips") and c.K == K):
            D.run_case(c, SW)


def test_exact_tier_pool_with_planted_ties():
    from tests import bn_passes_driver as D
    for c in L.POOL_LATTICE:
        D.run_pool_case(c, SW)


@pytest.mark.parametrize("c", L.SUMS_CASES, ids=[c.name for c in L.SUMS_CASES])
def test_column_sums_taken_and_declined(c):
    from tests import bn_passes_driver as D
    D.run_sums_case(c, SW)


def test_add_and_cvt_round_to_nearest_even():
    from tests import bn_passes_driver as D
    D.run_add_cvt()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", L.FLOAT_CASES, ids=[c.name for c in L.FLOAT_CASES])
def test_float_tier(c, bf16):
    from tests import bn_passes_driver as D
    worst, fails = D.run_float_case(c, SW, bf16)
    assert not fails, fails


def test_lattice_under_each_dispatch_switch():
    """Fresh child processes, one after the other, each with one switch changed; stops at the first that fails."""
    for changed in L.SWITCH_RUNS:
        env = dict(os.environ)
        for k, v in changed.items():
            env[L.SWITCH_ENV[k]] = str(v)
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bn_lattice_child.py")], env=env, capture_output=True,
                             text=True, timeout=240)
        assert res.returncode == 0, (changed, res.returncode, res.stdout[-1500:], res.stderr[-3000:])
