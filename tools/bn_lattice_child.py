"""Child process of tests/test_gpu_bn_passes.py::test_lattice_under_each_dispatch_switch: the whole BatchNorm pass lattice
(tests/bn_lattice.py) under the dispatch switches found in the environment (DPFT_BN_FIXC, DPFT_BN_WIDE16, DPFT_BN_FAT,
DPFT_POOL_BWD_TILED, DPFT_EW_BLOCKS_PER_CU -- the library reads them once per process).  Exit status 0 = every case passed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import bn_lattice as L          # noqa: E402
from tests import bn_passes_driver as D    # noqa: E402

if __name__ == "__main__":
    D.run_all(L.switches_from_env(os.environ))
