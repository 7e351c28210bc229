"""Child process of tests/test_gpu_conv_stats.py::test_reduction_launch_forms_in_a_child_process: the forced K splits of the
statistics lattice (tests/stats_lattice.py) with DPFT_SK_FIXUP=0 in the environment (the library reads it once per process), so
that they end in splitk_reduce_stats_kernel or in the plain reduction + bn_stats_kernel.  Exit status 0 = every launch passed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import conv_stats_driver as D    # noqa: E402

if __name__ == "__main__":
    D.run_child()
