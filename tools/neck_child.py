"""Child process of tests/test_gpu_neck_lattice.py::test_fused_forms_switched_off_in_a_child_process: the radar-5 and camera-3
cases of the neck lattice (tests/neck_lattice.py) with DPFT_FPN_FUSE=0 DPFT_BIAS_FUSE=0 DPFT_WGRAD16_TILED=0 in the environment
(the library reads them once per process), so that the top-down add, the positional embedding and the bias gradient run in their
own kernels and the conv16 weight gradient in its streaming form.  Prints every output's and gradient's distance to fp64, holds
them to the lattice's bound and saves the tensors to the path given as the only argument.  Exit status 0 = every check passed."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import neck_driver as D    # noqa: E402

if __name__ == "__main__":
    D.run_child(sys.argv[1])
