"""The slab-level region check of tests/test_region_gpu.py on one shape, in a process of its own so
that PFT_REGION_WGS (read at pft_slab_create) caps region_kernel's workgroups and its grid-stride
loop makes several trips:

    PFT_REGION_WGS=1 python tests/_region_wgs_worker.py <n1> <n2> <n3>

Exit status 0 and a last line "ok <number of images compared>" when every image equals numpy's."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import test_region_gpu as T  # noqa: E402


def main():
    n1, n2, n3 = (int(v) for v in sys.argv[1:4])
    assert int(os.environ["PFT_REGION_WGS"]) >= 1
    print("ok", T.check_slab(n1, n2, n3))


if __name__ == "__main__":
    main()
