"""TEST INFRASTRUCTURE -- records tests/golden/lbs_paths.npz: the SHA-256 of every output of the LBS and kinematic-chain kernels on
the cases of tests/test_lbs_paths_gpu.py::lbs_path_digests, for test_every_launch_path_gives_the_recorded_bits.  Needs the GPU:
    python -m oracle.gen_lbs_paths_golden [OUT.npz]"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_lbs_paths_gpu as t  # noqa: E402

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lbs_paths.npz")
np.savez_compressed(path, digests=np.stack([v.numpy() for v in t.lbs_path_digests().values()]))       # [36,32] uint8, in that order
print("wrote", path, os.path.getsize(path), "bytes")
