"""TEST INFRASTRUCTURE -- records tests/golden/mesh_bits.npz: the SHA-256 of every output of the mesh and reduction kernels on the
cases of tests/test_mesh_bits_gpu.py::mesh_kernel_digests, for test_every_mesh_kernel_gives_the_recorded_bits.  Needs the GPU:
    python -m oracle.gen_mesh_bits_golden [OUT.npz]"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_mesh_bits_gpu as t  # noqa: E402

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "mesh_bits.npz")
np.savez_compressed(path, digests=np.stack([v.numpy() for v in t.mesh_kernel_digests().values()]))     # [183,32] uint8, in that order
print("wrote", path, os.path.getsize(path), "bytes")
