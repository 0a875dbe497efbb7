"""TEST INFRASTRUCTURE -- records tests/golden/eval_bits.npz: the SHA-256 of everything the geometry evaluation hands out on the cases of
tests/test_eval_bits_gpu.py::eval_digests, for test_the_evaluation_stack_gives_the_recorded_bits.  Needs the GPU:
    python -m oracle.gen_eval_bits_golden [OUT.npz]"""
import os
import sys
import tempfile
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_eval_bits_gpu as t  # noqa: E402

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "eval_bits.npz")
with tempfile.TemporaryDirectory() as tmp:
    digests = t.eval_digests(tmp)
np.savez_compressed(path, digests=np.stack([v.numpy() for v in digests.values()]), names=np.array(list(digests)))     # [N,32] uint8, in that order
print("wrote", path, os.path.getsize(path), "bytes,", len(digests), "digests")
