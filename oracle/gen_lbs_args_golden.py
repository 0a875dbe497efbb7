"""TEST INFRASTRUCTURE -- records tests/golden/lbs_args.npz: the outputs of the three SrLbsArgs launches on the case of
tests/test_deformer_tracer_gpu.py::lbs_args_outputs, for test_lbs_struct_arguments_give_the_recorded_bits.  Needs the GPU:
    python -m oracle.gen_lbs_args_golden [OUT.npz]"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_deformer_tracer_gpu as t  # noqa: E402

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lbs_args.npz")
np.savez_compressed(path, **{k: v.numpy() for k, v in t.lbs_args_outputs().items()})
print("wrote", path, os.path.getsize(path), "bytes")
