"""TEST INFRASTRUCTURE -- shared deterministic inputs (thin re-export of the product's
synthetic-input helpers so that the reference run and the tests build identical tensors)."""
from selfreconcode_amd.synthetic import (  # noqa: F401
    det_array, det_tensor, det_params, det_normal, sphere_sdf_params, synthetic_joints, synthetic_lbs_volume,
    SDF_SPEC, DEF_SPEC, REND_SPEC, LBS_BMIN, LBS_BMAX, SMPL_PARENTS, cube_sphere, icosphere,
)


def digest(a):
    """sha256 of an array's shape and values (floats widened to float64, integers and booleans to int64, both exact): the committed
    form of a bit-equality check -- digest(a) == digest(b) exactly when a.shape == b.shape and np.array_equal(a, b)."""
    import hashlib
    import numpy as np
    a = np.asarray(a)
    a = np.ascontiguousarray(a, dtype=np.float64 if a.dtype.kind == "f" else np.int64)
    h = hashlib.sha256(repr(a.shape).encode())
    h.update(a.tobytes())
    return h.hexdigest()
