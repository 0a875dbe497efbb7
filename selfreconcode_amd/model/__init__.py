"""Host-side mirrors of the reference's model/ modules (same class names, call signatures and
state_dict keys), computing on the HIP kernels of libselfrecon_hip.so."""
from .Deformer import initial_lbs_skinner, compute_lbswField, smooth_weights  # noqa: E402,F401
