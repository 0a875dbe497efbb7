"""Host-side mirrors of the reference's model/ modules (same class names, call signatures and
state_dict keys), computing on the HIP kernels of libselfrecon_hip.so."""
from .Deformer import initial_lbs_skinner, initialLBSkinner, compute_lbswField, smooth_weights  # noqa: E402,F401


def __getattr__(name):
    if name == "getOptNet":                      # resolved on first use: importing the package does not import model.network
        from .network import getOptNet
        return getOptNet
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
