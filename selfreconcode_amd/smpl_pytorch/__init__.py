"""Mirror of the reference's smpl_pytorch package: the SMPL body model on the HIP kernels of csrc/smpl.hip."""
from .SMPL import SMPL, DifferentiableSMPL, getSMPL, load_model  # noqa: F401
