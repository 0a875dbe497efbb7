"""Drop-in for the reference's `MCGpu` pybind module (MCGpu/MCGpu.cpp:14-60).

    mc_gpu(sdfs[NX,NY,NZ] f32 GPU contiguous, xstep=1, ystep=1, zstep=1, xmin=0, ymin=0, zmin=0, fTargetValue=0)
        -> [verts[V,3] f32, faces[F,3] int64]
    mc_init(device_id)

Error convention kept from the reference: wrong dtype / non-positive dims return an EMPTY LIST (MCGpu.cpp:41-48); non-GPU /
non-contiguous input raises (the CHECK_INPUT macro, :3-5,31).  The reference also returns [] for a device index outside [0, 8)
(:43-45) -- the size of its fixed array of per-device singletons.  There is no such array here (workspace and outputs are sized
per call, on the caller's stream, and the output order is deterministic), so every device index works: on a node that exposes more
than 8 logical devices (CPX partitions, 16-GPU boxes) the reference's limit would only turn the first remesh into an unpack error.
"""
import torch
from .. import _lib


def mc_init(device_id):
    return None      # nothing to pre-allocate: tables are uploaded on first use


def mc_gpu(sdfs, xstep=1.0, ystep=1.0, zstep=1.0, xmin=0.0, ymin=0.0, zmin=0.0, fTargetValue=0.0):
    if not sdfs.is_cuda:
        raise RuntimeError("sdfs must be a CUDA tensor")
    if not sdfs.is_contiguous():
        raise RuntimeError("sdfs must be contiguous")
    if sdfs.dtype != torch.float32 or sdfs.dim() != 3:
        return []
    nx, ny, nz = sdfs.shape
    if nx <= 0 or ny <= 0 or nz <= 0:
        return []
    dev = sdfs.device
    ws = _lib.workspace("sr_mc_workspace_bytes", nx, ny, nz, device=dev)
    counts = torch.zeros((2,), dtype=torch.int32, device=dev)
    _lib.launch("sr_mc_count", sdfs, sdfs, nx, ny, nz, float(fTargetValue), ws, counts)
    nv, nf = counts.tolist()                           # the one host sync (the reference has the same one)
    verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((nf, 3), dtype=torch.int64, device=dev)
    if nv or nf:
        # a cell next to the far faces of the volume can emit a face whose three edges no cell owns -- F = 1, V = 0 -- and an empty tensor
        # has no address to pass: sr_mc_emit gets one row it will not touch
        _lib.launch("sr_mc_emit", sdfs, sdfs, nx, ny, nz, float(fTargetValue), ws, float(xstep), float(ystep), float(zstep), float(xmin), float(ymin),
                    float(zmin), verts if nv else verts.new_empty((1, 3)), faces if nf else faces.new_empty((1, 3)))
    return [verts, faces]
