"""Restatements of interp2x_boundary3d_kernel.cu:11-151 in numpy: the voxel-by-voxel loop, and the same thing as strided slices for
volumes the loop is too slow for.  Both sum a fine voxel's 1/2/4/8 coarse parents in the array's own precision, in the reference's
parent order, and divide in double; the flag is "the parents' (v > balance) do not all agree"."""
import numpy as np


def interp2x_loop(a, bal):
    """[d,h,w] float32 -> ([2d-1,2h-1,2w-1] float32, flags)."""
    d, h, w = a.shape
    D, H, W = 2 * d - 1, 2 * h - 1, 2 * w - 1
    out = np.zeros((D, H, W), np.float32); bnd = np.zeros((D, H, W), bool)
    for z in range(D):
        for y in range(H):
            for x in range(W):
                zs = [z // 2] if z % 2 == 0 else [(z - 1) // 2, (z + 1) // 2]
                ys = [y // 2] if y % 2 == 0 else [(y - 1) // 2, (y + 1) // 2]
                xs = [x // 2] if x % 2 == 0 else [(x - 1) // 2, (x + 1) // 2]
                if len(zs) == 2 and len(ys) == 2 and len(xs) == 2: order = [(zz, yy, xx) for zz in zs for yy in ys for xx in xs]
                elif len(zs) == 1: order = [(zs[0], yy, xx) for yy in ys for xx in xs]
                elif len(xs) == 1: order = [(zz, yy, xs[0]) for yy in ys for zz in zs]
                else: order = [(zz, ys[0], xx) for xx in xs for zz in zs]
                vals = [a[p] for p in order]
                s = np.float32(vals[0])
                for v in vals[1:]:
                    s = np.float32(s + v)
                out[z, y, x] = s if len(vals) == 1 else np.float32(np.float64(s) / len(vals))
                bnd[z, y, x] = len({bool(v > bal) for v in vals}) > 1
    return out, bnd


def _parent_shifts(oz, oy, ox):
    """(sz, sy, sx) of the parents of a fine voxel with the parities (oz, oy, ox), in the order the reference adds them: z outer and
    x inner for 8 parents (:119-126) and for the z-even face (:71-74), y outer and z inner for the x-even face (:86-89), x outer and
    z inner for the y-even face (:102-105).  A shift on an even axis is always 0."""
    zs, ys, xs = ((0, 1) if o else (0,) for o in (oz, oy, ox))
    if oz and oy and ox or not oz:
        return [(sz, sy, sx) for sz in zs for sy in ys for sx in xs]
    if not ox:
        return [(sz, sy, 0) for sy in ys for sz in zs]
    return [(sz, 0, sx) for sx in xs for sz in zs]


def interp2x_vectorised(a, bal):
    """[..., d, h, w] float32 or float64 -> ([..., 2d-1, 2h-1, 2w-1] of the same type, flags): one strided assignment per parity class."""
    d, h, w = a.shape[-3:]
    lead = a.shape[:-3]
    out = np.zeros(lead + (2 * d - 1, 2 * h - 1, 2 * w - 1), a.dtype)
    bnd = np.zeros(out.shape, bool)
    level = a.dtype.type(np.float32(bal))                         # the kernels take the level as a float and compare in the volume's type

    def parent(odd, shift):                                       # the coarse neighbours below (shift 0) / above (1) the odd fine voxels
        return slice(None) if not odd else slice(0, -1) if shift == 0 else slice(1, None)

    for oz in (0, 1):
        for oy in (0, 1):
            for ox in (0, 1):
                vals = [a[..., parent(oz, sz), parent(oy, sy), parent(ox, sx)] for sz, sy, sx in _parent_shifts(oz, oy, ox)]
                s = vals[0].copy()
                differ = np.zeros(s.shape, bool)
                for v in vals[1:]:
                    s = s + v                                     # stays in a.dtype: one rounding per parent, as the loop
                    differ |= (v > level) != (vals[0] > level)
                if len(vals) > 1:
                    s = (s.astype(np.float64) / len(vals)).astype(a.dtype)
                out[..., oz::2, oy::2, ox::2] = s
                bnd[..., oz::2, oy::2, ox::2] = differ
    return out, bnd
