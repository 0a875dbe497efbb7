"""Volumes that drive every launch path of csrc/mc.hip (tests/test_mc_paths_cpu.py asserts that each volume reaches its path,
tests/test_mc_paths_gpu.py runs the kernels on it).  Every volume is built from integers and the splitmix64 hash of
tests/test_mc_size_pin.py: no RNG state, no file -- a pure function of its name on every machine.

VOLUMES maps a name to (shape, kind, iso, path); volume(name) builds the float32 [NX,NY,NZ] array, reference(name) is the canonical
mesh of the sequential oracle (oracle/mc_oracle.c), computed once per process and read-only.  launch_plan(shape) restates the host
arithmetic of sr_mc_count / sr_mc_emit in integers; the four constants it uses are tied to the source text by the CPU tests."""
import functools
import numpy as np

from oracle import mc as mco
from test_mc_size_pin import _splitmix, volume as _shell

STEP, ORG = (0.1, 0.11, 0.09), (-1.0, -1.2, -0.7)       # the spacing / origin of tests/test_mc_reference_pin.py
MC_CHUNK = 16                     # groups of 64 voxels one wave of mc_classify_kernel sweeps
MC_BATCH = 4                      # groups whose loads are in flight together
SCAN_ITEMS = 2048                 # elements one workgroup of the exclusive scan covers
GRID_CAP = 2048                   # sr_stream_grid's cap on the number of workgroups
XCDS = 8

# corner b of a cell, as cube_case (mc.hip) and kVertexOffset (mc_oracle.c) number them
CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))


# ------------------------------------------------------------------------------------------------ the launch plan
def launch_plan(shape):
    """What sr_mc_count / sr_mc_emit launch for a volume of this shape (mc.hip: mc_classify_kernel's chunk split, exclusive_scan,
    the grid of the per-output kernels), in integers."""
    NX, NY, NZ = shape
    total = NX * NY * NZ
    G = (total + 63) // 64
    chunks = -(-G // MC_CHUNK)
    per_xcd = -(-chunks // XCDS)
    ranges = [max(0, min((x + 1) * per_xcd, chunks) - x * per_xcd) for x in range(XCDS)]           # chunks of each XCD's range
    grid = (min(GRID_CAP, max(1, -(-chunks * 64 // 256))) + 7) & ~7
    waves_per_xcd = (grid // XCDS) * 4
    out_grid = min(GRID_CAP, max(1, -(-min(G * 8, 1 << 22) // 256)))
    return dict(total=total, G=G, tail=total % 64, chunks=chunks, per_xcd=per_xcd, ranges=ranges, empty_xcds=ranges.count(0), grid=grid,
                waves_per_xcd=waves_per_xcd, second_chunk=max(ranges) > waves_per_xcd, scan_n=G + 1,
                scan_blocks=-(-(G + 1) // SCAN_ITEMS), tag_grid=min(GRID_CAP, max(1, -(-G // 256))), out_grid=out_grid,
                out_threads=out_grid * 256, planes_per_group=64 / (NY * NZ), rows_per_group=64 / NZ)


# ------------------------------------------------------------------------------------------------ the fields
def _hash(shape, seed):
    return _splitmix(np.arange(int(np.prod(shape)), dtype=np.uint64), seed).reshape(shape)


def _unit(h):
    """hash -> float64 in [0, 1)"""
    return (h >> np.uint64(11)).astype(np.float64) * (2.0 ** -53)


def dense(shape, seed=23):
    """The hash mapped to (-1, 1): about half of the lattice edges cross iso 0 and all 256 cases occur."""
    return (_unit(_hash(shape, seed)) * 2.0 - 1.0).astype(np.float32)


def ties(shape, seed=29):
    """Integers from {-1, 0, 1}: at iso 0 / -0 a third of the samples EQUAL iso (`<` is strict), at iso -1 nothing is below iso."""
    return (_hash(shape, seed) % np.uint64(3)).astype(np.float32) - np.float32(1.0)


DENORM_POS, DENORM_NEG = 0x00000002, 0x80000001       # 3e-45 and -1e-45 as float32: two and one denormal steps


def denormal(shape, seed=31):
    """All 3e-45, with -1e-45 at about a tenth of the samples of even i + j + k: no two of them share a lattice edge, so every crossing
    runs from a -1e-45 to a 3e-45 sample and lies a third of the edge from the negative one -- offset 2/3 from the positive sample,
    t = (0 - 2d) / (-1d - 2d).  A build that flushes float32 denormals sees no crossing, or delta == 0 and the offset 0.5."""
    i, j, k = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    neg = ((i + j + k) % 2 == 0) & (_hash(shape, seed) % np.uint64(5) == 0)
    return np.where(neg, np.uint32(DENORM_NEG), np.uint32(DENORM_POS)).astype(np.uint32).view(np.float32)


def nonfinite_plants(shape, seed=37):
    """[(i, j, k, value)]: one NaN, one +inf, one -inf and three +-3e38 pairs (one per axis: v2 - v1 overflows to inf between the two,
    so t = 0), on i-planes at least three apart, the pairs' partners next to them."""
    NX, NY, NZ = shape
    h = _splitmix(np.arange(6, dtype=np.uint64), seed)
    out = []
    for n, val in enumerate((np.nan, np.inf, -np.inf, 3e38, 3e38, 3e38)):
        i = 1 + n * (NX - 2) // 6
        j = 1 + int(h[n] % np.uint64(NY - 2))                          # off the faces of the volume: all six edges have an owner
        k = 1 + int((h[n] >> np.uint64(20)) % np.uint64(NZ - 2))
        out.append((i, j, k, val))
        if n >= 3:
            p = [i, j, k]
            axis = n - 3
            p[axis] += 1 if p[axis] + 1 < shape[axis] else -1
            out.append((p[0], p[1], p[2], -3e38))
    return out


def nonfinite(shape):
    s = dense(shape)
    for i, j, k, val in nonfinite_plants(shape):
        s[i, j, k] = val
    return s


ALL_CASES_PITCH = 6               # 216 voxels per block: the reference's scratch (0.6 vertices, 0.25 faces per voxel) holds the mesh
ALL_CASES_SHAPE = (8 * ALL_CASES_PITCH, 8 * ALL_CASES_PITCH, 4 * ALL_CASES_PITCH)


def all_cases(seed=41):
    """The 256 sign patterns of a 2 x 2 x 2 block, one per block, 8 x 8 x 4 blocks on a pitch of ALL_CASES_PITCH in an all-positive
    background; block n has its corner b (CORNERS) negative where bit b of n is set.  Magnitudes in [0.1, 1.1) from the hash.  The cell
    at the block's origin has case n; the 26 cells around it see the block's samples against the background."""
    p = ALL_CASES_PITCH
    s = (0.1 + _unit(_hash(ALL_CASES_SHAPE, seed))).astype(np.float32)
    for n in range(256):
        a, b, c = 1 + p * (n // 32), 1 + p * (n // 4 % 8), 1 + p * (n % 4)
        for bit, (di, dj, dk) in enumerate(CORNERS):
            if n >> bit & 1:
                s[a + di, b + dj, c + dk] *= np.float32(-1.0)
    return s


def far_corner(shape):
    """All 1.0 but the last sample: the one cell's triangle lies on three lattice edges that no cell owns (their origins are on the far
    faces of the volume), so the mesh has a face of three -1 and NO vertex."""
    s = np.ones(shape, np.float32)
    s[-1, -1, -1] = -1.0
    return s


def cube_cases(s, iso=0.0):
    """The case index of every cell, [NX-1, NY-1, NZ-1] (empty when an axis is 1), from the sign array."""
    neg = s < np.float32(iso)
    NX, NY, NZ = s.shape
    idx = np.zeros((max(NX - 1, 0), max(NY - 1, 0), max(NZ - 1, 0)), np.int32)
    for bit, (di, dj, dk) in enumerate(CORNERS):
        idx |= neg[di:NX - 1 + di, dj:NY - 1 + dj, dk:NZ - 1 + dk].astype(np.int32) << bit
    return idx


# ------------------------------------------------------------------------------------------------ the table
_DENSE = [
    ((1, 1, 1), "axis of 1: no cell, empty mesh"), ((1, 5, 7), "axis of 1 (NX): no cell, empty mesh"),
    ((5, 1, 7), "axis of 1 (NY): no cell, empty mesh"), ((5, 7, 1), "axis of 1 (NZ): no cell, empty mesh; 64 carry wraps a step"),
    ((2, 2, 2), "less than one group; 7 XCD ranges empty"), ((3, 3, 3), "less than one group; 7 XCD ranges empty"),
    ((4, 4, 4), "exactly one group; 7 XCD ranges empty"),
    ((9, 2, 2), "NY*NZ < 64: 16 i-planes per group, multi-wrap carry"), ((40, 3, 5), "NY*NZ < 64: multi-wrap carry; G % 4 = 2"),
    ((7, 5, 63), "row end against the group end; G % 4 = 3; tail 29"), ((7, 5, 64), "rows = groups; G % 4 = 3; no tail"),
    ((7, 5, 65), "row one longer than a group; tail 35"),
    ((3, 3, 255), "a batch of 4 groups inside one row (NZ 255)"), ((3, 3, 256), "a batch of 4 groups = one row"),
    ((3, 3, 257), "a batch of 4 groups inside one row (NZ 257)"),
    ((3, 2, 1030), "a row longer than a chunk (1024 voxels); 1 XCD range empty"),
    ((7, 31, 33), "7 chunks: one XCD range empty"), ((8, 32, 32), "8 chunks: one per XCD"),
    ((8, 32, 33), "9 chunks: per_xcd 2, three ranges empty, one range with a single chunk"),
    ((23, 89, 64), "scan length G+1 = 2048: one full scan block"), ((32, 64, 64), "G+1 = 2049: the second scan block holds only the sentinel"),
    ((33, 41, 97), "G+1 = 2052: two scan blocks"),
]
BIG_SHELL = (131, 257, 251)
SPECIAL_SHAPES = ((20, 9, 70), (40, 3, 5))
TIES_ISOS = (("iso0", 0.0), ("isom0", -0.0), ("iso1", 1.0), ("isom1", -1.0))


def _name(kind, shape, tag=None):
    return "%s_%dx%dx%d" % ((kind,) + tuple(shape)) + ("_" + tag if tag else "")


VOLUMES = {_name("dense", shape): (shape, "dense", 0.0, path) for shape, path in _DENSE}
VOLUMES[_name("shell", BIG_SHELL)] = (BIG_SHELL, "shell", 0.0, "classify grid capped: a second chunk per wave; capped emit grids; 65 scan blocks")
for _shape in SPECIAL_SHAPES:
    for _tag, _iso in TIES_ISOS:
        VOLUMES[_name("ties", _shape, _tag)] = (_shape, "ties", _iso, "samples equal to iso %r, strict <" % _iso)
    VOLUMES[_name("denormal", _shape)] = (_shape, "denormal", 0.0, "crossings between float32 denormals: offset 2/3")
    VOLUMES[_name("nonfinite", _shape)] = (_shape, "nonfinite", 0.0, "NaN, +-inf, +-3e38 samples")
VOLUMES[_name("all_cases", ALL_CASES_SHAPE)] = (ALL_CASES_SHAPE, "all_cases", 0.0, "each of the 256 cases in a block of its own")
ALL_CASES = _name("all_cases", ALL_CASES_SHAPE)
FAR_CORNER = _name("far_corner", (2, 2, 2))
VOLUMES[FAR_CORNER] = ((2, 2, 2), "far_corner", 0.0, "one face, no vertex: emit with V = 0 and F = 1")
AXIS_OF_ONE = [n for n, (shape, *_) in VOLUMES.items() if min(shape) == 1]


def volume(name):
    shape, kind, _, _ = VOLUMES[name]
    if kind == "all_cases":
        return all_cases()
    return {"dense": dense, "shell": _shell, "ties": ties, "denormal": denormal, "nonfinite": nonfinite, "far_corner": far_corner}[kind](shape)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(verts [V,3] f32, keys [V] i64, faces [F,3] i64) of the sequential oracle at STEP / ORG, canonical (vertices by lattice-edge
    key, face rows sorted), read-only.  The shell keeps the oracle's default buffers (3 vertices per voxel of 8.4 M voxels is 2 GB of
    face scratch); everything else gets buffers that cannot overflow."""
    shape, kind, iso, _ = VOLUMES[name]
    out = mco.canonical(*mco.marching_cubes(volume(name), STEP, ORG, iso, full=kind != "shell"))
    for a in out:
        a.setflags(write=False)
    return out
