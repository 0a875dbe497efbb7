"""Marching cubes (csrc/mc.hip) on every launch path, against the sequential oracle: the volumes of tests/_mc_volumes.py (each shown
by tests/test_mc_paths_cpu.py to reach the path it is for), through ext.MCGpu.mc_gpu and through the C ABI directly.

Every comparison is exact -- no tolerance appears in this file.  V and F equal the oracle's, the faces are equal after the row sort,
the vertices are equal bit for bit (compared as uint32, so that -0.0 and 0.0 differ).  The one exception: where the oracle's
coordinate is NaN (only in the `nonfinite` volumes, at most 5 % of their coordinates -- tests/test_mc_paths_cpu.py holds the cap)
the kernel's must be NaN too, with any sign and payload; infinities compare by bits like everything else.  Every volume is run
twice and must repeat bit for bit; before each run a buffer of the workspace's size filled with 0xFF is handed back to the caching
allocator, so that the `torch.empty` workspace holds foreign bytes.

Through the C ABI (sr_mc_count / sr_mc_emit) a handful of the small volumes and (32,64,64) run with the workspace exactly
sr_mc_workspace_bytes long, 8 bytes past a 256-byte boundary, inside a buffer of 0xFF, and verts / faces / counts between sentinel
margins; then on the used workspace of the larger volume and on a non-default stream; and the three entry points refuse bad arguments
without writing a byte.

Run on an MI355X (the table is in profiles/mc_paths.md): every volume below equal to the oracle, every guard byte intact, every volume
repeating bit for bit.  V and F are the oracle's at STEP / ORG.

  shape          kind        iso   V       F       reaches
  (1,1,1)        dense       0.0   0       0       axis of 1: no cell, empty mesh
  (1,5,7)        dense       0.0   0       0       axis of 1 (NX): no cell, empty mesh
  (5,1,7)        dense       0.0   0       0       axis of 1 (NY): no cell, empty mesh
  (5,7,1)        dense       0.0   0       0       axis of 1 (NZ): no cell, empty mesh; 64 carry wraps a step
  (2,2,2)        dense       0.0   2       4       less than one group; 7 XCD ranges empty
  (3,3,3)        dense       0.0   13      29      less than one group; 7 XCD ranges empty
  (4,4,4)        dense       0.0   35      84      exactly one group; 7 XCD ranges empty
  (9,2,2)        dense       0.0   15      33      NY*NZ < 64: 16 i-planes per group, multi-wrap carry
  (40,3,5)       dense       0.0   471     1014    NY*NZ < 64: multi-wrap carry; G % 4 = 2
  (7,5,63)       dense       0.0   2246    4816    row end against the group end; G % 4 = 3; tail 29
  (7,5,64)       dense       0.0   2278    4831    rows = groups; G % 4 = 3; no tail
  (7,5,65)       dense       0.0   2292    4903    row one longer than a group; tail 35
  (3,3,255)      dense       0.0   1548    3192    a batch of 4 groups inside one row (NZ 255)
  (3,3,256)      dense       0.0   1498    3176    a batch of 4 groups = one row
  (3,3,257)      dense       0.0   1531    3202    a batch of 4 groups inside one row (NZ 257)
  (3,2,1030)     dense       0.0   3052    6606    a row longer than a chunk (1024 voxels); 1 XCD range empty
  (7,31,33)      dense       0.0   8652    18446   7 chunks: one XCD range empty
  (8,32,32)      dense       0.0   10068   21450   8 chunks: one per XCD
  (8,32,33)      dense       0.0   10446   22243   9 chunks: per_xcd 2, three ranges empty, one range with a single chunk
  (23,89,64)     dense       0.0   182927  390915  scan length G+1 = 2048: one full scan block
  (32,64,64)     dense       0.0   184375  393634  G+1 = 2049: the second scan block holds only the sentinel
  (33,41,97)     dense       0.0   183979  393097  G+1 = 2052: two scan blocks
  (131,257,251)  shell       0.0   98202   196308  classify grid capped: a second chunk per wave; capped emit grids; 65 scan blocks
  (20,9,70)      ties        0.0   14070   26572   a third of the samples equal iso, `<` is strict
  (20,9,70)      ties        -0.0  14070   26572   the same mesh as iso 0.0
  (20,9,70)      ties        1.0   13834   30677   a third of the samples equal iso
  (20,9,70)      ties        -1.0  0       0       nothing below iso: empty mesh
  (20,9,70)      denormal    0.0   6269    8386    crossings between float32 denormals: offset 2/3
  (20,9,70)      nonfinite   0.0   15730   33713   NaN, +-inf, +-3e38 samples (0.025 % of the coordinates NaN)
  (40,3,5)       ties        0.0   455     882     as above, several i-planes per group
  (40,3,5)       ties        -0.0  455     882
  (40,3,5)       ties        1.0   390     880
  (40,3,5)       ties        -1.0  0       0
  (40,3,5)       denormal    0.0   167     224
  (40,3,5)       nonfinite   0.0   468     1008    (1.9 % of the coordinates NaN)
  (48,48,24)     all_cases   0.0   4608    7796    each of the 256 cases in a block of its own
  (2,2,2)        far_corner  0.0   0       1       one face, no vertex: emit with V = 0 and F = 1

What the first run found: a vertex whose offset t is NaN (a NaN sample, or inf - inf next to an infinite one) has THREE NaN coordinates
in the reference -- it multiplies t by the edge direction on every axis, and 0 * NaN is NaN -- where mc_vertex_kernel wrote one
(nonfinite (20,9,70) and (40,3,5)).  Found by reading while the tests were written, and pinned here: mc_gpu handed sr_mc_emit the null
address of an empty vertex tensor on the far_corner volume, whose one face has no vertex, and sr_mc_emit did not refuse a workspace
address that is no multiple of 8.  All three are fixed.
"""
import numpy as np
import pytest
import torch

import _mc_volumes as mv
from selfreconcode_amd import _lib
from selfreconcode_amd.ext import MCGpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 64                       # sentinel elements on either side of verts, faces and counts
GUARD = 512                       # 0xFF bytes on either side of the workspace
V_SENT, F_SENT, C_SENT = -(2.0 ** 100), -0x7777777777777777, 0x5A5A5A5A


def _sorted_rows(f):
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


def _assert_is_the_oracles(name, v, f):
    """v [V,3] float32, f [F,3] int64 as the kernels wrote them (numpy) against mv.reference(name)."""
    kind = mv.VOLUMES[name][1]
    vo, _, fo = mv.reference(name)
    assert v.dtype == np.float32 and f.dtype == np.int64
    assert v.shape == vo.shape and f.shape == fo.shape, (v.shape, vo.shape, f.shape, fo.shape)
    assert np.array_equal(_sorted_rows(f), fo)
    same = v.view(np.uint32) == vo.view(np.uint32)                      # the HIP output is already in lattice-edge-key order
    nan = np.isnan(vo)
    if kind == "nonfinite":
        assert nan.any() and np.isnan(v[nan]).all()
        same |= nan
    else:
        assert not nan.any()
    assert same.all(), (int((~same).sum()), v[~same][:4], vo[~same][:4])


def _poison_the_allocator(shape):
    n = int(_lib.raw("sr_mc_workspace_bytes")(*shape)) + 256
    junk = torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)
    del junk


@pytest.mark.parametrize("name", list(mv.VOLUMES))
def test_mc_gpu_equals_the_oracle(name):
    shape, kind, iso, path = mv.VOLUMES[name]
    s = torch.from_numpy(mv.volume(name)).to(DEV)
    _poison_the_allocator(shape)
    verts, faces = MCGpu.mc_gpu(s, *mv.STEP, *mv.ORG, iso)
    _poison_the_allocator(shape)
    verts2, faces2 = MCGpu.mc_gpu(s, *mv.STEP, *mv.ORG, iso)
    print("%-28s iso %-5r V %-7d F %-7d %s" % (name, iso, len(verts), len(faces), path))
    _assert_is_the_oracles(name, verts.cpu().numpy(), faces.cpu().numpy())
    assert torch.equal(verts.view(torch.int32), verts2.view(torch.int32)) and torch.equal(faces, faces2)
    if kind != "nonfinite":
        assert torch.equal(verts, verts2)


# ------------------------------------------------------------------------------------------------ through the C ABI
class _Arena:
    """A byte buffer filled with 0xFF whose `ws` region starts 8 bytes past a 256-byte boundary, GUARD bytes or more from either end."""

    def __init__(self, nbytes):
        self.buf = torch.full((nbytes + 2 * GUARD + 512,), 0xFF, dtype=torch.uint8, device=DEV)
        self.off = GUARD + (8 - (self.buf.data_ptr() + GUARD)) % 256
        assert (self.buf.data_ptr() + self.off) % 256 == 8 and self.off + nbytes + GUARD <= self.buf.numel()


class _Guarded:
    """n elements between two margins of MARGIN sentinel elements, all filled with the sentinel."""

    def __init__(self, n, dtype, sent):
        self.n, self.sent = n, sent
        self.buf = torch.full((n + 2 * MARGIN,), sent, dtype=dtype, device=DEV)
        self.ptr = self.buf.data_ptr() + MARGIN * self.buf.element_size()

    def inner(self):
        return self.buf[MARGIN:MARGIN + self.n]

    def margins_intact(self):
        return bool((self.buf[:MARGIN] == self.sent).all()) and bool((self.buf[MARGIN + self.n:] == self.sent).all())


def _abi_run(name, arena=None):
    """sr_mc_count + sr_mc_emit on torch's current stream, the workspace exactly sr_mc_workspace_bytes long at arena.off; checks counts,
    mesh and every guard byte.  -> the arena (used)."""
    shape, kind, iso, _ = mv.VOLUMES[name]
    vo, _, fo = mv.reference(name)
    s = torch.from_numpy(mv.volume(name)).to(DEV)
    nbytes = int(_lib.raw("sr_mc_workspace_bytes")(*shape))
    assert nbytes > 0
    arena = arena or _Arena(nbytes)
    assert arena.off + nbytes + GUARD <= arena.buf.numel()
    before = arena.buf.clone()
    ws = arena.buf.data_ptr() + arena.off
    counts = _Guarded(2, torch.int32, C_SENT)
    _lib.launch("sr_mc_count", s, s, *shape, float(iso), ws, counts.ptr)
    V, F = counts.inner().tolist()
    assert (V, F) == (len(vo), len(fo)) and counts.margins_intact()
    verts, faces = _Guarded(3 * V, torch.float32, V_SENT), _Guarded(3 * F, torch.int64, F_SENT)
    _lib.launch("sr_mc_emit", s, s, *shape, float(iso), ws, *mv.STEP, *mv.ORG, verts.ptr, faces.ptr)
    torch.cuda.current_stream().synchronize()
    assert verts.margins_intact() and faces.margins_intact() and counts.margins_intact()
    after = arena.buf
    assert torch.equal(after[:arena.off], before[:arena.off]) and torch.equal(after[arena.off + nbytes:], before[arena.off + nbytes:])
    _assert_is_the_oracles(name, verts.inner().view(V, 3).cpu().numpy(), faces.inner().view(F, 3).cpu().numpy())
    return arena


ABI_SMALL = ["dense_5x7x1", "dense_2x2x2", mv.FAR_CORNER, "dense_9x2x2", "dense_7x5x65", "dense_3x3x256", "dense_8x32x33", "ties_40x3x5_iso0"]
ABI_LARGE = "dense_32x64x64"


@pytest.mark.parametrize("name", ABI_SMALL + [ABI_LARGE])
def test_c_abi_writes_inside_its_buffers_only(name):
    """A workspace of exactly sr_mc_workspace_bytes, 8-byte but not 256-byte aligned, 0xFF inside and around it; verts, faces and counts
    between sentinel margins."""
    _abi_run(name)


def test_c_abi_on_a_used_workspace_and_on_another_stream():
    """The workspace of the small volumes is the head of the one (32,64,64) has just used: stale planes, stale scanned offsets, a stale
    off[G] sentinel further in -- and what lies past the small volume's bytes stays as the large run left it.  Then the same on a
    non-default stream."""
    arena = _abi_run(ABI_LARGE)
    assert not bool((arena.buf[arena.off:arena.off + 4096] == 0xFF).all())          # it IS used
    for name in ABI_SMALL:
        _abi_run(name, arena)
    _abi_run(ABI_LARGE, arena)                                                      # ... and back, over the small volumes' bytes
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert _lib.stream_of(arena.buf) == side.cuda_stream != 0
        for name in ("dense_7x5x65", ABI_LARGE, "dense_8x32x33"):
            _abi_run(name, arena)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)


def test_refusals_write_nothing():
    """SR_EINVAL, and not a byte written, for a non-positive axis, a null volume / workspace / counts pointer and a workspace address
    that is not a multiple of 8 -- at each of the three entry points that takes the argument."""
    size, count, emit = _lib.raw("sr_mc_workspace_bytes"), _lib.raw("sr_mc_count"), _lib.raw("sr_mc_emit")
    shape = (4, 4, 4)
    s = torch.from_numpy(mv.dense(shape)).to(DEV)
    arena = _Arena(int(size(*shape)))
    ws = arena.buf.data_ptr() + arena.off
    counts = _Guarded(2, torch.int32, C_SENT)
    verts, faces = _Guarded(3 * 64, torch.float32, V_SENT), _Guarded(3 * 128, torch.int64, F_SENT)
    step_org = tuple(mv.STEP) + tuple(mv.ORG)
    bad_shapes = [(0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (4, -4, 4), (4, 4, -2 ** 31)]
    calls = []
    for bad in bad_shapes:
        assert size(*bad) == _lib.SR_EINVAL
        calls.append((count, (s.data_ptr(),) + bad + (0.0, ws, counts.ptr, 0)))
        calls.append((emit, (s.data_ptr(),) + bad + (0.0, ws) + step_org + (verts.ptr, faces.ptr, 0)))
    for sdf_p, ws_p, counts_p in ((0, ws, counts.ptr), (s.data_ptr(), 0, counts.ptr), (s.data_ptr(), ws, 0), (s.data_ptr(), ws + 4, counts.ptr),
                                  (s.data_ptr(), ws + 1, counts.ptr), (s.data_ptr(), ws - 2, counts.ptr)):
        calls.append((count, (sdf_p,) + shape + (0.0, ws_p, counts_p, 0)))
        if counts_p:
            calls.append((emit, (sdf_p,) + shape + (0.0, ws_p) + step_org + (verts.ptr, faces.ptr, 0)))
    assert len(calls) == 12 + 6 + 5
    with torch.cuda.device(DEV):
        for fn, args in calls:
            assert fn(*args) == _lib.SR_EINVAL, args
    torch.cuda.synchronize()
    assert bool((arena.buf == 0xFF).all())
    for g in (counts, verts, faces):
        assert g.margins_intact() and bool((g.inner() == g.sent).all())
    # ... and the same buffers are accepted once the arguments are right
    assert size(*shape) > 0
    _abi_run("dense_4x4x4")
