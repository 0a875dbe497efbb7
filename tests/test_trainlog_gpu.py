"""The device-side training log: the row kernel (ops.log_row / sr_log_row) at its smallest shapes, inside a sentinel-filled buffer whose
neighbours are checked, and trainlog.TrainLog beyond the capacity of its ring."""
import ctypes

import numpy as np
import pytest
import torch

from selfreconcode_amd import _lib, ops
from selfreconcode_amd.trainlog import TrainLog

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL, GUARD = -7.0, 64


def _guarded(rows, ld):
    """A [rows, ld] float32 ring filled with a sentinel, GUARD floats into a buffer that goes on for GUARD floats behind it."""
    buf = torch.full((GUARD + rows * ld + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + rows * ld].view(rows, ld)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _bits(t):
    return (t.detach().cpu().contiguous() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))).view(torch.int32)


def _f32(x):
    return torch.tensor(x, dtype=torch.float32, device=DEV)


def _i64(x):
    return torch.tensor(x, dtype=torch.int64, device=DEV)


def test_smallest_call():
    buf, ring = _guarded(1, 1)
    src = _f32(3.25)
    ops.log_row(ring, 0, [src])
    assert ring.tolist() == [[3.25]] and _guards_intact(buf)
    ops.log_row(ring, 5, [None])                                    # any row number lands in the only slot; an empty slot is NaN
    assert bool(torch.isnan(ring).all()) and _guards_intact(buf)


def test_all_kinds_in_one_row_of_32():
    n = ops.LOG_MAX_SLOTS
    assert n == 32
    buf, ring = _guarded(2, n)
    f, i = _f32([0.5 * k - 3. for k in range(n)]), _i64([k * k - 40 for k in range(n)])
    values = [(None, f[k], i[k], 0.1 * k)[k % 4] for k in range(n)]
    ops.log_row(ring, 1, values)
    want = np.array([(np.nan, np.float32(0.5 * k - 3.), np.float32(k * k - 40), np.float32(0.1 * k))[k % 4] for k in range(n)], np.float32)
    assert torch.equal(_bits(ring[1]), _bits(want))
    assert bool((ring[0] == SENTINEL).all()) and _guards_intact(buf)       # the other row is not this call's


def test_nan_tail():
    buf, ring = _guarded(2, 8)
    ops.log_row(ring, 0, [1., 2., 3., 4., 5.])
    assert ring[0, :5].tolist() == [1., 2., 3., 4., 5.] and bool(torch.isnan(ring[0, 5:]).all())
    assert bool((ring[1] == SENTINEL).all()) and _guards_intact(buf)


def test_wrap():
    buf, ring = _guarded(3, 2)
    src = [_f32(float(10 + r)) for r in range(8)]
    for r in range(8):
        ops.log_row(ring, r, [src[r], r])
    assert ring.tolist() == [[16., 6.], [17., 7.], [15., 5.]] and _guards_intact(buf)       # rows 6, 7, 5 in slots 0, 1, 2


def test_f32_sources_are_copied_bit_for_bit():
    patterns = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc12345, 0xffa00001, 0x00000001, 0x807fffff], np.uint32)     # -0, +-inf, NaNs with
    src = torch.from_numpy(patterns.view(np.int32)).to(DEV).view(torch.float32)                                           # payloads, denormals
    buf, ring = _guarded(1, len(patterns))
    ops.log_row(ring, 0, [src[k] for k in range(len(patterns))])
    assert torch.equal(_bits(ring[0]), torch.from_numpy(patterns.view(np.int32))) and _guards_intact(buf)


def test_i64_sources_are_converted_as_float32():
    ints = [2 ** 24 + 1, -3, 0, 2 ** 24 + 3, -(2 ** 40) - 1, 2 ** 62 + 2 ** 38]
    src = _i64(ints)
    buf, ring = _guarded(1, len(ints))
    ops.log_row(ring, 0, [src[k] for k in range(len(ints))])
    want = np.array([np.float32(v) for v in ints], np.float32)
    assert want[0] == 2 ** 24 and want[3] == 2 ** 24 + 4                       # ties to even, both ways
    assert torch.equal(_bits(ring[0]), _bits(want)) and _guards_intact(buf)


def test_sources_are_read_in_stream_order():
    """The pointer is captured at issue, the value is what the stream left there: a source written on the launch stream immediately
    before the call is seen, and one written after it is not."""
    from selfreconcode_amd import mlp_engine
    side = mlp_engine._tn_stream(torch.device(DEV))                 # (an existing stream that is not the default one)
    buf, ring = _guarded(2, 1)
    src = _f32(1.)
    A = torch.randn(2048, 2048, device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(4):
            A = A @ A * 1e-3                                        # work in front of the write, so that issue time and run time differ
        src.copy_(A.sum().isnan().float() + 41.)                    # 41 or 42, decided on the device
        src.add_(1.)
        ops.log_row(ring, 0, [src])
        src.fill_(7.)
        ops.log_row(ring, 1, [src])
    torch.cuda.current_stream().wait_stream(side)
    assert ring[0, 0].item() in (42., 43.) and ring[1, 0].item() == 7. and _guards_intact(buf)


def test_invalid_arguments_are_refused_and_write_nothing():
    buf, ring = _guarded(4, 8)
    f, i = _f32([1., 2., 3.]), _i64([1, 2])
    EINVAL = pytest.raises(_lib.SrError, match="SR_EINVAL")

    def raw(slots, n=1, ring_t=ring, rows=4, ld=8, row=0):
        _lib.launch("sr_log_row", ring, ctypes.byref(slots) if slots is not None else None, n, ring_t, rows, ld, row)

    def slots(kind, src=0, k=0):
        s = _lib.SrLogSlots()
        s.kind[k], s.src[k] = kind, src
        return s
    good = slots(_lib.SR_LOG_F32, f.data_ptr())
    cases = [lambda: raw(good, n=0), lambda: raw(good, n=-1), lambda: raw(good, n=33), lambda: raw(good, n=4, ld=3), lambda: raw(good, rows=0),
             lambda: raw(good, rows=-2), lambda: raw(good, row=-1), lambda: raw(slots(4)), lambda: raw(slots(255)),
             lambda: raw(slots(_lib.SR_LOG_F32, 0)), lambda: raw(slots(_lib.SR_LOG_I64, 0)),
             lambda: raw(slots(_lib.SR_LOG_F32, f.data_ptr() + 2)), lambda: raw(slots(_lib.SR_LOG_I64, i.data_ptr() + 4)),
             lambda: raw(slots(_lib.SR_LOG_F32, 0, k=1), n=2),        # a bad slot behind a good (empty) one
             lambda: raw(good, ring_t=None), lambda: raw(None)]
    for case in cases:
        with EINVAL:
            case()
    raw(slots(_lib.SR_LOG_I64, i.data_ptr() + 8), row=2)           # the aligned neighbours of the refused pointers are fine
    raw(slots(_lib.SR_LOG_F32, f.data_ptr() + 4), row=3)
    with pytest.raises(RuntimeError, match="non-GPU"):
        ops.log_row(ring.cpu(), 0, [1.])
    with pytest.raises(RuntimeError, match="non-GPU"):
        ops.log_row(ring, 0, [torch.tensor(1.)])
    for bad in (lambda: ops.log_row(ring, 0, [0.] * 33), lambda: ops.log_row(ring, 0, [f]), lambda: ops.log_row(ring, 0, [f[0].double()]),
                lambda: ops.log_row(ring[:, :4], 0, [1.])):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert bool((ring[:2] == SENTINEL).all()) and _guards_intact(buf)                       # no refused call wrote anything
    assert ring[2, 0].item() == 2. and ring[3, 0].item() == 2.
    assert ctypes.sizeof(_lib.SrLogSlots) == 32 * 8 + 32 * 4 + 32


def test_trainlog_beyond_the_capacity_of_its_ring():
    """40 appends into 8 ring rows, a drain every third: every row arrives, in order, exactly once."""
    log = TrainLog(('step', 'device_f32', 'device_i64', 'absent'), ring_rows=8, device=DEV)
    got = []
    for k in range(40):
        log.append({'step': k, 'device_f32': _f32(0.5 * k), 'device_i64': _i64(3 * k)})
        if k % 3 == 2:
            got += list(log.drain())
    got += list(log.drain(block=True))
    print(f"TrainLog: 40 rows through 8 ring rows, drained every 3 appends: {log.stalls} stalls")
    got = np.stack(got)
    assert got.shape == (40, 4) and got[:, 0].tolist() == list(range(40))
    assert got[:, 1].tolist() == [0.5 * k for k in range(40)] and got[:, 2].tolist() == [3. * k for k in range(40)] and np.isnan(got[:, 3]).all()
    assert log.drain(block=True).shape == (0, 4) and log.issued == 40 and not log._alive and 0 <= log.stalls <= 40
    # without any drain the ring overflows every ring_rows appends: the log waits (and counts it) instead of losing rows
    log = TrainLog(('step',), ring_rows=4, device=DEV)
    for k in range(10):
        log.append({'step': k})
    assert log.stalls == 2 and log.drain(block=True)[:, 0].tolist() == list(range(10))
    with pytest.raises(KeyError):
        log.append({'nope': 1})
    with pytest.raises(RuntimeError):
        TrainLog(('a',), device="cpu")
