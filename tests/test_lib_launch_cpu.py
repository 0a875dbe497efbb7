"""CPU-side checks of the operator layer in _lib: what launch() hands to a kernel entry point, and the workspace helper.  Nothing here
runs a kernel (the size functions are plain host code of the cross-compiled library)."""
import ctypes

import pytest
import torch

from selfreconcode_amd import _lib


def test_device_args_converts_tensors_and_passes_everything_else_through():
    on = torch.zeros(3)
    t = torch.arange(4.)
    arr = (ctypes.c_float * 3)(1., 2., 3.)
    ref = ctypes.byref(_lib.SrLbsArgs())
    desc = _lib.desc5(torch.zeros(1, 1, 1, 1, 1))
    out = _lib.device_args(on, (t, None, 7, 0.5, arr, ref, desc, t[1:]))
    assert out[0] == t.data_ptr() and type(out[0]) is int
    assert out[1] == 0 and type(out[1]) is int
    assert out[2] == 7 and out[3] == 0.5
    assert out[4] is arr and out[5] is ref and out[6] is desc
    assert out[7] == t.data_ptr() + 4                       # a view goes as ITS address
    assert _lib.device_args(on, ()) == []


def test_device_args_refuses_a_tensor_on_another_device():
    on = torch.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.device_args(on, (on, 1, torch.empty(2, device="meta")))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.device_args(torch.empty(2, device="meta"), (on,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # launch() converts before it touches any device state
        _lib.launch("sr_svd3x3", on, torch.empty(9, device="meta"), 1, on, on, on)


def test_workspace_raises_on_an_error_code():
    with pytest.raises(_lib.SrError, match="sr_texture_fill_workspace_bytes.*SR_EINVAL"):
        _lib.workspace("sr_texture_fill_workspace_bytes", -1, device="cpu")


@pytest.mark.parametrize("name,args,dtype", [("sr_texture_fill_workspace_bytes", (1,), torch.uint8), ("sr_texture_fill_workspace_bytes", (5,), torch.uint8),
                                             ("sr_smpl_regress_workspace_floats", (1, 1, 1), torch.float32)])
def test_workspace_is_aligned_and_large_enough(name, args, dtype):
    need = _lib.raw(name)(*args)
    assert need >= 0
    ws = _lib.workspace(name, *args, device="cpu", dtype=dtype)
    assert ws.dtype == dtype and ws.dim() == 1 and ws.is_contiguous()
    assert ws.data_ptr() % 256 == 0
    assert ws.numel() >= 1 and ws.numel() >= need
    ws.fill_(1)                                             # the whole view is writable memory of its allocation
    assert ws.untyped_storage().nbytes() >= ws.storage_offset() * ws.element_size() + ws.numel() * ws.element_size()


def test_workspace_default_dtype_is_bytes():
    assert _lib.workspace("sr_texture_fill_workspace_bytes", 5, device="cpu").dtype == torch.uint8


def test_normalisers_skip_no_op_conversions_and_give_the_chain_results():
    x = torch.arange(12.).view(3, 4).requires_grad_(True)
    y = _lib.f32c(x)
    assert y.data_ptr() == x.data_ptr() and not y.requires_grad and y.dtype == torch.float32
    z = _lib.f32c(x.double().t())
    assert z.dtype == torch.float32 and z.is_contiguous() and torch.equal(z, x.detach().t().contiguous().float())
    i = torch.arange(6, dtype=torch.int32).view(2, 3)
    assert torch.equal(_lib.i64c(i.t()), i.t().long().contiguous()) and _lib.i64c(i.t()).is_contiguous()
    j = torch.arange(6)
    assert _lib.i64c(j).data_ptr() == j.data_ptr()
