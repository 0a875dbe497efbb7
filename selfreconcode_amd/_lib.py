"""ctypes binding of libselfrecon_hip.so -- the only door from Python to the HIP kernels.

There is NO fallback: if the shared library is missing or lacks a symbol the import of any
operator module fails loudly (a product path that silently ran on CPU/eager PyTorch would
void every parity and performance claim).
"""
import ctypes
import os
import torch

from . import _abi
from .build import LIB

# include/selfrecon_hip.h is the one statement of the boundary: its #defines, argument structs and prototypes are read from it here,
# once per process, and nothing of them is restated in Python (tests/test_abi.py checks the reading against gcc).
try:
    _DEFINES, _STRUCTS, _PROTOTYPES = _abi.load()
except (OSError, _abi.AbiError) as e:
    raise ImportError(f"{_abi.HEADER}: {e}") from e
globals().update(_DEFINES)                                        # SR_TN_GROUP_MAX = 12, ...: every integer #define
globals().update({c.__name__: c for c in _STRUCTS.values()})      # SrTensor5 (sr_tensor5), SrGemmArgs (sr_gemm_args), ...


class SrError(RuntimeError):
    pass


_CODES = {_DEFINES["SR_EINVAL"]: "SR_EINVAL (bad argument)", _DEFINES["SR_ELAUNCH"]: "SR_ELAUNCH (kernel launch failed)",
          _DEFINES["SR_ENOSPC"]: "SR_ENOSPC (workspace too small)"}

if "SELFRECON_HIP_LIB" in os.environ:
    LIB = os.environ["SELFRECON_HIP_LIB"]         # tuning hook: point at an experimental build of the same ABI
else:
    from .build import is_stale, build_lib
    if is_stale():                                # sources changed since the .so was linked (or no .so yet): kernels and the ctypes
        try:                                      # structs below must come from the same tree -- rebuild (one process builds under an
            build_lib(verbose=False)              # flock, the others wait; atomic publish) or fail loudly
        except RuntimeError as e:
            raise ImportError(str(e)) from e
if not os.path.isfile(LIB):
    raise ImportError(f"{LIB} not found: run `python -m selfreconcode_amd.build` (hipcc --offload-arch=gfx950). "
                      "There is no CPU fallback for the HIP hot path.")
_lib = ctypes.CDLL(LIB)

_INFO = ("sr_abi_version", "sr_build_arch", "sr_build_digest")   # (called through the functions below, not through call())
SIGNATURES = {name: argtypes for name, (_, argtypes) in _PROTOTYPES.items() if name not in _INFO}     # name -> argtypes

_fn = {}
for _name, _args in SIGNATURES.items():
    try:
        _f = getattr(_lib, _name)
    except AttributeError as e:  # pragma: no cover
        raise ImportError(f"{LIB} does not export {_name}; rebuild it") from e
    _f.argtypes = _args
    _f.restype = _PROTOTYPES[_name][0]
    _fn[_name] = _f
for _name in _INFO:
    getattr(_lib, _name).restype, getattr(_lib, _name).argtypes = _PROTOTYPES[_name]


def bind_header(path):
    """(defines, structs) of an extension header next to the kernels (csrc/*_abi.h, read by _abi.parse like the main header): its
    prototypes get their argtypes / restype on the loaded library and join `_fn`, so call, launch, raw and workspace serve them.
    SIGNATURES and this module's SR_* attributes stay the main header's.  ImportError for a header that does not parse, a name the
    main header already declares, or a symbol the library lacks -- there is no fallback."""
    try:
        with open(path) as fh:
            defines, structs, prototypes = _abi.parse(fh.read())
    except (OSError, _abi.AbiError) as e:
        raise ImportError(f"{path}: {e}") from e
    fresh = {}
    for name, (restype, argtypes) in prototypes.items():
        if name in _PROTOTYPES:
            raise ImportError(f"{path}: {name} is declared by {_abi.HEADER}")
        try:
            f = getattr(_lib, name)
        except AttributeError as e:
            raise ImportError(f"{LIB} does not export {name}; rebuild it") from e
        f.argtypes, f.restype = argtypes, restype
        fresh[name] = f
    _fn.update(fresh)
    return defines, structs


def abi_version():
    return _lib.sr_abi_version()


def build_arch():
    return _lib.sr_build_arch().decode()


def build_digest():
    return _lib.sr_build_digest().decode()


def raw(name):
    return _fn[name]


def call(name, *args):
    rc = _fn[name](*args)
    if rc != 0:
        raise SrError(f"{name} failed: {_CODES.get(rc, rc)}")


def ptr(t):
    return 0 if t is None else t.data_ptr()


def device_args(on, args):
    """The flat C arguments of a launch anchored on tensor `on`: a tensor goes as its address, None as a null pointer, anything else
    (ints, floats, ctypes arrays, structs, byref objects) as it is.  A tensor on another device than `on` is refused here -- behind
    whatever require_gpu() the operator did on its own arguments -- instead of becoming a GPU fault."""
    dev, out = on.device, []
    for a in args:
        if isinstance(a, torch.Tensor):
            if a.device != dev:
                raise RuntimeError(f"selfreconcode_amd: HIP operator called with a tensor on {a.device} in a launch on {dev} "
                                   "(there is deliberately no CPU fallback)")
            out.append(a.data_ptr())
        elif a is None:
            out.append(0)
        else:
            out.append(a)
    return out


def launch(name, on, *args):
    """call(name, *args, stream): THE way to run a stream-taking entry point with flat arguments (see device_args) -- on the device
    of tensor `on` and on torch's current stream there, which every kernel entry point takes last."""
    flat = device_args(on, args)
    with on_device(on.device):
        call(name, *flat, stream_of(on))


def workspace(name, *args, device, dtype=torch.uint8):
    """Scratch for a kernel whose size function is `name(*args)` (in elements of `dtype`; negative: an error code -> SrError): at
    least one element, 256-byte aligned.  The result is a view into a slightly larger allocation and is itself what to pass and save."""
    n = _fn[name](*args)
    if n < 0:
        raise SrError(f"{name} failed: {_CODES.get(n, n)}")
    n, per = max(int(n), 1), 256 // dtype.itemsize
    buf = torch.empty((n + per,), dtype=dtype, device=device)
    off = (-buf.data_ptr()) % 256 // dtype.itemsize
    return buf[off:off + n]


def f32c(t):
    """t.detach().contiguous().float() without the conversions that would be no-ops (each is a dispatcher round trip)."""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def i64c(t):
    t = t.detach()
    if t.dtype != torch.int64:
        t = t.long()
    return t if t.is_contiguous() else t.contiguous()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_of(t):
    """hipStream_t of torch's CURRENT stream on the tensor's device (kernels are stream-ordered
    with the surrounding torch ops; the reference's FastMinv/MCGpu used the legacy default stream).
    (The raw-handle query is ~0.3 us; `torch.cuda.current_stream(dev).cuda_stream` builds a Stream object per call, ~5 us -- 120 of them per
    iteration, which shows at one frame per rank where the step is bound by the host.)"""
    if _raw_stream is not None and t.device.index is not None:
        return _raw_stream(t.device.index)
    return torch.cuda.current_stream(t.device).cuda_stream


class _NoContext:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_CONTEXT = _NoContext()


def on_device(dev):
    """`with on_device(t.device):` = `with torch.cuda.device(t.device):` that costs nothing when that device is already current (the
    one-process-per-GPU case: ~180 context entries per iteration at ~4 us each otherwise)."""
    if dev.index is not None and dev.index == torch.cuda.current_device():
        return _NO_CONTEXT
    return torch.cuda.device(dev)


def desc5(t):
    d = SrTensor5()
    for i in range(5):
        d.size[i] = t.shape[i]
        d.stride[i] = t.stride(i)
    return d


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("selfreconcode_amd: HIP operator called with a non-GPU tensor "
                               "(there is deliberately no CPU fallback)")
