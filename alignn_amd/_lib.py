"""ctypes binding of libalignn_hip.so.  The C ABI is declared once, in include/alignn_hip.h: the prototypes and argument
structs used here are read from that header (_abi.py), not restated.  The batched workflows declare theirs in headers of
their own; ``bind`` types those of one such header on the same library.

The product path has NO fallback: if the shared library is missing or a GPU call fails, an
exception is raised.  PyTorch appears here only as the owner of device memory and streams.
"""

from __future__ import annotations

import ctypes as C
import os

import torch

from ._abi import SIGNATURES, STRUCTS  # name -> (restype, argtypes) of every entry point; the argument structs by their C names

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libalignn_hip.so")
LIB_PATH = os.environ.get("ALIGNN_AMD_LIB_PATH", LIB_PATH)  # (A/B runs of differently compiled libraries: tools/gpu/*.sh)

# argument blocks of the composite entry points, of alignn_fire_step and of alignn_md_step (the header describes every field).
# Filled by name, a field left out is NULL / 0; passed with ``ctypes.byref``.  load() checks the sizes against the library's.
EgcFwdArgs, EgcBwdArgs, EgcWgradArgs = (STRUCTS[f"alignn_egc_{k}_args"] for k in ("fwd", "bwd", "wgrad"))
FireArgs, MdArgs = STRUCTS["alignn_fire_args"], STRUCTS["alignn_md_args"]


_lib = None
_bound = {}  # header path -> the library object its entry points were last typed on


def _type(lib, signatures):
    for name, (res, args) in signatures.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args


def _check_size(name, size, block):
    if size != C.sizeof(block):  # (a library built from another header than the one read here)
        raise RuntimeError(f"argument block {name}: library says {size} bytes, the header gives {C.sizeof(block)}")


def load() -> C.CDLL:
    """Load the HIP library (once).  Raises if it has not been built - there is no CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -m alignn_amd.build` "
                "(hipcc --offload-arch=gfx950); alignn_amd has no CPU/eager fallback."
            )
        lib = C.CDLL(LIB_PATH)
        _type(lib, SIGNATURES)
        sizes = [lib.alignn_egc_args_sizeof(k) for k in range(3)] + [lib.alignn_fire_args_sizeof(), lib.alignn_md_args_sizeof()]
        for size, block in zip(sizes, (EgcFwdArgs, EgcBwdArgs, EgcWgradArgs, FireArgs, MdArgs)):
            _check_size(block.__name__, size, block)
        _lib = lib
    return _lib


def bind(header, lib=None):
    """The library of ``load()`` (or ``lib``) with the entry points of ``header`` (an ``_abi.Header``) typed, once per library
    object; every argument block ``S`` of the header is checked against the library's ``S_size()``."""
    lib = load() if lib is None else lib
    if _bound.get(header.path) is not lib:
        _type(lib, header.signatures)
        for name, block in header.structs.items():
            _check_size(name, getattr(lib, name + "_size")(), block)
        _bound[header.path] = lib
    return lib


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """Raw handle of torch's current HIP stream (what every launch goes to).  ``torch.cuda.current_stream()`` builds a
    Python Stream object per call (~8 us, ~650 calls per training step); the raw getter is a plain C call."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def device_guard(t):
    """Every launch goes to the CURRENT device's current stream (``stream()``): make the tensors' device current for
    the duration of a module forward when it is not already (a model living on a non-current GPU).  The autograd
    engine replays backward nodes under the device of their forward, so guarding the forward covers both."""
    if t.is_cuda and t.device.index != torch.cuda.current_device():
        return torch.cuda.device(t.device)
    return _NO_GUARD


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"libalignn_hip: {what} failed with hipError {rc}")


def require_f32(*tensors):
    for t in tensors:
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_cuda:
            raise TypeError(
                f"alignn_amd kernels take float32 CUDA(HIP) tensors, got {t.dtype} on {t.device}; "
                "there is no CPU fallback"
            )
