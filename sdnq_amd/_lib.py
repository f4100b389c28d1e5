"""ctypes binding of the C-ABI library ``libsdnq_hip.so`` (include/sdnq_hip.h).

The shared object is built in-tree by ``build()`` (the recipe is ``sdnq_amd/_build.py``; hipcc --offload-arch=gfx950) so
that it travels with the source snapshot; nothing here falls back to another implementation: if
the library is missing or the device is not gfx950 the product path raises.
"""
from __future__ import annotations

import ctypes
import os
import threading

from . import _abi, _build
from ._abi import SdnqHipError  # noqa: F401  (raised here, defined beside the header reader)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDNQ_HIP_LIB") or os.path.join(_HERE, "libsdnq_hip.so")  # override: development builds only

with open(_build._API_H) as _f:  # read once: everything below that mirrors include/sdnq_hip.h comes from it
    _ABI = _abi.Header(_f.read())

# the enum constants without their SDNQ_ prefix: F32 BF16 F16, MM_*, ST_*, IDS_*, KIND_*, OK and ERR_* (SdnqStatus)
globals().update({name[len("SDNQ_"):]: value for name, value in _ABI.enums.items()})
EXPORTS = [name for (_, name, _) in _ABI.prototypes]
SdnqWeight, SdnqLinearArgs = _ABI.classes["SdnqWeight"], _ABI.classes["SdnqLinearArgs"]
SdnqGemmUnit = _ABI.classes["SdnqGemmUnit"]  # the table of these lives in DEVICE memory: passed as an address

_lock = threading.Lock()
_lib = None


def source_hash() -> str:
    """The source hash of the tree (_build.source_hash): the library that is loaded is the one built from the sources in the tree iff
    this equals the contents of ``libsdnq_hip.so.srchash``."""
    return _build.source_hash()


def lib_is_current() -> bool:
    try:
        return (os.path.exists(LIB_PATH) and all(os.path.exists(f) for f in _build.host_modules(LIB_PATH))
                and open(LIB_PATH + ".srchash").read().strip() == source_hash())
    except OSError:
        return False


def build(force: bool = False) -> str:
    """Compile every HIP source for gfx950 into sdnq_amd/libsdnq_hip.so (no GPU needed).  Content-addressed: nothing is rebuilt
    when the library's recorded source hash equals the hash of the tree; `force` recompiles every object."""
    if force or not lib_is_current():
        _build.build(LIB_PATH, force=force)
    return LIB_PATH


def _declare(lib):
    for name, (restype, argtypes) in _ABI.signatures.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    # the one exception to the header's types (the SdnqWeight by address: csrc/binding.c serves it too)
    lib.sdnq_hip_embedding.argtypes = [ctypes.c_void_p] + _ABI.signatures["sdnq_hip_embedding"][1][1:]


def load():
    """Load the library (building it first if the sources are newer). Raises if unavailable."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise SdnqHipError(
                        f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950). There is no fallback path.")
                lib = ctypes.CDLL(LIB_PATH)
                _declare(lib)
                _lib = _with_typed_binding(lib)
    return _lib


USE_BINDING = os.environ.get("SDNQ_HIP_BINDING", "1").lower() not in {"0", "false", "no"}


class _BoundLib:
    """The ctypes handle with its hot entry points served by the typed CPython binding (csrc/binding.c: the same named symbols of
    the same library, ~0.5 us instead of ~10 us of argument conversion per call; an eager diffusion step makes ~900 calls).
    Every other entry point -- and every entry point when _binding.so is absent or SDNQ_HIP_BINDING=0 -- goes through ctypes."""

    def __init__(self, lib, binding):
        self._ctypes = lib
        for name in dir(binding):
            if name.startswith("sdnq_hip_"):
                setattr(self, name, getattr(binding, name))

    def __getattr__(self, name):  # not in the binding: the ctypes function
        return getattr(self._ctypes, name)


def _with_typed_binding(lib):
    if not USE_BINDING:
        return lib
    try:
        from . import _binding  # built by build() next to the library
    except ImportError:
        return lib  # binding only: every call still lands in libsdnq_hip.so, through ctypes
    _binding.init(LIB_PATH)
    return _BoundLib(lib, _binding)


USE_FAST_PLANS = os.environ.get("SDNQ_HIP_FAST_PLANS", "1").lower() not in {"0", "false", "no"}
_fastpath = None  # None: not looked for yet; False: unavailable / switched off


def fastpath():
    """The C++ fast path of the eager Linear forward (csrc/fastpath.cpp -> sdnq_amd/_fastpath.so), or None with SDNQ_HIP_FAST_PLANS=0 /
    when the module or the kernel library is not built: host logic only -- every launch it makes is a named entry point of
    libsdnq_hip.so, and sdnq_amd/linear.py is the complete forward without it."""
    global _fastpath
    if _fastpath is None:
        with _lock:
            if _fastpath is None:
                mod = False
                if USE_FAST_PLANS and os.path.exists(LIB_PATH):
                    try:
                        import torch  # noqa: F401  (the module links against torch's libraries: they must be loaded first)
                        from . import _fastpath as mod
                        mod.init(LIB_PATH)
                    except (ImportError, OSError) as e:
                        import warnings
                        warnings.warn(f"sdnq_amd._fastpath is unavailable ({e}); eager Linear calls take the Python forward")
                        mod = False
                _fastpath = mod
    return _fastpath or None


def check(status: int, what: str = ""):
    if status != 0:
        lib = load()
        try:  # a call that failed in front of its GEMM launch leaves its weight-prefetch hint pending: drop it
            lib.sdnq_hip_prefetch_hint(None, 0, None, 0, None, 0, None, 0)
        except Exception:  # noqa: BLE001
            pass
        msg = lib.sdnq_hip_strerror(status).decode()
        raise SdnqHipError(f"sdnq_hip {what} failed: {msg} (status {status})")
