"""Bindings of the one-launch Linear's library-internal hooks (csrc/gemm_aq.hip; C++ symbols, not part of the C ABI of include/sdnq_hip.h)."""
import ctypes

from sdnq_amd import _lib

GEO_64x128, GEO_32x256 = 0, 1
PLAN_FIELDS = ("geometry", "bm", "bn", "tiles_m", "tiles_n", "group_m", "prefetch_room")


def _cdll():
    _lib.load()
    return ctypes.CDLL(_lib.LIB_PATH)


def set_geometry(geometry: int) -> None:
    """-1: by shape (the default); 0: 64 x 128; 1: 32 x 256."""
    f = getattr(_cdll(), "_Z25sdnq_internal_aq_geometryi")
    f.argtypes, f.restype = [ctypes.c_int], None
    f(geometry)


def plan(mm: int, m: int, n: int, k: int, cus: int) -> dict:
    """What sdnq_hip_linear_w8a8_fused chooses for this problem on a part with `cus` CUs."""
    f = getattr(_cdll(), "_Z21sdnq_internal_aq_planixxxiPx")
    f.argtypes, f.restype = [ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)], None
    out = (ctypes.c_longlong * len(PLAN_FIELDS))()
    f(mm, m, n, k, cus, out)
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))
