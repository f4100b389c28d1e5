"""The one-launch Linear's choice function (csrc/gemm_aq.hip, aq_plan) on the problems whose 64 x 128 tiles outnumber the CUs.  No GPU:
the function is host code.

The rule, written out: int8, K of at most five 128-byte stages, more tiles of 64 x 128 than CUs, but no more than the resident
workgroup slots of the tall form -> geometry 2, the 64 x 128 tile on a 2-slot weight ring, two workgroups per CU.  Its prefetch room
is resident slots - tiles = 2 CUs - tiles.  Everything else answers as tests/test_gemm_aq_plan.py's table says; a few of its rows are repeated here as a guard."""
import pytest

from sdnq_amd import _lib
from tests import aq_internal as A

MM_I8, MM_FP8 = 0, 1
BF16 = 1
CUS = 256
GEO_TALL = 2
SHAPE = {0: (64, 128), 1: (32, 256), 2: (64, 128)}

#        mm      M     N     K    cus  geometry tiles_m tiles_n group_m room
TABLE = [
    (MM_I8, 4096, 640, 640, 256, 2, 64, 5, 8, 192),     # the SDXL step's 640-channel projections: 320 tiles on 512 slots
    (MM_I8, 4096, 640, 384, 256, 2, 64, 5, 8, 192),     # fewer stages than the image holds
    (MM_I8, 4000, 640, 640, 256, 2, 63, 5, 8, 197),     # ragged M
    (MM_I8, 4096, 1024, 128, 256, 2, 64, 8, 8, 0),      # exactly the resident slots
    (MM_I8, 4096, 640, 1280, 256, 0, 64, 5, 8, -64),    # ten stages: the tall image holds five
    (MM_I8, 4096, 640, 768, 256, 0, 64, 5, 8, -64),
    (MM_FP8, 4096, 640, 640, 256, 0, 64, 5, 8, -64),    # fp8 stays on the 64 x 128 tile (and off the route)
    (MM_I8, 4160, 1024, 128, 256, 0, 65, 8, 8, -264),   # 520 tiles: more than 2 x 256 slots
    (MM_I8, 8192, 640, 640, 256, 0, 128, 5, 8, -384),
    (MM_I8, 3264, 640, 640, 256, 0, 51, 5, 8, 1),       # 255 tiles: one round of geometry 0 fits, nothing changes
    (MM_I8, 2048, 640, 640, 128, 2, 32, 5, 8, 96),      # 160 tiles on a 128-CU part: 256 slots
    (MM_I8, 4096, 640, 640, 128, 0, 64, 5, 8, -192),    # ... where 320 tiles do not fit
    (MM_I8, 2048, 640, 640, 256, 0, 32, 5, 8, 96),
    # rows of tests/test_gemm_aq_plan.py, unchanged
    (MM_I8, 1024, 1280, 1280, 256, 1, 32, 5, 8, 96),
    (MM_I8, 2048, 1280, 1280, 256, 0, 32, 10, 8, -64),
    (MM_I8, 1024, 1280, 640, 256, 0, 16, 10, 8, 96),
    (MM_I8, 96, 256, 1280, 256, 1, 3, 1, 3, 253),
    (MM_FP8, 1024, 1280, 1280, 256, 0, 16, 10, 8, 96),
]


@pytest.fixture(autouse=True)
def _by_shape():
    A.set_geometry(-1)
    yield
    A.set_geometry(-1)


@pytest.mark.parametrize("mm,m,n,k,cus,geo,tm,tn,gm,room", TABLE)
def test_plan_of_the_tall_problems(mm, m, n, k, cus, geo, tm, tn, gm, room):
    p = A.plan(mm, m, n, k, cus)
    bm, bn = SHAPE[geo]
    assert p == dict(geometry=geo, bm=bm, bn=bn, tiles_m=tm, tiles_n=tn, group_m=gm, prefetch_room=room), p


def test_supported_follows_the_plan():
    """`supported()` reads the device's CU count, 256 where there is no device: one round of resident tiles or no one-launch route."""
    sup = _lib.load().sdnq_hip_linear_w8a8_fused_supported
    assert sup(MM_I8, BF16, BF16, 4096, 640, 640) == 1
    assert sup(MM_I8, BF16, BF16, 4096, 640, 384) == 1
    assert sup(MM_I8, BF16, BF16, 4096, 640, 768) == 0     # K of six stages, 320 tiles
    assert sup(MM_I8, BF16, BF16, 4096, 640, 1280) == 0
    assert sup(MM_I8, BF16, BF16, 8192, 640, 640) == 0     # 640 tiles
    assert sup(MM_FP8, BF16, BF16, 4096, 640, 640) == 0
    assert sup(MM_I8, BF16, BF16, 1024, 1280, 1280) == 1   # as before
    assert sup(MM_I8, BF16, BF16, 2048, 1280, 1280) == 0


def test_forced_tall_geometries():
    """The hook reaches the tall form; on a problem it has no kernel for (fp8, K > 640) the shape rule answers instead.  An id the hook
    does not know (3) answers as id 1 does."""
    A.set_geometry(GEO_TALL)
    p = A.plan(MM_I8, 200, 136, 384, CUS)
    assert (p["geometry"], p["bm"], p["bn"], p["tiles_m"], p["tiles_n"], p["group_m"], p["prefetch_room"]) == (2, 64, 128, 4, 2, 4, 504)
    assert A.plan(MM_I8, 1024, 1280, 1280, CUS)["geometry"] == 1
    assert A.plan(MM_FP8, 200, 136, 384, CUS)["geometry"] == 0
    A.set_geometry(A.GEO_32x256)
    as_one = A.plan(MM_I8, 200, 136, 384, CUS)
    A.set_geometry(3)
    assert A.plan(MM_I8, 200, 136, 384, CUS) == as_one and as_one["geometry"] == 1
    A.set_geometry(A.GEO_64x128)
    assert A.plan(MM_I8, 4096, 640, 640, CUS)["geometry"] == 0
