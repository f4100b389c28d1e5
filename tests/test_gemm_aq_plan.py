"""The one-launch Linear's choice function (csrc/gemm_aq.hip, aq_plan): shape -> tile geometry, tile counts, row-block grouping of the
walk and the room left for hosted weight-prefetch workgroups.  No GPU: the function is host code.

The table is the heuristic, written out: the 32 x 256 geometry (3 ring slots) runs for int8 problems with K of more than five 128-byte
stages, N a multiple of 256 and at most one tile per CU; everything else keeps 64 x 128 (4 ring slots).  An edit that turns the route
off, or moves it to other shapes, fails here."""
import pytest

from tests import aq_internal as A

MM_I8, MM_FP8 = 0, 1
CUS = 256

#        mm      M     N     K    geometry tiles_m tiles_n group_m room
TABLE = [
    (MM_I8, 1024, 1280, 1280, 1, 32, 5, 8, 96),    # the SDXL step's one-launch shape: 160 workgroups, 96 CUs for the prefetch
    (MM_I8, 1000, 1280, 1280, 1, 32, 5, 8, 96),    # ragged M
    (MM_I8, 2048, 1280, 1280, 0, 32, 10, 8, -64),   # 64 x 5 = 320 tiles of 32 x 256: more than one round -> 64 x 128
    (MM_I8, 1024, 1280, 640, 0, 16, 10, 8, 96),     # five K stages: the front is short already
    (MM_I8, 1024, 640, 1280, 0, 16, 5, 8, 176),     # N not a multiple of 256
    (MM_I8, 1024, 1152, 1280, 0, 16, 9, 8, 112),
    (MM_I8, 1024, 1280, 768, 1, 32, 5, 8, 96),     # six stages
    (MM_I8, 96, 256, 1280, 1, 3, 1, 3, 253),        # the grouping never exceeds the row blocks there are
    (MM_FP8, 1024, 1280, 1280, 0, 16, 10, 8, 96),   # fp8 keeps the 64 x 128 tile
]


@pytest.fixture(autouse=True)
def _by_shape():
    A.set_geometry(-1)
    yield
    A.set_geometry(-1)


@pytest.mark.parametrize("mm,m,n,k,geo,tm,tn,gm,room", TABLE)
def test_plan_is_the_heuristics_table(mm, m, n, k, geo, tm, tn, gm, room):
    p = A.plan(mm, m, n, k, CUS)
    bm, bn = ((64, 128), (32, 256))[geo]
    assert p == dict(geometry=geo, bm=bm, bn=bn, tiles_m=tm, tiles_n=tn, group_m=gm, prefetch_room=room), p


def test_fewer_cus_move_the_choice():
    """The one-round condition reads the part's CU count: 160 tiles do not fit 128 CUs."""
    assert A.plan(MM_I8, 1024, 1280, 1280, 160)["geometry"] == 1
    assert A.plan(MM_I8, 1024, 1280, 1280, 128)["geometry"] == 0


def test_forced_geometry_overrides_the_shape_rule():
    A.set_geometry(A.GEO_32x256)
    p = A.plan(MM_FP8, 100, 136, 256, CUS)
    assert (p["geometry"], p["bm"], p["bn"], p["tiles_m"], p["tiles_n"], p["prefetch_room"]) == (1, 32, 256, 4, 1, 252)
    A.set_geometry(A.GEO_64x128)
    p = A.plan(MM_I8, 1024, 1280, 1280, CUS)
    assert (p["geometry"], p["bm"], p["bn"], p["tiles_m"], p["tiles_n"], p["group_m"], p["prefetch_room"]) == (0, 64, 128, 16, 10, 8, 96)
