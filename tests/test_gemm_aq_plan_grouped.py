"""The rule of the grouped one-launch Linear (aq_plan_grouped in csrc/gemm_aq.hip), through the library's planning hook: no launch, no
GPU.  A group is accepted where its members are int8 layers of ONE width that is a multiple of the 256-column block, K is six to ten
stages of 128, and every 32 x 256 tile of every member is resident at once -- two per CU (the direct form keeps no weight ring in LDS).
An accepted launch gets NO prefetch room: a hosted prefetch workgroup would share a CU with a tile, and the step measured slower with them
(profiles/linear_aq_qkv_grouped.txt)."""
import ctypes

import pytest

from sdnq_amd import _lib

FIELDS = ("ok", "bm", "bn", "tiles_m", "tiles_n", "group_m", "resident", "prefetch_room")


def plan(m, n_member, n_members, k, cus):
    _lib.load()
    f = getattr(ctypes.CDLL(_lib.LIB_PATH), "_Z29sdnq_internal_aq_plan_groupedxxxxiPx")
    f.argtypes, f.restype = [ctypes.c_longlong] * 4 + [ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)], None
    out = (ctypes.c_longlong * len(FIELDS))()
    f(m, n_member, n_members, k, cus, out)
    return dict(zip(FIELDS, (int(v) for v in out)))


def test_the_sdxl_qkv_group_is_one_round_of_two_tiles_per_cu():
    p = plan(1024, 1280, 3, 1280, 256)
    assert p == {"ok": 1, "bm": 32, "bn": 256, "tiles_m": 32, "tiles_n": 15, "group_m": 8, "resident": 2, "prefetch_room": 0}
    assert plan(1024, 1280, 3, 1280, 240)["ok"] == 1              # exactly one round
    assert plan(1024, 1280, 3, 1280, 239)["ok"] == 0              # a second round: the two launches keep the group


@pytest.mark.parametrize("m, n, g, k, cus, tiles_m, tiles_n", [
    (33, 256, 2, 768, 256, 2, 2),     # the smallest K; a ragged second row block
    (160, 512, 3, 896, 256, 5, 6),
    (1024, 1280, 2, 1280, 256, 32, 10),
    (256, 256, 2, 1280, 64, 8, 2),    # a smaller part
    (1024, 256, 4, 1280, 64, 32, 4),  # ... filled to its last slot: 128 tiles on 64 CUs
    (32, 256, 8, 1280, 64, 1, 8),     # eight members
])
def test_accepted(m, n, g, k, cus, tiles_m, tiles_n):
    p = plan(m, n, g, k, cus)
    assert p["ok"] == 1 and (p["bm"], p["bn"], p["resident"]) == (32, 256, 2)
    assert (p["tiles_m"], p["tiles_n"]) == (tiles_m, tiles_n)
    assert p["group_m"] == min(8, tiles_m)
    assert p["prefetch_room"] == 0


@pytest.mark.parametrize("m, n, g, k, cus, why", [
    (1024, 1280, 3, 1280, 64, "480 tiles on a 64-CU part: four rounds"),
    (4096, 640, 3, 640, 256, "K = 640: five stages, the tall single-layer forms' range (and 960 tiles)"),
    (4096, 1280, 3, 1280, 256, "1920 tiles"),
    (77, 1280, 2, 2048, 256, "the cross-attention k / v group: K = 2048 does not stay resident"),
    (1024, 1280, 3, 1408, 256, "K > 1280"),
    (1024, 1280, 3, 1200, 256, "K % 128"),
    (1024, 320, 3, 1280, 256, "n_member % 256"),
    (1024, 1280, 9, 1280, 1024, "more members than the kernel's table holds"),
    (1024, 1280, 0, 1280, 256, "no member"),
    (0, 1280, 3, 1280, 256, "no row"),
])
def test_rejected(m, n, g, k, cus, why):
    assert plan(m, n, g, k, cus)["ok"] == 0, why
