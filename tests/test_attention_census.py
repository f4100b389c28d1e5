"""Quantized attention forward, per launch path: an exact census of the keys every query saw (family A) and planted dominant keys at the block and
part boundaries (family B) -- see tests/attn_census_util.py.  The CPU tests prove that the case table reaches every path and that the two checks are
sharp (the mutants); the GPU tests run the table."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import attn_census_util as U

ALL_IDS = list(U.CASES)
DEFAULT_IDS = [c.id for c in U.DEFAULT_CASES]


@pytest.fixture(autouse=True)
def _launcher_makes_its_own_choice():
    U.require_default_tuning()


# ---- CPU: the table reaches what it claims ---------------------------------------------------------------------------------------------------
def test_launch_path_restates_the_launcher_on_known_shapes():
    # the shapes whose path the comments of tests/test_attention.py and sdnq_amd/csrc/attention.hip name
    assert U.launch_path(1, 10, 1024, 77, 64, False, False) == "inline"       # 77-key cross-attention: one launch
    assert U.launch_path(1, 5, 1, 500, 72, False, False) == "split4"          # 5 tiles, 16 key blocks: 4 parts of 4
    assert U.launch_path(1, 20, 1024, 1024, 64, False, False) == "split4"     # 640 tiles: 4 key parts
    assert U.launch_path(1, 18, 2048, 2100, 64, False, True) == "split4"      # 1152 tiles x 2 < 4096 and 66 key blocks
    assert U.launch_path(1, 10, 4096, 4096, 64, False, False) == "split4"     # SDXL: 1280 tiles x 2 < 4096
    assert U.launch_path(1, 24, 4608, 4608, 128, False, False) == "shared"    # FLUX
    assert U.launch_path(1, 24, 4608, 4608, 128, True, False) == "split2"     # causal: no sharing, 3456 tiles
    assert U.launch_path(4, 32, 131080, 131080, 128, False, False) == "shared"
    assert U.launch_path(4, 32, 131080, 131080, 64, False, False) == "whole"  # enough tiles
    # the thresholds: 8 / 16 key blocks, 4096 / 2048 tiles, 2048 keys and a padded head dim above 64 for sharing
    assert [U.launch_path(1, 2, 70, kn, 64, False, False) for kn in (128, 129, 224, 225, 480, 481)] == ["inline", "whole", "whole", "split2", "split2", "split4"]
    assert [U.launch_path(1, 1, 32 * t, 600, 64, False, False) for t in (2047, 2048, 4095, 4096)] == ["split4", "split2", "split2", "whole"]
    assert [U.launch_path(1, 2, 70, kn, d, False, False) for kn, d in ((2047, 128), (2048, 128), (2048, 72), (2048, 64))] == ["split4", "shared", "shared", "split4"]


def test_key_parts_deal_every_block_exactly_once():
    for kn in (129, 225, 300, 481, 520, 544, 581, 2100):
        for split in (1, 2, 4):
            for causal in (False, True):
                for masked in (False, True):
                    for q0 in range(0, 640, 32):
                        parts = U.key_parts(kn, q0, split, causal, masked)
                        nkb = min((kn + 31) // 32, q0 // 32 + 1) if causal else (kn + 31) // 32
                        assert sorted(b for p in parts for b in p) == list(range(nkb))
    assert [len(p) for p in U.key_parts(544, 0, 4, False, False)] == [5, 5, 5, 2]  # 17 plain blocks, no tail
    assert [len(p) for p in U.key_parts(581, 0, 4, False, False)] == [5, 5, 5, 4]  # 18 plain blocks (5, 5, 5, 3) and the tail
    assert [len(p) for p in U.key_parts(520, 0, 4, False, False)] == [4, 4, 4, 5]  # 16 plain blocks and the tail
    assert U.key_parts(520, 64, 4, True, False) == [[0], [1], [], [2]]             # causal: empty parts, the diagonal block in the last part only


def test_case_table_covers_every_path_and_form():
    by = {}
    for c in U.DEFAULT_CASES:
        by.setdefault(c.path, []).append(c)
    assert set(by) == {"inline", "whole", "split2", "split4", "shared"}
    need = {"inline": (1, 33, 128), "whole": (129, 224), "split2": (225, 256, 300, 480), "split4": (481, 512, 520, 544, 581)}
    for path, kns in need.items():
        cs = by[path]
        forms = ("plain", "causal", "mask") + (("mask+causal",) if path.startswith("split") else ())
        for kn in kns:
            for form in forms:
                assert any(c.kn == kn and c.form == form and (not c.causal or c.qn == kn) for c in cs), (path, kn, form)
        assert {c.tag for c in cs} == {"f16", "bf16"}, path
        assert {64, 128} <= {c.d for c in cs} and any(c.d in (40, 80) for c in cs), path
        assert any(c.qh == c.kh for c in cs) and any(c.qh > c.kh for c in cs) and any(c.z > 1 for c in cs), path
    for path in ("split2", "split4"):
        cs = by[path]
        for form in ("causal", "mask+causal"):  # q_len below and above kv_len: the first tiles have empty parts, the diagonal block sits in the last part only
            assert any(c.form == form and c.qn < c.kn for c in cs) and any(c.form == form and c.qn > c.kn for c in cs), (path, form)
        c = next(c for c in cs if c.form == "causal" and c.qn > c.kn)
        first = U.key_parts(c.kn, 0, c.split, True, False)
        assert first[-1] == [0] and not any(first[:-1])
        assert {c.mask for c in cs} == {None, "bool", "f32", "bf16", "bcast"}, path
        for c in cs:  # masked: some query tile has a part (part 0 for one tile, a later part for another) that sees nothing, and one row sees nothing
            if c.mask in ("bool", "f32", "bf16") and not c.causal:
                vis = U.inputs(c, "A")["vis"]
                empty = set()
                for q0 in range(0, c.qn, 32):
                    for part, blocks in enumerate(U.key_parts(c.kn, q0, c.split, False, True)):
                        if blocks and not any(vis[:, q0:q0 + 32, b * 32:(b + 1) * 32].any() for b in blocks):
                            empty.add(part)
                assert 0 in empty and 1 in empty, c.id
                assert (vis.sum(-1) == 0).any() and ((vis.reshape(c.qh, c.qn, -1)[:, :, 32:64]).sum() == 0), c.id
    sh = by["shared"]
    assert {(c.qn, c.kn) for c in sh} == {(33, 2048), (130, 2048), (33, 2100), (130, 2100)} and {c.d for c in sh} == {128}
    assert {c.tag for c in sh} == {"f16", "bf16"} and any(c.qh == c.kh for c in sh) and any(c.qh > c.kh for c in sh)
    for c in sh:  # causal and masked calls of these shapes fall back to the key split, which the split rows cover
        assert U.launch_path(c.z, c.qh, c.qn, c.kn, c.d, True, False) == "split4" and U.launch_path(c.z, c.qh, c.qn, c.kn, c.d, False, True) == "split4"
    # the other formats: every format at every key length and in every form, both head dims, one bf16 column
    vs = U.VARIANT_CASES
    for mm, pv in U.VARIANT_FORMATS:
        cs = [c for c in vs if (c.mm, c.pv) == (mm, pv)]
        assert {c.kn for c in cs} == set(U.VARIANT_KN) and {c.d for c in cs} == {64, 128} and {c.tag for c in cs} == {"f16", "bf16"}, (mm, pv)
        assert {c.form for c in cs} == {"plain", "causal", "mask", "mask+causal"}
        assert {np.sign(c.qn - c.kn) for c in cs if c.form == "causal"} == {-1, 0, 1}
    for kn in U.VARIANT_KN:
        assert sum(c.kn == kn for c in vs) == len(U.VARIANT_FORMS)
    assert len(U.CASES) <= 120  # x 2 families x 2 query layouts: a few hundred launches


@pytest.mark.parametrize("cid", DEFAULT_IDS)
def test_planted_rows_of_a_tile_sit_in_different_parts(cid):
    """Family B: the planted keys cover every critical key the rows can reach, and within one query tile they fall into different key parts."""
    c = U.CASES[cid]
    x = U.inputs(c, "B")
    pos, vis = x["pos"], x["vis"]
    crit = U.critical_keys(c.kn)
    if c.qh * c.qn >= len(crit) and c.form == "plain":
        assert set(crit) == set(pos.ravel().tolist()), cid
    assert not vis[:, :, crit][pos < 0].any() and vis[np.nonzero(pos >= 0) + (pos[pos >= 0],)].all()  # planted keys are visible; no row is left out needlessly
    if c.split > 1:
        several = 0
        for h in range(c.qh):
            for q0 in range(0, c.qn - 31, 32):  # full tiles
                parts = U.key_parts(c.kn, q0, c.split, c.causal, c.mask is not None)
                owner = {b: p for p, blocks in enumerate(parts) for b in blocks}
                several += len({owner[j // 32] for j in pos[h, q0:q0 + 32] if j >= 0}) > 1
        if not (c.causal and c.qn < c.kn):  # (70 causal rows: two full tiles of one and two key blocks)
            assert several >= 1, cid
        if not c.causal and c.mask is None:
            assert several == c.qh * (c.qn // 32)


# ---- CPU: the references agree, and the checks are sharp --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ALL_IDS)
def test_census_reference_matches_oracle(cid):
    """Family A: the oracle's restatement of the kernel arithmetic lands on the float64 census to within 0.01 key on every case (so the quarter-key
    bound of the GPU test leaves the kernel 25 times the oracle's own error)."""
    c = U.CASES[cid]
    ref, n = U.census_reference(c)
    U.assert_census(U.run_oracle(c, "A", out_tag="f32"), ref, n, cid, bound=0.01)


@pytest.mark.parametrize("cid", ALL_IDS)
def test_planted_key_removal_moves_its_row(cid):
    """Family B: taking the planted key alone away from a row (through the oracle's mask) moves that row by at least 10 times the limit the GPU test
    compares at -- for every planted row, hence every critical key."""
    c = U.CASES[cid]
    x = U.inputs(c, "B")
    ref = U.planted_reference(c)
    vis = x["vis"].copy()
    h, i = np.nonzero(x["pos"] >= 0)
    vis[h, i, x["pos"][h, i]] = False
    without = U.run_oracle(c, "B", mask=vis[None])
    moved = np.abs(without - ref).max(-1) / np.abs(ref).max()  # [Z, QH, QN]
    lim = U.planted_limits(c)[0]
    assert h.size and moved[:, h, i].min() >= 10 * lim, (cid, float(moved[:, h, i].min()), lim)
    with pytest.raises(AssertionError, match="worst at batch"):
        U.assert_planted(without, ref, *U.planted_limits(c), cid)


def _case(path, form, **kw):
    return next(c for c in U.DEFAULT_CASES if c.path == path and c.form == form and all(getattr(c, k) == v for k, v in kw.items()))


def _partwise(c, x, vis, parts_of_tile, skip_factor_of=None):
    """float64 flash attention in key parts on the oracle's quantized operands: per query tile every part keeps (m, l, o) over its own blocks and the
    parts are merged as attention.hip:671-690 does.  `skip_factor_of`: that part is merged without its 2^(m_i - m) weight (the mutant)."""
    _, qs, _, ks, vals = O.attention_quantize(x["q"], x["k"], True, 0, c.tag, c.mm, v=x["v"])
    out = np.zeros((c.z, c.qh, c.qn, c.d))
    for z in range(c.z):
        for h in range(c.qh):
            kh = h * c.kh // c.qh
            s = (vals["q"][z, h].astype(np.float64) @ vals["k"][z, kh].astype(np.float64).T) * qs[z, h][:, None] * ks[z, kh][None] * (c.d ** -0.5 * np.log2(np.e))
            s = np.where(vis[h], s, -np.inf)
            for q0 in range(0, c.qn, 32):
                rows = slice(q0, min(q0 + 32, c.qn))
                ms, ls, os_ = [], [], []
                for blocks in parts_of_tile(q0):
                    keys = np.array([j for b in blocks for j in range(b * 32, min(b * 32 + 32, c.kn))], dtype=np.int64)
                    sp = s[rows][:, keys]
                    m = sp.max(-1, initial=-np.inf)
                    p = np.exp2(sp - np.where(np.isneginf(m), 0.0, m)[:, None])
                    ms.append(m)
                    ls.append(p.sum(-1))
                    os_.append(p @ vals["v"][z, kh][keys].astype(np.float64))
                m = np.max(ms, axis=0)
                m = np.where(np.isneginf(m), 0.0, m)
                w = [np.ones_like(m) if i == skip_factor_of else np.exp2(mi - m) for i, mi in enumerate(ms)]
                l = sum(wi * li for wi, li in zip(w, ls))
                o = sum(wi[:, None] * oi for wi, oi in zip(w, os_))
                out[z, h, rows] = o / np.where(l > 0, l, 1.0)[:, None]
    return out


def test_mutants_are_caught():
    """The classic mistakes of a key-split flash kernel, built from the oracle, and which of the two checks sees each.  The census sees every key
    that is dropped, counted twice or let through; only the planted keys see the running maximum (in the census all maxima are equal and every merge
    weight is 1), and they see a dropped key where it is the dominant one."""
    def census_catches(c, got, what):
        ref, n = U.census_reference(c)
        with pytest.raises(AssertionError, match=r"worst at batch \d+ head \d+ row \d+ channel \d+: [+-]"):
            U.assert_census(got, ref, n, what)

    def planted_catches(c, got, what):
        with pytest.raises(AssertionError, match="worst at batch"):
            U.assert_planted(got, U.planted_reference(c), *U.planted_limits(c), what)

    c = _case("split4", "plain", kn=581)
    parts = U.key_parts(c.kn, 0, 4, False, False)
    # 1. the last key of part 0 dropped
    vis = U.inputs(c, "A")["vis"].copy()
    last0 = parts[0][-1] * 32 + 31
    vis[:, :, last0] = False
    census_catches(c, U.run_oracle(c, "A", mask=vis[None], out_tag="f32"), "last key of part 0 dropped")
    assert (U.inputs(c, "B")["pos"] == last0).any()
    planted_catches(c, U.run_oracle(c, "B", mask=vis[None]), "last key of part 0 dropped")
    # 2. the tail block counted twice: the tail keys appended once more
    tail = slice(c.kn // 32 * 32, c.kn)
    x = U.inputs(c, "A")
    twice = O.attention(x["q"], np.concatenate([x["k"], x["k"][:, :, tail]], 2), np.concatenate([x["v"], x["v"][:, :, tail]], 2), c.tag, out_tag="f32")
    census_catches(c, twice, "tail block counted twice")
    # 3. one part merged without its 2^(m_i - m) factor: the correct part-wise merge passes, the mutant does not
    xb = U.inputs(c, "B")
    tile_parts = lambda q0: U.key_parts(c.kn, q0, 4, False, False)  # noqa: E731
    U.assert_planted(_partwise(c, xb, xb["vis"], tile_parts), U.planted_reference(c), *U.planted_limits(c), "part-wise merge")
    for part in range(4):
        planted_catches(c, _partwise(c, xb, xb["vis"], tile_parts, skip_factor_of=part), f"part {part} merged without its factor")
    ref, n = U.census_reference(c)
    U.assert_census(_partwise(c, x, x["vis"], tile_parts, skip_factor_of=1), ref, n, "the census cannot see a merge weight")
    # 4. key i + 1 visible under causal
    c = _case("split4", "causal", kn=520, qn=520)
    vis = np.broadcast_to(np.arange(c.kn)[None, :] <= np.arange(c.qn)[:, None] + 1, (c.qh, c.qn, c.kn))
    x = U.inputs(c, "A")
    leaky = O.attention(x["q"], x["k"], x["v"], c.tag, is_causal=False, mask=vis[None], out_tag="f32")
    census_catches(c, leaky, "key i + 1 visible under causal")
    # 5. a masked block let through
    c = _case("split2", "mask", kn=300)
    vis = U.inputs(c, "A")["vis"].copy()
    assert not vis[:, :, 32:64].any()
    vis[:, :, 32:64] = True
    census_catches(c, U.run_oracle(c, "A", mask=vis[None], out_tag="f32"), "a masked block let through")


def test_census_flags_one_key_in_2100():
    """The sharpness the big oracle comparisons lack: one key of 2100 dropped, or counted twice, in one row of the largest case."""
    c = next(c for c in U.DEFAULT_CASES if c.path == "shared" and (c.qn, c.kn) == (130, 2100))
    ref, n = U.census_reference(c)
    got = ref.astype(np.float32)
    assert U.assert_census(got, ref, n, c.id) < 1e-3
    for delta in (-1.0, 1.0):
        bad = got.copy()
        bad[0, 1, 77] = ((ref[0, 1, 77] * 2100 + delta * (np.arange(c.d) == 2047 % c.d)) / (2100 + delta)).astype(np.float32)
        with pytest.raises(AssertionError, match=r"row 77 channel 127: [+-]0\.9"):
            U.assert_census(bad, ref, n, c.id)
    nan = got.copy()
    nan[0, 0, 3, 5] = np.nan
    with pytest.raises(AssertionError, match="row 3 channel 5"):
        U.assert_census(nan, ref, n, c.id)


def test_tuning_overrides_fail_with_a_clear_message(monkeypatch):
    monkeypatch.setattr(U, "_TUNING_SET", {"SDNQ_HIP_ATTN_SPLIT": "2"})
    with pytest.raises(AssertionError, match="unset .*SDNQ_HIP_ATTN_SPLIT"):
        U.require_default_tuning()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def _gpu_run(c, family, dev, out_f32):
    """The kernel's output for the case, as float32 numpy: on contiguous tensors and once more on the token-major query view an attention processor
    passes (tests/test_attention.py, test_hip_attention_strided_views_match_contiguous)."""
    import torch
    from sdnq_amd import attention as A
    x = U.inputs(c, family)
    tdt = {"bf16": torch.bfloat16, "f16": torch.float16}[c.tag]
    q, k, v = (torch.tensor(x[t], dtype=tdt, device=dev) for t in ("q", "k", "v"))
    mask = None
    if x["mask"] is not None:
        mask = torch.tensor(x["mask"], dtype=torch.bfloat16 if c.mask == "bf16" else None, device=dev)
    kw = dict(attn_mask=mask, out_dtype=torch.float32 if out_f32 else None, **c.kwargs())
    q_tm = q.transpose(1, 2).contiguous().transpose(1, 2)
    assert q_tm.stride(2) > q_tm.stride(1) or c.qn == 1
    outs = [A.sdnq_hip_atten(qv, k, v, **kw) for qv in (q, q_tm)]
    assert all(o.dtype == (torch.float32 if out_f32 else tdt) and o.shape == q.shape for o in outs)
    return [(o.float().cpu().numpy(), what) for o, what in zip(outs, ("contiguous", "token-major query"))]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ALL_IDS)
def test_hip_attention_key_census(cid, gpu_device):
    """Family A: every query counted exactly its visible keys -- to a quarter of one key, per row and channel."""
    c = U.CASES[cid]
    ref, n = U.census_reference(c)
    for got, what in _gpu_run(c, "A", gpu_device, out_f32=True):
        err = np.abs(U.census_error(got, ref, n)).max()
        print(f"CENSUS path={c.path} fmt={c.fmt} tag={c.tag} keys={err:.3e} case={cid} ({what})")
        U.assert_census(got, ref, n, f"{cid} ({what})")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ALL_IDS)
def test_hip_attention_planted_keys(cid, gpu_device):
    """Family B: a dominant key planted at every block and part boundary, against the oracle at the limits of tests/test_attention.py."""
    c = U.CASES[cid]
    ref = U.planted_reference(c)
    lim, lim2 = U.planted_limits(c)
    for got, what in _gpu_run(c, "B", gpu_device, out_f32=False):
        err = np.abs(got - ref).max() / np.abs(ref).max()
        err2 = np.linalg.norm(got - ref) / np.linalg.norm(ref)
        print(f"PLANTED path={c.path} fmt={c.fmt} tag={c.tag} max={err:.3e} l2={err2:.3e} lim={lim:g} lim2={lim2:g} case={cid} ({what})")
        U.assert_planted(got, ref, lim, lim2, f"{cid} ({what})")
