"""Quantized attention backward, per kernel (lse, delta, dQ, dK / dV of sdnq_amd/csrc/attention_bwd.hip): an exact census of the queries and keys
every gradient element counted (family A), planted dominant keys on every in-block position (family B) and the random sweeps per element instead
of per norm (family C) -- see tests/attn_bwd_census_util.py.  The CPU tests prove the inputs exact, the table complete, the tiers reachable by a
correct implementation and the checks sharp (the mutants); the GPU tests run the table."""
import math

import numpy as np
import pytest
import torch

from tests import attn_bwd_census_util as U

IDS = list(U.CASES)
B_IDS = [c.id for c in U.CASES.values() if "B" in c.families]
VARIANTS = ("count", "delta")


# ---- CPU: K in fragment order -------------------------------------------------------------------------------------------------------------------
def test_pack_k_fragments_inverts_unpack():
    from sdnq_amd.attention import unpack_k_fragments
    g = torch.Generator().manual_seed(3)
    for dp in (64, 128):
        x = torch.randint(-128, 128, (2, 3, 96, dp), generator=g, dtype=torch.int8)
        f = U.pack_k_fragments(x)
        assert f.shape == (2, 3, 3, dp // 32, 64, 16) and f.is_contiguous()
        assert torch.equal(unpack_k_fragments(f), x)
        assert torch.equal(U.pack_k_fragments(unpack_k_fragments(f)), f)
    # lane g * 32 + rho holds bytes [32 kk + 16 g, + 16) of key pi(rho): one entry by hand (rho 4 <-> key 8)
    x = torch.zeros(1, 1, 32, 64, dtype=torch.int8)
    x[0, 0, 8, 32 + 16 + 5] = 77
    assert U.pack_k_fragments(x)[0, 0, 0, 1, 32 + 4, 5] == 77


# ---- CPU: the table -----------------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_kernel_and_form():
    cs = list(U.CASES.values())
    assert len(cs) <= 40  # + 22 family C cases: under 100 in all
    assert {c.instance for c in cs} == {"bf16/64", "bf16/128", "f16/64", "f16/128"}
    for inst in ("bf16/64", "bf16/128", "f16/64", "f16/128"):  # every instance: causal, masked, grouped heads, a float32 gradient
        mine = [c for c in cs if c.instance == inst]
        assert any(c.causal for c in mine) and any(c.mask for c in mine) and any(c.ratio > 1 for c in mine) and any(c.gdt == "f32" for c in mine), inst
        assert {c.assign for c in mine} == {"inblock", "block"}, inst
    assert {c.d for c in cs} == {8, 24, 40, 64, 72, 80, 128}
    assert {(c.tag, c.gdt) for c in cs} == {("bf16", "bf16"), ("f16", "f16"), ("bf16", "f32"), ("f16", "f32")}
    assert {1, 31, 32, 33, 72, 129} <= {c.qn for c in cs} and {1, 33, 64, 97, 200} <= {c.kn for c in cs}
    for sign in (-1, 0, 1):  # causal with q_len below, equal to, above kv_len, each with a key tail
        assert any(c.causal and np.sign(c.qn - c.kn) == sign and c.kn % 32 and c.kn > 32 for c in cs), sign
    assert {c.ratio for c in cs if c.z > 1} >= {1, 2, 4}
    masked = [c for c in cs if c.mask]
    assert {c.mask for c in masked} == {"bool", "f32", "bf16", "f16"}
    assert all(any(dim in c.bcast for c in masked) for dim in "zhq") and any(not c.bcast for c in masked)
    for c in masked:
        m = U.census_inputs(c)["mask"]
        assert m.ndim == 4 and m.shape == tuple(1 if dim in c.bcast else n for dim, n in zip("zhq", (c.z, c.qh, c.qn))) + (c.kn,), c.id
        vis = U.visibility(c)
        if "q" not in c.bcast:
            assert (vis.sum(-1) == 0).any(), c.id                       # a dead row
        if c.kn > 32:
            assert not vis[:, :, :32, 32:64].any() and vis[:, :, :32, :32].any(), c.id  # a hidden (query block, key block) pair next to a live one
        assert vis.any(-1).any()
    assert any(c.mask and "z" in c.bcast and c.z > 1 for c in cs) and any(c.mask and "h" in c.bcast and c.qh > 1 for c in cs)
    assert {c.layout for c in cs} == {None, "tm", "vpitch", "dotm"}
    n = U.NEED_CASE
    assert n.causal and n.mask and n.ratio > 1 and n.z > 1 and len(U.NEED_SUBSETS) == 6
    had = [c for c in cs if c.group]
    assert {c.d for c in had} == {40, 80} and all(c.group == 32 and c.gdt == "f32" for c in had)
    for c in cs:  # class channels below the head dim, Q and K on disjoint halves
        mp = U._census_maps(c)
        assert mp["qch"].max() < c.d // 2 <= mp["kch"].min() and mp["kch"].max() < c.d and mp["och"].max() < c.d, c.id
        assert len(np.unique(mp["L"][0, 0, :32])) == min(4, c.qn)    # lse varies inside a query block


@pytest.mark.parametrize("cid", IDS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_census_closed_form_equals_restatement(cid, variant):
    """Family A is exact: the restatement lands on the closed-form counts with error 0 (1e-3 count through the float32 rotation), the counts are exact in
    the gradient dtype (so a bf16 store loses nothing), and the parameterised block loop agrees."""
    c = U.CASES[cid]
    x = U.census_inputs(c, variant)
    ref = U.census_closed_form(c, variant)
    # count: exactly 0.  delta: blocks of weight 1 and 2 meet in one sum and 127 * (2 sm / 127) is not 2 sm to the last bit
    tol = 1e-3 if c.group else (1e-6 if variant == "delta" else 0.0)
    for got in (U.restated(x), U.block_loop(x)):
        assert max(U.census_errors(c, got, variant)) <= tol, (cid, U.census_errors(c, got, variant))
    if not c.group:
        for r, unit in zip(ref[:3], (U.SM_SCALE, U.SM_SCALE, 1.0)):
            t = torch.from_numpy(r * unit)
            assert torch.equal(t.to(U.TDT[c.gdt]).double(), t) and np.abs(r).max() <= 256, cid
    if variant == "delta":
        w = U._census_maps(c)["w_delta"]
        assert set(np.unique(w)) <= {-2, -1, 1, 2} and (c.qn < 3 or len(np.unique(w[0, 0, :32])) > 1)


@pytest.mark.parametrize("cid", B_IDS)
def test_planted_keys_dominate_and_cover(cid):
    c = U.CASES[cid]
    x = U.planted_inputs(c)
    pos, live = x["pos"], x["live"]
    assert x["min_gap_nat"] >= U.GAP_NAT, (cid, x["min_gap_nat"])
    assert pos.min() >= 0 and pos.max() < c.kn
    if c.qn <= c.kn:
        assert all(len(set(pos[h])) == c.qn for h in range(c.qh)), cid   # injective
    if c.mask is None:
        assert live.all()
        if c.causal:
            assert (pos[:, :min(c.qn, c.kn)] == np.arange(min(c.qn, c.kn))).all()   # the diagonal
        elif c.qn >= 2:
            assert 0 in pos and c.kn - 1 in pos                            # key 0, the last valid key (of the tail block)
    assert torch.equal(x["qq"][0, 0, 0], x["kc"][0, 0, pos[0, 0]])


def test_planted_keys_cover_every_in_block_position():
    """Over the table: planted keys on all 32 in-block positions of at least two key blocks, planted queries on all 32 in-block positions and in a
    tail query block, for both padded head dims; the diagonal under causal; key 0 and KN - 1."""
    for dp in (64, 128):
        blocks, qpos, tailq = {}, set(), False
        for c in U.CASES.values():
            if "B" not in c.families or c.dp != dp:
                continue
            x = U.planted_inputs(c)
            for h in range(c.qh):
                for q in np.nonzero(x["live"][0, h])[0]:
                    blocks.setdefault((c.id, h, x["pos"][h, q] // 32), set()).add(x["pos"][h, q] % 32)
                    qpos.add(q % 32)
                    tailq |= c.qn % 32 != 0 and q >= c.qn // 32 * 32
        assert sum(len(v) == 32 for v in blocks.values()) >= 2 and qpos == set(range(32)) and tailq, dp


# ---- CPU: a correct implementation keeps to the tiers ----------------------------------------------------------------------------------------------
CAP_SHAPES = [dict(z=2, qh=4, kh=2, qn=72, kn=97, d=40), dict(z=1, qh=3, kh=1, qn=129, kn=70, d=128)]


@pytest.mark.parametrize("shape", CAP_SHAPES, ids=lambda s: f"{s['qh']}x{s['qn']}x{s['kn']}x{s['d']}")
@pytest.mark.parametrize("tag, gdt, causal", [("bf16", "bf16", False), ("f16", "f16", True), ("bf16", "f32", False)])
def test_reference_alone_keeps_to_the_tiers(shape, tag, gdt, causal):
    """The restatement against itself with P moved by up to 2 ulp and dP accumulated in float64: nothing outside the loose tier, under 1 % of a
    tensor outside the tight tier (half the cap the GPU test holds the kernel to).  The unperturbed block loop is the restatement itself."""
    x = U.random_operands(**shape, tag=tag, gdt=gdt, causal=causal, seed=11)
    ref = U.restated(x)
    r = U.reference64(x)
    for name, a, b, p in zip(("dq", "dk", "dv"), ref, U.block_loop(x), U.block_loop(x, perturb=5)):
        tight, loose = U.budgets(r, name, a, arith=False)
        assert U.tier_report(b, a, tight, loose)[0] <= 0.001, name
        share, worst = U.assert_tiers(p, a, tight, loose, name, cap=0.01)
        print(f"CAP {tag}/{gdt} {name} share={share:.4f} worst={worst:.3f}")
        # and the float64 reference of family B sits within its budget of the float32 restatement
        t64, l64 = U.budgets(r, name, U.finish64(r, name), arith=True)
        U.assert_tiers(a, U.finish64(r, name), t64, l64, name + " (float64 reference)")


# ---- CPU: the checks are sharp ------------------------------------------------------------------------------------------------------------------
def _find(**kw):
    return next(c for c in U.CASES.values() if all(getattr(c, k) == v for k, v in kw.items()))


def _census_miss(c, mut, variant="count"):
    """Worst census error, in counts, of the mutated block loop."""
    return max(U.census_errors(c, U.block_loop(U.census_inputs(c, variant), mut=mut), variant))


def _planted_miss(c, mut):
    """Worst error of the mutated block loop against the float64 reference, as a fraction of the loose budget."""
    x = U.planted_inputs(c)
    r = U.reference64(x)
    worst = 0.0
    for name, got in zip(("dq", "dk", "dv"), U.block_loop(x, mut=mut)):
        ref = U.finish64(r, name)
        worst = max(worst, U.tier_report(got, ref, *U.budgets(r, name, ref, arith=True))[1])
    return worst


MUTANT_CASES = {
    "drop_qblock": dict(mask=None, causal=False, layout=None, z=2, qh=4, kh=2),
    "causal_start": dict(causal=True, mask=None, qn=72, kn=97),
    "diag_hidden": dict(causal=True, mask=None, qn=72, kn=97),
    "tail_keys": dict(mask=None, causal=False, layout=None, z=2, qh=4, kh=2),
    "clamped_rows": dict(mask=None, causal=False, layout=None, z=2, qh=4, kh=2),
    "mask_batch": dict(mask="bool", bcast="", layout=None),
    "mask_head": dict(mask="bool", bcast="", layout=None),
    "delta_row": dict(mask=None, causal=False, layout=None, z=2, qh=4, kh=2),
    "swap_keys": dict(mask=None, causal=False, layout=None, z=2, qh=4, kh=2),
    "kvhead_mod": dict(mask=None, causal=False, layout=None, z=2, qh=4, kh=2),
}


@pytest.mark.parametrize("mut", list(U.MUTANTS))
def test_mutants_are_caught_by_the_family_that_claims_them(mut):
    """Every mutant misses the check of the family named in MUTANTS by at least 4 times its bound; the family named blind passes it."""
    what, catcher, blind = U.MUTANTS[mut]
    c = _find(**MUTANT_CASES[mut])
    assert "B" in c.families
    miss = {"A": lambda: _census_miss(c, mut) / U.QUARTER, "A-delta": lambda: _census_miss(c, mut, "delta") / U.QUARTER, "B": lambda: _planted_miss(c, mut)}
    assert miss[catcher]() >= 4.0, (what, catcher, miss[catcher]())
    if blind is not None:
        assert miss[blind]() <= 1.0, (what, blind, miss[blind]())
    if mut == "swap_keys":  # blind in both census variants: every dS of a block is equal up to sign and the sign pattern is per query
        assert _census_miss(c, mut, "delta") <= U.QUARTER
    if mut in ("diag_hidden", "delta_row", "drop_qblock"):  # the planted keys see these too
        assert _planted_miss(c, mut) >= 4.0, what


def test_unmutated_loop_passes_both_families():
    c = _find(**MUTANT_CASES["swap_keys"])
    assert _census_miss(c, None) == 0.0 and _census_miss(c, None, "delta") <= 1e-6 and _planted_miss(c, None) <= 1.0


@pytest.mark.parametrize("cid", [c.id for c in U.CASES.values() if "B" in c.families and c.mask is None and not c.layout and c.kn >= 33 and c.qn >= 31])
def test_planted_checks_are_sharp(cid):
    """Swapping the V rows or the K code rows of two planted keys of one block, or hiding the planted key, moves the rows concerned by at least 10
    times their loose budget; a key no query planted gets dk and dv within the budget of zero."""
    c = U.CASES[cid]
    x = U.planted_inputs(c)
    r = U.reference64(x)
    pos, h = x["pos"], 0
    kv = U.kv_head(h, c.qh, c.kh)
    # two queries on neighbouring keys of one block: of all such pairs the one whose V rows differ most as seen by its dO rows
    best = None
    for q in range(c.qn - 1):
        a, b = int(pos[h, q]), int(pos[h, q + 1])
        if a // 32 == b // 32 and a != b:
            dvv = (x["v"][:, kv, a] - x["v"][:, kv, b]).double()
            score = min(float((x["do"][:, h, qq].to(x["v"].dtype).double() * dvv).sum(-1).abs().min()) for qq in (q, q + 1))
            if best is None or score > best[0]:
                best = (score, q, q + 1, a, b)
    _, qa, qb, ka, kb = best

    def moved(r2, name, head, rows):
        ref = U.finish64(r, name)
        loose = U.budgets(r, name, ref, arith=True)[1]
        return float(torch.nan_to_num((U.finish64(r2, name) - ref).abs() / loose, nan=float("inf"))[:, head][:, rows].amax(-1).min())

    for key in ("v", "kc"):
        t = x[key].clone()
        t[:, kv, [ka, kb]] = t[:, kv, [kb, ka]]
        r2 = U.reference64({**x, key: t})
        assert moved(r2, "dq", h, [qa, qb]) >= 10, (cid, key, "dq")
        assert moved(r2, "dk", kv, [ka, kb]) >= 10, (cid, key, "dk")   # (dv = P^T.dO does not read V; it moves with the K rows)
        if key == "kc":
            assert moved(r2, "dv", kv, [ka, kb]) >= 10, (cid, key, "dv")
    hide = torch.zeros(c.z, c.qh, c.qn, c.kn, dtype=torch.bool)
    hide[:, h, qa, ka] = True
    r2 = U.reference64(x, hide=hide)
    assert moved(r2, "dq", h, [qa]) >= 10 and moved(r2, "dk", kv, [ka]) >= 10 and moved(r2, "dv", kv, [ka]) >= 10, cid
    unplanted = sorted(set(range(c.kn)) - {int(k) for hh in range(c.qh) if U.kv_head(hh, c.qh, c.kh) == kv for k in pos[hh]})
    if unplanted:
        for name in ("dk", "dv"):
            ref = U.finish64(r, name)
            tight, loose = U.budgets(r, name, torch.zeros_like(ref), arith=True)
            leak = math.exp(-U.GAP_NAT) * c.qn * c.ratio * float(ref.abs().max())  # every pair off the planted ones carries P <= e^-15
            assert (ref[:, kv][:, unplanted].abs() <= loose[:, kv][:, unplanted] + leak).all(), (cid, name)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
def _dev(x, dev):
    """The operands on the device as atten_bwd / atten_lse take them, in the case's layout."""
    from sdnq_amd import attention as A
    c = x.get("case")
    layout = c.layout if c is not None else None
    t = {k: x[k].to(dev) for k in ("qq", "qs", "ks", "v", "do", "out", "lse")}
    kn, knp = x["v"].shape[2], (x["v"].shape[2] + 31) // 32 * 32
    kc = torch.zeros(*x["kc"].shape[:2], knp, x["kc"].shape[3], dtype=torch.int8)
    kc[:, :, :x["kc"].shape[2]] = x["kc"]
    t["kq"] = U.pack_k_fragments(kc).to(dev)
    if t["ks"].shape[2] != knp:
        t["ks"] = torch.nn.functional.pad(t["ks"], (0, knp - kn), value=1.0)
    t["mask"] = A.prepare_mask(x["raw_mask"].to(dev), x["qq"].shape[2], kn) if x["raw_mask"] is not None else None
    if layout == "vpitch":
        t["v"] = torch.cat([t["v"], torch.zeros_like(t["v"])], -1)[..., :t["v"].shape[-1]]
        assert t["v"].stride(2) == 2 * t["v"].shape[-1]
    if layout == "dotm":
        t["do"], t["out"] = (a.transpose(1, 2).contiguous().transpose(1, 2) for a in (t["do"], t["out"]))
    return t


def _bwd(x, dev, need=(True, True, True)):
    from sdnq_amd import attention as A
    t = _dev(x, dev)
    c = x.get("case")
    tm = c is not None and c.layout == "tm"
    got = A.atten_bwd(t["do"], t["out"], t["lse"], t["qq"], t["qs"], t["kq"], t["ks"], t["v"], x["sm"], x["causal"], t["mask"], x["group"], need=need,
                      token_major=tm)
    if tm and got[0] is not None and c.qh > 1 and c.qn > 1:
        assert got[0].stride(2) > got[0].stride(1)
    for g, ref_like in zip(got, (x["do"], x["v"], x["v"])):
        assert g is None or (g.dtype == x["do"].dtype and g.shape == ref_like.shape)
    return tuple(g.cpu() if g is not None else None for g in got)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_hip_backward_census(cid, variant, gpu_device):
    """Family A: every gradient element counted exactly its visible queries / keys, to a quarter of one item."""
    c = U.CASES[cid]
    got = _bwd(U.census_inputs(c, variant), gpu_device)
    err = U.census_errors(c, got, variant)
    print(f"CENSUS inst={c.instance} gdt={c.gdt} variant={variant} dq={err[0]:.3e} dk={err[1]:.3e} dv={err[2]:.3e} case={cid}")
    U.assert_census(c, got, variant, f"{cid} ({variant})")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_hip_lse_census(cid, gpu_device):
    """attn_lse_kernel on the census operands: 2^lse is the visible-key count of the row; a row the mask leaves without keys gets exactly 0."""
    from sdnq_amd import attention as A
    c = U.CASES[cid]
    x = U.census_inputs(c)
    t = _dev(x, gpu_device)
    lse = A.atten_lse(t["qq"], t["qs"], t["kq"], t["ks"], c.kn, x["sm"], c.causal, torch.float32, t["mask"], head_dim=c.d).cpu().double().numpy()
    n = U.census_closed_form(c)[3]
    assert lse.shape == n.shape
    err = np.abs(np.exp2(lse) - np.maximum(n, 1))
    print(f"LSE inst={c.instance} keys={err.max():.3e} case={cid}")
    assert (err <= U.QUARTER).all(), (cid, float(err.max()))
    assert (lse[n == 0] == 0).all(), cid


@pytest.mark.gpu
@pytest.mark.parametrize("cid", B_IDS)
def test_hip_backward_planted_keys(cid, gpu_device):
    """Family B: one dominant key per query on every in-block position, per element against the float64 restatement."""
    c = U.CASES[cid]
    x = U.planted_inputs(c)
    r = U.reference64(x)
    got = _bwd(x, gpu_device)
    fails = []
    for name, g in zip(("dq", "dk", "dv"), got):
        ref = U.finish64(r, name)
        tight, loose = U.budgets(r, name, ref, arith=True)
        share, worst = U.tier_report(g, ref, tight, loose)
        print(f"PLANTED inst={c.instance} gdt={c.gdt} {name} worst={worst:.3e} share={share:.5f} case={cid}")
        try:
            U.assert_tiers(g, ref, tight, loose, f"{cid} {name}")
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["A", "B"])
def test_hip_backward_need_subsets_bit_identical(family, gpu_device):
    """atten_bwd called directly with every `need` subset on the masked, causal, grouped-heads case: the parts computed equal the full run bit for bit."""
    x = U.census_inputs(U.NEED_CASE, "delta") if family == "A" else U.planted_inputs(U.NEED_CASE)
    full = _bwd(x, gpu_device)
    for need in U.NEED_SUBSETS:
        part = _bwd(x, gpu_device, need=need)
        for n, f, p in zip(need, full, part):
            assert (p is not None) == n
            if n:
                assert torch.equal(f.view(torch.int16), p.view(torch.int16)), (need, family)


# family C: tests/test_attention_backward_gpu.py's sweep shapes (four of them once more with a float32 gradient, one per kernel instance) and the fixtures
def _random_cases():
    from tests.test_attention_backward_gpu import SWEEP
    from tests.test_attention_backward_host import abwd_names
    out = [(f"sweep{i}", None) for i in range(len(SWEEP))] + [(f"sweep{i}", "f32") for i in (0, 1, 2, 4)]
    return out + [(n, None) for n in abwd_names()]


@pytest.mark.gpu
@pytest.mark.parametrize("name, gdt", _random_cases(), ids=lambda v: str(v))
def test_hip_backward_random_per_element(name, gdt, gpu_device):
    """Family C: the HIP gradients against the restatement on the HIP forward's saved tensors, element by element."""
    from sdnq_amd import attention as A
    from tests.test_attention_backward_gpu import SWEEP, _inputs
    from tests.test_attention_backward_host import load
    if name.startswith("sweep"):
        case = SWEEP[int(name[5:])]
        g = torch.Generator().manual_seed(7)
        q = torch.randn(case["z"], case["qh"], case["qn"], case["d"], generator=g).to(case["dtype"]).to(gpu_device)
        k = (torch.randn(case["z"], case["kh"], case["kn"], case["d"], generator=g) + 2.0).to(case["dtype"]).to(gpu_device)
        v = torch.randn(case["z"], case["kh"], case["kn"], case["d"], generator=g).to(case["dtype"]).to(gpu_device)
        do = torch.randn(case["z"], case["qh"], case["qn"], case["d"], generator=g).to(case["dtype"]).to(gpu_device)
        kw, mask = case["kw"], None
    else:
        meta, t = load(name)
        q, k, v, do, mask = _inputs(meta, t, torch.bfloat16 if meta["dtype"] == "bf16" else torch.float16)
        kw = meta["kwargs"]
    gd = torch.float32 if gdt == "f32" else q.dtype
    d, kn = q.shape[-1], k.shape[2]
    group = 0
    if kw.get("use_hadamard"):
        from sdnq_amd.quant_utils import get_hadamard_group_size
        dp = 64 if d <= 64 else 128
        ok, group = get_hadamard_group_size(dp, min(kw.get("hadamard_group_size", 256), dp))
        group = group if ok else 0
    sm, causal = kw.get("scale") or d ** -0.5, kw.get("is_causal", False)
    m = A.prepare_mask(mask, q.shape[2], kn) if mask is not None else None
    qq, qs, kq, ks, vt = A.quantize_attn(q, k, v, smooth_k=kw.get("smooth_k", True), hadamard_group=group)
    out = A.atten_fwd(qq, qs, kq, ks, vt, kn, sm, causal, gd, m, head_dim=d)
    lse = A.atten_lse(qq, qs, kq, ks, kn, sm, causal, gd, m, head_dim=d)
    got = A.atten_bwd(do.to(gd), out, lse, qq, qs, kq, ks, v, sm, causal, m, group)
    x = dict(qq=qq.cpu().view(torch.int8), qs=qs.cpu(), kc=A.unpack_k_fragments(kq).cpu().view(torch.int8), ks=ks.cpu(), v=v.cpu(), do=do.to(gd).cpu(),
             out=out.cpu(), lse=lse.cpu(), sm=sm, causal=causal, mask=m.cpu() if m is not None else None, group=group)
    refs = U.restated(x)
    r = U.reference64(x)
    fails = []
    for nm, g, ref in zip(("dq", "dk", "dv"), got, refs):
        tight, loose = U.budgets(r, nm, ref.double(), arith=False)
        share, worst = U.tier_report(g.cpu(), ref, tight, loose)
        print(f"RANDOM inst={'bf16' if q.dtype == torch.bfloat16 else 'f16'}/{64 if d <= 64 else 128} gdt={gd} {nm} worst={worst:.3e} share={share:.5f} case={name}")
        try:
            U.assert_tiers(g.cpu(), ref, tight, loose, f"{name} {nm}")
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_pack_matches_the_prepare_kernel(gpu_device):
    """`pack_k_fragments` of the codes quantize_attn produced is its k_q, byte for byte (key tail and padded head dim included)."""
    from sdnq_amd import attention as A
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(2, 2, 70, 40, generator=g).to(torch.float16).to(gpu_device) for _ in range(3))
    kq = A.quantize_attn(q, k, v)[2]
    assert kq.shape == (2, 2, 3, 2, 64, 16)
    assert torch.equal(U.pack_k_fragments(A.unpack_k_fragments(kq).cpu()).view(torch.int8), kq.cpu().view(torch.int8))
