"""Lab of the one-launch w8a8 Linear (csrc/gemm_aq.hip) against the two-launch route: graph-replayed pairs on cold / warm operands and the
phase stamps of the fused kernel.  usage: python tools/aq_lab.py [--forms 0,1] [MxNxK ...] | --grouped [MxGxNxK ...]
--forms: the forms of the 32 x 256 tile to run one after the other (sdnq_internal_aq_direct: 0 the LDS ring, 1 the direct form on the
slab copy of the weight; default: -1, whatever the library ships).  Every fused call is handed the slab copy; the ring form ignores it."""
import ctypes
import sys

import torch

sys.path.insert(0, ".")
from sdnq_amd import _lib, ops  # noqa: E402

dev = torch.device("cuda:0")
lib = _lib.load()
args = sys.argv[1:]
forms = [-1]
if "--forms" in args:
    i = args.index("--forms")
    forms = [int(v) for v in args[i + 1].split(",")]
    del args[i:i + 2]
aq_direct = getattr(ctypes.CDLL(_lib.LIB_PATH), "_Z23sdnq_internal_aq_directi")
aq_direct.argtypes, aq_direct.restype = [ctypes.c_int], None
shapes = [tuple(int(v) for v in a.split("x")) for a in args if "--grouped" not in args] or [(1024, 1280, 1280), (1024, 1280, 640), (4096, 640, 640), (1024, 640, 1280), (2048, 1280, 1280), (1024, 3840, 1280)]


def timed(fn, pool, reps=5):
    """`pool` launches in ONE graph (each on its own operands), replayed `reps` times: us per launch."""
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for i in range(len(pool)):
            fn(i)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for i in range(len(pool)):
                fn(i)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / len(pool))
    return best


def phases(run):
    """Mean phase stamps of the one-launch kernel over the workgroups of the launch `run` makes (memtime ticks)."""
    buf = torch.zeros(1024 * 8, dtype=torch.int64, device=dev)
    aq_trace = getattr(ctypes.CDLL(_lib.LIB_PATH), "_Z22sdnq_internal_aq_tracePy")
    aq_trace.argtypes = [ctypes.c_void_p]
    aq_trace.restype = None
    aq_trace(buf.data_ptr())
    for _ in range(3):
        buf.zero_()
        run()
        torch.cuda.synchronize()
    aq_trace(None)
    t = buf.view(1024, 8).cpu()
    t = t[t[:, 0] > 0]
    d = (t[:, 1:7] - t[:, 0:6]).double()
    names = ["entry->issued", "issued->quantized", "K loop", "drain+sync", "epilogue math", "stores"]
    print("   phases (memtime ticks, mean over", t.shape[0], "workgroups):", ", ".join(f"{nm} {v:.0f}" for nm, v in zip(names, d.mean(0).tolist())),
          "| total", f"{(t[:, 6] - t[:, 0]).double().mean():.0f}", flush=True)


if "--grouped" in args:
    # the linked q / k / v problem, M x (G x N) x K: the grouped one-launch form (sdnq_hip_linear_w8a8_fused_grouped: the 32 x 256 tile,
    # two per CU) against ops.rowquant + ops.scaled_mm_grouped.
    # usage: python tools/aq_lab.py --grouped [MxGxNxK ...]
    args.remove("--grouped")
    for m, g, n, k in ([tuple(int(v) for v in a.split("x")) for a in args] or [(1024, 3, 1280, 1280)]):
        for pool_n, tag in ((1, "re-read"), (24, "distinct operands")):
            xs_ = [torch.randn(m, k, device=dev).to(torch.bfloat16) for _ in range(pool_n)]
            ws = [[torch.randint(-128, 128, (n, k), dtype=torch.int8, device=dev) for _ in range(g)] for _ in range(pool_n)]
            sb = torch.rand(n, device=dev) * 0.02 + 1e-4
            bias = torch.randn(n, device=dev).to(torch.bfloat16)
            groups = [ops.GemmGroup([(w, sb, bias) for w in wl]) for wl in ws]
            members = [[(ops.aq_slab_pack(w), sb, bias) for w in wl] for wl in ws]
            idx = list(range(max(pool_n, 32)))

            def two_launches(i):
                xq, xs, _, _ = ops.rowquant(xs_[i % pool_n], ops.MM_I8)
                return ops.scaled_mm_grouped(ops.MM_I8, xq, xs, groups[i % pool_n], torch.bfloat16)

            two = timed(two_launches, idx)
            one = timed(lambda i: ops.linear_w8a8_fused_grouped(ops.MM_I8, xs_[i % pool_n], members[i % pool_n], torch.bfloat16), idx)
            print(f"{m}x({g}x{n})x{k} {tag:18s}: rowquant + grouped GEMM {two:7.2f} us | one grouped launch {one:7.2f} us", flush=True)
        a, b = two_launches(0), ops.linear_w8a8_fused_grouped(ops.MM_I8, xs_[0], members[0], torch.bfloat16)
        torch.cuda.synchronize()
        print("   same bits:", all(torch.equal(u.view(torch.int16), v.view(torch.int16)) for u, v in zip(a, b)), flush=True)
        phases(lambda: ops.linear_w8a8_fused_grouped(ops.MM_I8, xs_[0], members[0], torch.bfloat16))
    sys.exit(0)

for (m, n, k), form in ((sh, f) for sh in shapes for f in forms):
    aq_direct(form)
    if len(forms) > 1:
        print(f"-- form {form}", flush=True)
    for pool_n, tag in ((1, "re-read"), (64, "distinct operands")):
        xs_ = [torch.randn(m, k, device=dev).to(torch.bfloat16) for _ in range(pool_n)]
        bs = [torch.randint(-128, 128, (n, k), dtype=torch.int8, device=dev) for _ in range(pool_n)]
        slabs = [ops.aq_slab_pack(w) if ops.aq_slab_bytes(n, k) else None for w in bs]
        sb = torch.rand(n, device=dev) * 0.02 + 1e-4
        bias = torch.randn(n, device=dev).to(torch.bfloat16)
        reps = max(pool_n, 32)
        idx = list(range(reps))
        two = timed(lambda i: ops.linear_w8a8(ops.MM_I8, xs_[i % pool_n], bs[i % pool_n], sb, bias, torch.bfloat16), idx)
        sup = lib.sdnq_hip_linear_w8a8_fused_supported(0, 1, 1, m, n, k)
        try:
            one = timed(lambda i: ops.linear_w8a8_fused(ops.MM_I8, xs_[i % pool_n], bs[i % pool_n], sb, bias, torch.bfloat16, slabs[i % pool_n]), idx)
        except Exception as e:  # noqa: BLE001
            one = float("nan")
            print("  fused route refused:", e)
        print(f"{m}x{n}x{k} {tag:18s}: two launches {two:7.2f} us | one launch {one:7.2f} us   (supported() = {sup})", flush=True)
    # phase stamps (shader clock, 100 MHz memtime ticks -> reported in ticks): entry, loads+ring issued, quantized, K loop done, synced, staged, stored
    # (the 32 x 256 tile drains its first two weight stages before "quantized", and its "K loop" has no barrier: thread 0's own loop)
    try:
        x = torch.randn(m, k, device=dev).to(torch.bfloat16)
        b = torch.randint(-128, 128, (n, k), dtype=torch.int8, device=dev)
        slab = ops.aq_slab_pack(b) if ops.aq_slab_bytes(n, k) else None
        phases(lambda: ops.linear_w8a8_fused(ops.MM_I8, x, b, sb, bias, torch.bfloat16, slab))
    except Exception as e:  # noqa: BLE001
        print("   trace failed:", e)
