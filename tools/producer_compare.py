#!/usr/bin/env python3
"""The fused producers (sdnq_amd.norms, sdnq_amd.activations) of this tree against those of another checkout, alternating in one call.

Per round and per tree, each in a process of its own: tools/normquant_bench.py and tools/actquant_bench.py at their own shapes, and the
host time of ``SDNQFusedNorm.forward`` / ``SDNQFusedActivation.forward`` on a [2, 64, 512] bf16 input, where the host dominates (host
clock around 2000 calls ending in a synchronise, median of 9 repeats; "seeding": the codes are written and parked, "y_only": the state
after ``linear.UNSHARED_AFTER`` unused steps).  Per case: every round's median of both trees, the median of those, the parent's
spread (max - min of ITS medians) and ``passes``: this tree's median <= the parent's median + the parent's spread.

Usage: python tools/producer_compare.py --parent <checkout with its library built> [--rounds 3] [--out profiles/producer_refactor_bench.jsonl]
                                        [--tag key=value ...]     (tags are copied into every record: what was compared)
The first process that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"norm_rowquant": ("norm", "m", "k"), "norm_block": ("m", "k"), "act_rowquant": ("case", "m", "n"), "wrapper_host": ("case", "mode")}
METRICS = {"norm_rowquant": ("fused_us", "fused_noy_us"), "norm_block": ("fused_us",), "act_rowquant": ("fused_us", "fused_noy_us"), "wrapper_host": ("us",)}


def wrapper_host(root, out, calls=2000, repeats=9):
    """Child process: the wrappers of the package under `root`."""
    sys.path.insert(0, root)
    import torch

    import sdnq_amd
    from sdnq_amd import linear
    from sdnq_amd.activations import SDNQFusedActivation
    from sdnq_amd.norms import SDNQFusedNorm
    assert os.path.samefile(os.path.dirname(os.path.dirname(sdnq_amd.__file__)), root), sdnq_amd.__file__
    dev = torch.device("cuda:0")

    class GEGLU(torch.nn.Module):  # the shape of diffusers' class
        def __init__(self, k, n):
            super().__init__()
            self.proj = torch.nn.Linear(k, 2 * n)

        def forward(self, x):
            h, gate = self.proj(x).chunk(2, dim=-1)
            return h * torch.nn.functional.gelu(gate)

    torch.manual_seed(0)
    x = torch.randn(2, 64, 512, device=dev, dtype=torch.bfloat16)
    scale, shift = (0.1 * torch.randn(2, 512, device=dev, dtype=torch.bfloat16) for _ in range(2))
    cases = {"norm_layer": (SDNQFusedNorm(torch.nn.LayerNorm(512).to(dev, torch.bfloat16)), (x,)),
             "norm_layer_adaln": (SDNQFusedNorm(torch.nn.LayerNorm(512, elementwise_affine=False).to(dev, torch.bfloat16)), (x, scale, shift)),
             "act_gelu_tanh": (SDNQFusedActivation(torch.nn.GELU(approximate="tanh")), (x,)),
             "act_geglu_proj": (SDNQFusedActivation(GEGLU(512, 512).to(dev, torch.bfloat16)), (x,))}
    with torch.no_grad(), open(out, "a") as f:
        for name, (mod, args) in cases.items():
            for mode, unshared in (("seeding", -(1 << 30)), ("y_only", 1 << 20)):
                mod.__dict__["_sdnq_unshared"] = unshared
                for _ in range(200):
                    mod(*args)
                torch.cuda.synchronize()
                assert bool(linear._ts.act_cache.entries) == (mode == "seeding"), (name, mode)
                times = []
                for _ in range(repeats):
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        mod(*args)
                    torch.cuda.synchronize()
                    times.append((time.perf_counter() - t0) / calls * 1e6)
                linear.clear_activation_cache()
                f.write(json.dumps(dict(bench="wrapper_host", case=name, mode=mode, us=round(statistics.median(times), 3))) + "\n")


def run(argv, cwd, limit=300):
    print("+", " ".join(argv), flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + argv, cwd=cwd, stdout=subprocess.DEVNULL)
    if r.returncode != 0:
        sys.exit(f"exit status {r.returncode}: stopping")


def collect(path):
    got = {}
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            for metric in METRICS[r["bench"]]:
                got.setdefault((r["bench"], tuple(r[k] for k in KEYS[r["bench"]]), metric), []).append(r[metric])
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "producer_refactor_bench.jsonl"))
    ap.add_argument("--tag", action="append", default=[])
    ap.add_argument("--wrapper-host", nargs=2, metavar=("ROOT", "OUT"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.wrapper_host:
        return wrapper_host(*a.wrapper_host)
    if not a.parent:
        ap.error("--parent is required")
    trees = {"parent": os.path.abspath(a.parent), "branch": ROOT}
    tmp = tempfile.mkdtemp(prefix="producer_compare_")
    raw = {b: os.path.join(tmp, b + ".jsonl") for b in trees}
    for _ in range(a.rounds):
        for build, root in trees.items():
            run([sys.executable, os.path.join(root, "tools", "normquant_bench.py"), "--out", raw[build]], root)
            run([sys.executable, os.path.join(root, "tools", "actquant_bench.py"), "--out", raw[build]], root)
            run([sys.executable, os.path.abspath(__file__), "--wrapper-host", root, raw[build]], root)
    parent, branch = collect(raw["parent"]), collect(raw["branch"])
    tags = dict(t.split("=", 1) for t in a.tag)
    failed = 0
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as f:
        for (bench, case, metric), pv in parent.items():
            bv = branch[bench, case, metric]
            pm, bm, spread = statistics.median(pv), statistics.median(bv), max(pv) - min(pv)
            rec = dict(bench=bench, **dict(zip(KEYS[bench], case)), metric=metric, **tags, alternations=a.rounds, parent_medians=pv,
                       branch_medians=bv, parent_us=round(pm, 3), branch_us=round(bm, 3), parent_spread_us=round(spread, 3),
                       passes=bm <= pm + spread)
            failed += not rec["passes"]
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)
    print(f"{len(parent)} cases, {failed} above the parent's median + spread")


if __name__ == "__main__":
    main()
