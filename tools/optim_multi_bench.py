#!/usr/bin/env python3
"""``AdamW.step()`` (sdnq_amd.optim) on parameter sets of MANY tensors, where one launch per tensor is all launch and host cost, with the
multi-tensor step (csrc/optim.hip: one launch per table of tensors) against one launch per parameter.  Sets, bf16 and float32, dense
state and -- where the shapes allow it -- uint8 state:

  adapters   rank-16 adapters A [16, K] and B [N, 16] for every Linear of the SDXL step bench.py models (sdnq_amd.shapes): 1482 tensors.
             uint8 state: the A matrices (their last dimension is a multiple of 32) in a group of their own, the B matrices dense
  biases     one bias [N] per such layer: 741 tensors (1-D: dense state only)
  big4       the four tensors of tools/optim_bench.py: [640, 640], [5120, 640], [3072, 12288], [16384, 5120]
  mixed      adapters and big4 together

Contenders, each a process of its own (another tree's package cannot be imported beside this one's), run in alternation `--passes` times:
  parent     the package of the tree given by --parent (a checkout of the parent commit with its library built): one launch per parameter
  batched    this tree
  single     this tree with SDNQ_HIP_OPTIM_MULTI=0: the cross-check of `parent`
and, in the first `batched` process only, torch.optim.AdamW(fused=True) and (foreach=True) on the same sets for context (another
arithmetic: no condition).

Measures: "eager_ms", the wall time of an eager ``opt.step()`` in the default (stochastic) configuration with a synchronize after it,
host included; "graph_us", the device time of one replay of a captured deterministic ``opt.step()`` between two events.  After
`--warmup` steps, `--rounds` windows per process; the figure is the median over all windows of all passes, "spread" is (max - min) /
median of the baseline's windows, the run-to-run spread of the machine.  Exit status 1 if `batched` is slower than the baseline
(`parent`, or `single` without --parent) by more than that spread on any set in either measure.  One JSON line per (set, dtype, state).
Usage: python tools/optim_multi_bench.py [--parent DIR] [--out profiles/optim_multi_bench.jsonl] [--passes 2] [--rounds 7] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG4 = [(640, 640), (5120, 640), (3072, 12288), (16384, 5120)]
RANK = 16


def parameter_sets(shapes):
    """{set: [(shape, may have uint8 state)]} from the layer list of `shapes` (the measured tree's sdnq_amd.shapes)."""
    layers = [(k, n) for (_, _, k, n, _, _) in shapes.sdxl_unet_layer_sequence()]
    adapters = [s for k, n in layers for s in (((RANK, k), True), ((n, RANK), False))]
    big4 = [(s, True) for s in BIG4]
    return dict(adapters=adapters, biases=[((n,), False) for _, n in layers], big4=big4, mixed=adapters + big4)


def configurations(shapes):
    for name, shapes_ in parameter_sets(shapes).items():
        for dtype in ("bfloat16", "float32"):
            for state in ("dense", "uint8"):
                if state == "uint8" and not any(q for _, q in shapes_):
                    continue
                yield name, dtype, state, shapes_


# ---- one contender: a process of its own -----------------------------------------------------------------------------------------------------
def measure(a):
    sys.path.insert(0, a.root)
    import torch
    from sdnq_amd import optim, shapes
    assert os.path.dirname(os.path.dirname(os.path.abspath(optim.__file__))) == os.path.abspath(a.root), optim.__file__
    dev = torch.device("cuda:0")

    def make(shapes_, dtype, state, factory, **kw):
        g = torch.Generator(device=dev).manual_seed(5)
        groups = {False: [], True: []}
        for shape, may in shapes_:
            p = torch.nn.Parameter((torch.randn(shape, device=dev, generator=g) * 0.5).to(dtype))
            p.grad = (torch.randn(shape, device=dev, generator=g) * 0.3).to(dtype)
            groups[state == "uint8" and may].append(p)
        if factory is not None:
            return factory(groups[False] + groups[True])
        spec = [dict(params=ps, use_quantized_buffers=q, quantized_buffers_minimum_numel=512) for q, ps in groups.items() if ps]
        return optim.AdamW(spec, lr=1e-4, **kw)

    def eager(opt):
        out = []
        for i in range(a.warmup + a.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            opt.step()
            torch.cuda.synchronize()
            if i >= a.warmup:
                out.append((time.perf_counter() - t0) * 1e3)
        return out

    def graph(opt):
        opt.step()  # creates the state
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            opt.step()
        out = []
        for i in range(a.warmup + a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                out.append(e0.elapsed_time(e1) * 1e3)
        return out

    for name, dtype, state, shapes_ in configurations(shapes):
        dt = getattr(torch, dtype)
        line = dict(set=name, dtype=dtype, state=state, tensors=len(shapes_), elements=sum(torch.Size(s).numel() for s, _ in shapes_))
        line["eager_ms"] = eager(make(shapes_, dt, state, None))
        line["graph_us"] = graph(make(shapes_, dt, state, None, use_stochastic_rounding=False, use_stochastic_buffers=False))
        if a.torch_context and state == "dense":
            for key, kw in (("torch_fused", dict(fused=True)), ("torch_foreach", dict(foreach=True))):
                line[key + "_eager_ms"] = eager(make(shapes_, dt, state, lambda ps: torch.optim.AdamW(ps, lr=1e-4, **kw)))
                line[key + "_graph_us"] = graph(make(shapes_, dt, state, lambda ps: torch.optim.AdamW(ps, lr=1e-4, capturable=True, **kw)))
        print("LINE " + json.dumps(line), flush=True)
        torch.cuda.empty_cache()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------
def contender(root, multi, a, torch_context):
    env = dict(os.environ, SDNQ_HIP_OPTIM_MULTI="1" if multi else "0")
    argv = [sys.executable, os.path.abspath(__file__), "--measure", "--root", root, "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
    r = subprocess.run(argv + (["--torch-context"] if torch_context else []), env=env, capture_output=True, text=True,
                       timeout=a.process_timeout)
    if r.returncode != 0:
        sys.exit(f"measuring {root} failed (exit {r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return [json.loads(ln[5:]) for ln in r.stdout.splitlines() if ln.startswith("LINE ")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", help="a checkout of the parent commit with its library built: the baseline")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_multi_bench.jsonl"))
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--process-timeout", type=int, default=300, help="seconds for one contender's process")
    ap.add_argument("--measure", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--torch-context", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.measure:
        return measure(a)
    contenders = ([("parent", os.path.abspath(a.parent), True)] if a.parent else []) + [("batched", ROOT, True), ("single", ROOT, False)]
    base = contenders[0][0] if a.parent else "single"
    windows = {}  # (set, dtype, state) -> {field: [windows]}
    for p in range(a.passes):
        for label, root, multi in contenders:
            lines = contender(root, multi, a, torch_context=label == "batched" and p == 0)
            print(f"pass {p + 1} of {a.passes}: {label} measured {len(lines)} configurations", file=sys.stderr, flush=True)
            for line in lines:
                key = (line["set"], line["dtype"], line["state"])
                slot = windows.setdefault(key, dict(tensors=line["tensors"], elements=line["elements"]))
                for field, value in line.items():
                    if isinstance(value, list):
                        slot.setdefault(f"{label}_{field}" if not field.startswith("torch_") else field, []).extend(value)
    import torch
    lost = []
    with open(a.out, "w") as f:
        for (name, dtype, state), w in windows.items():
            line = dict(bench="adamw_multi", set=name, dtype=dtype, state=state, tensors=w["tensors"], elements=w["elements"],
                        baseline=base, passes=a.passes, rounds=a.rounds, device=torch.cuda.get_device_name(0))
            for field, values in w.items():
                if isinstance(values, list):
                    line[field] = round(statistics.median(values), 3)
                    line[field.rsplit("_", 1)[0] + "_min_" + field.rsplit("_", 1)[1]] = round(min(values), 3)
            for measure_ in ("eager_ms", "graph_us"):
                b = w[f"{base}_{measure_}"]
                spread = (max(b) - min(b)) / statistics.median(b)
                line[f"{measure_.split('_')[0]}_spread"] = round(spread, 4)
                line[f"{base}_over_batched_{measure_.split('_')[0]}"] = round(line[f"{base}_{measure_}"] / line[f"batched_{measure_}"], 3)
                if line[f"batched_{measure_}"] > line[f"{base}_{measure_}"] * (1 + spread):
                    lost.append(f"{name} {dtype} {state} {measure_}")
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")
    if lost:
        sys.exit(f"the batched step is slower than `{base}` beyond the run-to-run spread at: " + ", ".join(lost))


if __name__ == "__main__":
    main()
