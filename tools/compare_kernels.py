#!/usr/bin/env python3
"""Compare the kernels of two builds of the library: the proof a kernel refactor wants ("the generated code did not change").
For every kernel symbol of either build: the resource notes (VGPRs, AGPRs, SGPRs, LDS, scratch, spills, kernarg bytes) and whether
the instruction listings are equal.  The listings are `llvm-objdump -d --no-show-raw-insn` without what only says WHERE the code
lies: the address / encoding comments, the resolved branch targets (the relative offsets stay), the literals of
pc-relative address computations (s_getpc_b64 and the add pair behind it) and the `...` objdump prints for the zero padding between
one function's end and the next one's aligned start (it depends on which function the linker placed behind).

usage: tools/compare_kernels.py <parent lib> <branch lib> [--diff <substr>]
One line per kernel: name, resources, `same` | `differs (<+/- instructions>)` | `resources differ` | `only in ...`; then totals.
--diff prints a unified diff of the listings of the kernels whose name contains <substr>.
Exit status: 0 every kernel same, 1 listings differ, 2 kernel sets or resources differ."""
import difflib
import re
import sys

from check_spills import NOTES, code_objects, disassemble, kernel_resources

SHORT = dict(zip(NOTES, ("vgpr", "agpr", "sgpr", "lds", "scratch", "vgpr_spill", "sgpr_spill", "kernarg")))


def listings(lib):
    """{kernel symbol: [normalized instruction lines]} of every function in the code objects of `lib`."""
    out = {}
    with code_objects(lib) as cos:
        for co in cos:
            cur, pcrel = None, 0
            for line in disassemble(co).splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = out.setdefault(m.group(1), [])
                    continue
                ins = line.split("//")[0].strip()
                if cur is None or not ins or ins == "...":
                    continue
                if pcrel and re.match(r"s_addc?_u32 ", ins):
                    ins = re.sub(r"(0x[0-9a-f]+|\d+)$", "<pcrel>", ins)
                pcrel = 2 if ins.startswith("s_getpc_b64") else max(0, pcrel - 1)
                cur.append(ins)
    return out


def main():
    args = sys.argv[1:]
    show = None
    if "--diff" in args[:-1]:
        i = args.index("--diff")
        show = args[i + 1]
        del args[i:i + 2]
    if len(args) != 2:
        print(__doc__)
        return 2
    res = [{r["symbol"].removesuffix(".kd"): r for r in kernel_resources(lib)} for lib in args]
    lst = [listings(lib) for lib in args]
    same = differs = bad = 0
    for name in sorted(set(res[0]) | set(res[1])):
        if name not in res[0] or name not in res[1]:
            print(f"{name}  only in the {'branch' if name in res[1] else 'parent'} build")
            bad += 1
            continue
        notes = " ".join(f"{SHORT[k]}={res[0][name][k]}" for k in NOTES)
        if any(res[0][name][k] != res[1][name][k] for k in NOTES):
            print(f"{name}  {notes}  resources differ: " + " ".join(f"{SHORT[k]}={res[1][name][k]}" for k in NOTES if res[0][name][k] != res[1][name][k]))
            bad += 1
            continue
        a, b = lst[0].get(name, []), lst[1].get(name, [])
        if a == b:
            same += 1
            print(f"{name}  {notes}  same")
        else:
            differs += 1
            print(f"{name}  {notes}  differs ({len(b) - len(a):+d} instructions: {len(a)} -> {len(b)})")
        if show is not None and show in name:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(a, b, "parent", "branch", lineterm=""))
    print(f"{same + differs + bad} kernels: {same} same, {differs} with a different listing, {bad} with different resources or in one build only")
    return 2 if bad else (1 if differs else 0)


if __name__ == "__main__":
    sys.exit(main())
