#!/usr/bin/env python3
"""Development aid: disassemble the kernels of sdnq_amd/libsdnq_hip.so whose (mangled) name contains every given substring.
usage: tools/disasm_kernel.py <substr> [<substr> ...] [--count]   (--count: instruction histogram instead of the listing)"""
import os, re, sys, collections
from check_spills import ROOT, code_objects, disassemble
lib = os.environ.get("SDNQ_HIP_LIB") or os.path.join(ROOT, "sdnq_amd", "libsdnq_hip.so")
subs = [a for a in sys.argv[1:] if not a.startswith("--")]
count = "--count" in sys.argv
with code_objects(lib) as cos:
    for co in cos:
        cur, keep, hist = None, False, collections.Counter()
        for line in disassemble(co).splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                if keep and count:
                    print(cur); [print(f"  {k:40s} {v}") for k, v in hist.most_common(40)]
                cur, hist = m.group(1), collections.Counter()
                keep = all(s in cur for s in subs)
                if keep and not count:
                    print(line)
                continue
            if keep:
                if count:
                    t = line.split()
                    if t: hist[t[0]] += 1
                else:
                    print(line)
        if keep and count:
            print(cur); [print(f"  {k:40s} {v}") for k, v in hist.most_common(40)]
