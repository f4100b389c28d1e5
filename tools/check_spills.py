#!/usr/bin/env python3
"""Fail when any kernel of the built library uses scratch memory (register spills or a stack): reads the AMDGPU metadata notes of
sdnq_amd/libsdnq_hip.so (every embedded gfx950 code object) with llvm-readelf and checks `.private_segment_fixed_size` and
`.vgpr_spill_count` / `.sgpr_spill_count` of every kernel.  Run by __graft_entry__.build().   usage: tools/check_spills.py [lib] [-v]
Also the one place that takes a built library apart (code_objects, disassemble): tools/disasm_kernel.py and
tools/compare_kernels.py import it from here."""
import contextlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
# the integer notes of a kernel record that anybody here reads
NOTES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
         "sgpr_spill_count", "kernarg_segment_size")


@contextlib.contextmanager
def code_objects(lib):
    """Paths of the gfx950 code objects (ELF files) embedded in the fat binary `lib`, in a temporary directory that lives as long
    as the `with` block."""
    with tempfile.TemporaryDirectory() as tmp:
        # the device code objects sit in the .hip_fatbin section as a clang offload bundle
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        data = open(fat, "rb").read()
        # every embedded ELF starts with \x7fELF; cut them out (the bundle header holds offsets, but scanning is enough here)
        starts = [m.start() for m in re.finditer(b"\x7fELF", data)]
        paths = []
        for n, st in enumerate(starts):
            paths.append(os.path.join(tmp, f"co{n}.elf"))
            open(paths[-1], "wb").write(data[st:starts[n + 1] if n + 1 < len(starts) else len(data)])
        yield paths


def disassemble(co):
    """The text of `llvm-objdump -d --no-show-raw-insn` of one code object."""
    return subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout


def kernel_resources(lib):
    """[{"symbol": kernel descriptor symbol, <every note of NOTES>: int}] of every kernel in the fat binary `lib`."""
    out = []
    with code_objects(lib) as cos:
        for co in cos:
            r = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True)
            if r.returncode != 0:
                continue
            cur = {}
            for line in r.stdout.splitlines():
                m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)", line)
                if not m:
                    continue
                k, v = m.group(1), m.group(2).strip()
                if k == "symbol":
                    cur[k] = v
                elif k in NOTES:
                    cur[k] = int(v)
                if k == "wavefront_size":  # last key of a kernel record
                    if "symbol" in cur:
                        out.append({**dict.fromkeys(NOTES, 0), **cur})
                    cur = {}
    return out


def waterfall_loops(lib):
    """Number of readfirstlane "waterfall" loops in front of memory instructions, over the whole library: a buffer descriptor (or any
    scalar operand of a memory instruction) that the compiler could not keep in SGPRs is fed through `v_readfirstlane ... v_cmp_eq ...
    s_and_saveexec ... <memory instruction> ... s_cbranch_execnz`.  Every descriptor of this library is wave-uniform by construction, so
    the expected count is 0 (round 3: 6-24 such loops per GEMM kernel, the K loop's LDS-DMAs included, went unnoticed for a while)."""
    pattern = r"v_readfirstlane_b32[^\n]*\n(?:[^\n]*\n){0,6}?[^\n]*v_cmp_eq_u64[^\n]*\n(?:[^\n]*\n){0,4}?[^\n]*s_and_saveexec_b64"
    with code_objects(lib) as cos:
        return sum(len(re.findall(pattern, disassemble(co))) for co in cos)


def main():
    lib = next((a for a in sys.argv[1:] if not a.startswith("-")), os.path.join(ROOT, "sdnq_amd", "libsdnq_hip.so"))
    res = kernel_resources(lib)
    if not res:
        print("no kernels found in", lib)
        return 2
    # SGPR spills go to VGPR lanes (no scratch memory): reported with -v only
    bad = [r for r in res if r["private_segment_fixed_size"] > 0 or r["vgpr_spill_count"] > 0]
    sg = [r for r in res if r["sgpr_spill_count"] > 0 and r not in bad]
    if "-v" in sys.argv:
        for r in sorted(res, key=lambda r: -r["vgpr_count"])[:25]:
            print(f"{r['vgpr_count']:4d} vgprs  scratch {r['private_segment_fixed_size']:5d}  {r['symbol'][:150]}")
    print(f"{len(res)} kernels, {len(bad)} with scratch memory / vector-register spills ({len(sg)} more keep spilled SGPRs in VGPR lanes)")
    for r in bad:
        print(f"  scratch {r['private_segment_fixed_size']} B, vgpr spills {r['vgpr_spill_count']}, sgpr spills {r['sgpr_spill_count']}: {r['symbol'][:200]}")
    if "--waterfalls" in sys.argv:
        wf = waterfall_loops(lib)
        print(f"{wf} readfirstlane waterfall loops in front of memory instructions")
        if wf:
            return 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
