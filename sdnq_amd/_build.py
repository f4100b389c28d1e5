"""The build recipe of the C-ABI library ``libsdnq_hip.so`` and its two host modules -- the only one.  hipcc cross-compiles for gfx950
(MI355X) without a GPU.

Content-addressed: every object is keyed on the SHA-256 of its source, every header and its compiler flags, the library on the hashes of
its units (written next to it as ``<lib>.srchash``), so what is loaded can be checked against what is in the tree (``source_hash()``),
independent of file times.  Standard library only and no relative imports: ``import sdnq_amd`` loads torch and the built modules, which
a build must not need, so this also runs as a script:

    python sdnq_amd/_build.py [--force]                                                  the product: sdnq_amd/libsdnq_hip.so
    python sdnq_amd/_build.py --define SDNQ_TRACE --out build/libsdnq_hip_trace.so       a lab variant (tools/trace_gemm.py)

A variant compiles every unit with the product's flags plus its ``-D`` defines into an object directory of its own, so it never
overwrites the product's objects; a library outside ``sdnq_amd/`` gets no ``_binding.so`` / ``_fastpath.so`` next to it.
Environment: HIPCC, SDNQ_OBJ_DIR, SDNQ_EXTRA_FLAGS, SDNQ_FP_CONTRACT, SDNQ_PRELOAD_ROWQUANT, SDNQ_PRELOAD_GEMM, SDNQ_SKIP_FASTPATH, MAX_JOBS.
"""
import argparse
import hashlib
import importlib.util
import os
import shlex
import subprocess
import sys
import sysconfig
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libsdnq_hip.so")
_API_H = os.path.join(HERE, "..", "include", "sdnq_hip.h")
# clang derives the __hip_cuid_* symbol of an object from the spelling of its source and output paths: this spelling of the object
# directory is part of what makes two builds of the same tree byte-identical
_OBJ = CSRC + "/../../build/obj"

_PRELOAD = "-mllvm -amdgpu-kernarg-preload-count=14"
# The units in link order, which is also their order in the source hash: (name of csrc/<name>.hip, extra flags, environment switch
# that leaves the extra flags out when it is 0).
UNITS = (
    ("api", "", None),
    # rowquant.hip: kernarg preload -- the first 14 argument dwords of the row quantizer (everything its row loads need) arrive in
    # SGPRs with the wave, so the loads go out without a scalar round trip first; the other arguments are fetched behind them
    ("rowquant", "-DSDNQ_PRELOAD_ROWQUANT " + _PRELOAD, "SDNQ_PRELOAD_ROWQUANT"),
    # gemm.hip: the same for the GEMM kernel's 14 leading scalar arguments (tile mapping, operand descriptors, prologue DMAs)
    ("gemm", "-DSDNQ_PRELOAD_GEMM " + _PRELOAD, "SDNQ_PRELOAD_GEMM"),
    # the other kernels with scalar arguments get theirs preloaded as well: the GEMM variants, the weight-side units (dequant.hip's
    # dequantizers and re-quantizers, skinny.hip's few-row linears, linear_float.hip's linear_float and lowrank_down), conv_pixel_amax,
    # the adapter kernels of lowrank_train.hip, ...
    ("gemm_aq", _PRELOAD, None),
    ("gemm_ks", _PRELOAD, None),
    ("gemm_w4", _PRELOAD, None),
    ("dequant", _PRELOAD, None),
    ("skinny", _PRELOAD, None),
    ("linear_float", _PRELOAD, None),
    ("quantize", "", None),
    ("conv", _PRELOAD, None),
    ("convt", "", None),
    ("dequant_t", "", None),
    ("lowrank_train", _PRELOAD, None),
    # the conv adapters' implicit GEMMs take their geometry as one by-value struct: no preload
    ("conv_lowrank", "", None),
    # DoRA's norm kernel takes the weight descriptor as one by-value struct, as dequant_t does: no preload
    ("dora", "", None),
    # the merge kernel takes two descriptors and the pack table by value, as quantize does: no preload
    ("merge", "", None),
    # attention.hip, attention_var.hip (the forward kernels): keep the MFMA accumulators in VGPRs (the softmax rescales / reads them
    # with VALU every block; in AGPR form the compiler moved 80 registers per 32-key block through v_accvgpr_read/write)
    ("attention", "-mllvm -amdgpu-mfma-vgpr-form", None),
    ("attention_var", "-mllvm -amdgpu-mfma-vgpr-form", None),
    ("attention_bwd", "", None),
    ("colquant", "", None),
    ("optim", "", None),
    ("parallel", "", None),
)


def _sha(*parts: bytes) -> str:
    return hashlib.sha256(b"".join(parts)).hexdigest()


def _read(path: str) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def _flags(defines) -> str:
    """The flags of every unit, as the one string that is hashed.  -ffp-contract=off: a*b+c is fused ONLY where the source says fmaf --
    the reference's roundings are part of the contract (round 4: the configuration fuzzer found epilogue terms the compiler had fused
    into one rounding where torch rounds twice; small fixtures hid it)."""
    return (os.environ.get("SDNQ_EXTRA_FLAGS", "") + " --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract="
            + (os.environ.get("SDNQ_FP_CONTRACT") or "off") + " -Wno-unused-command-line-argument" + "".join(" -D" + d for d in defines))


def _units(flags: str):
    """[(name, extra flags, hash)] of every unit, in link order."""
    hdr = _sha(*(_read(os.path.join(CSRC, f)) for f in sorted(os.listdir(CSRC)) if f.endswith(".h")), _read(_API_H))
    out = []
    for name, extra, switch in UNITS:
        if switch and (os.environ.get(switch) or "1") == "0":
            extra = ""
        out.append((name, extra, _sha(f"{hdr} {flags} {extra}\n".encode(), _read(os.path.join(CSRC, name + ".hip")))))
    return out


def _fastpath_hash() -> str:
    return _sha(_read(os.path.join(CSRC, "fastpath.cpp")), _read(_API_H))


def source_hash(extra_defines=()) -> str:
    """SHA-256 over every HIP source, header and compiler flag and the two host modules' sources: a library built here from the
    tree as it is now has exactly this in its ``.srchash``."""
    parts = "".join(f" {name}:{h}" for name, _, h in _units(_flags(extra_defines)))
    parts += " binding:" + _sha(_read(os.path.join(CSRC, "binding.c"))) + " fastpath:" + _fastpath_hash()
    return _sha((parts + "\n").encode())


def host_modules(out: str):
    """The Python extension modules a build of `out` leaves next to it: none for a library outside the package."""
    if os.path.dirname(os.path.abspath(out)) != HERE:
        return []
    return [os.path.join(HERE, "_binding.so")] + ([] if os.environ.get("SDNQ_SKIP_FASTPATH") == "1" else [os.path.join(HERE, "_fastpath.so")])


def _recorded(product: str, hash_file: str, h: str) -> bool:
    """`product` exists and was built from inputs with hash `h`."""
    try:
        return os.path.isfile(product) and _read(hash_file).decode().strip() == h
    except OSError:
        return False


def _compile(jobs) -> None:
    """Run [(unit, argv, hash file, hash)] up to MAX_JOBS at once, recording the hash of every object that compiled; raise naming
    every unit that failed, with the compiler's stderr."""
    def run(job):
        name, argv, hash_file, h = job
        r = subprocess.run(argv, capture_output=True, text=True)
        sys.stderr.write(r.stdout + r.stderr)
        if r.returncode == 0:
            with open(hash_file, "w") as f:
                f.write(h + "\n")
        return name, r
    workers = int(os.environ.get("MAX_JOBS") or min(16, os.cpu_count() or 1))
    with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
        failed = [(name, r) for name, r in pool.map(run, jobs) if r.returncode != 0]
    if failed:
        raise RuntimeError("".join(f"compiling {name}.hip failed (exit {r.returncode}):\n{r.stderr}\n" for name, r in failed))


def build(out: str = LIB, force: bool = False, obj_dir=None, defines=(), dry_run: bool = False):
    """Build `out` and its host modules (see host_modules) and write ``<out>.srchash``; `force` recompiles every unit.  Objects go to
    `obj_dir`, else SDNQ_OBJ_DIR, else build/obj -- with ``-<defines>`` appended for a variant.  Returns `out`; with `dry_run` the
    argv of every command the build would run instead, running nothing and writing nothing."""
    defines = tuple(defines)
    if obj_dir is None:
        obj_dir = (os.environ.get("SDNQ_OBJ_DIR") or _OBJ) + "".join("-" + d for d in defines)
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    flags = _flags(defines)
    units = _units(flags)
    compiles = []
    for name, extra, h in units:
        obj, hash_file = f"{obj_dir}/{name}.o", f"{obj_dir}/{name}.hash"
        if force or not _recorded(obj, hash_file, h):
            compiles.append((name, [hipcc] + flags.split() + extra.split() + ["-c", f"{CSRC}/{name}.hip", "-o", obj], hash_file, h))
    cmds = [job[1] for job in compiles]
    cmds.append([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wno-unused-command-line-argument", "-o", out]
                + [f"{obj_dir}/{name}.o" for name, *_ in units])
    modules = host_modules(out)
    pyinc = sysconfig.get_paths()["include"]
    if modules:
        # typed CPython binding of the hot entry points (host C; calls the library's named symbols, see binding.c)
        cmds.append(["gcc", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + pyinc, os.path.join(CSRC, "binding.c"),
                     "-o", modules[0], "-ldl"])
    fp_hash, fp_hash_file = _fastpath_hash(), f"{obj_dir}/fastpath.hash"
    build_fp = len(modules) > 1 and (force or not _recorded(modules[1], fp_hash_file, fp_hash))
    if build_fp:
        # host-side fast path of the eager Linear forward (C++ against torch's headers: tensor checks, allocation and the launches of a
        # plain w8a8 layer in ONE call, see fastpath.cpp); torch is located, not imported
        ti = os.path.dirname(importlib.util.find_spec("torch").origin)
        cmds.append(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__=1",
                     "-DUSE_ROCM=1", "-D_GLIBCXX_USE_CXX11_ABI=1", f"-I{ti}/include", f"-I{ti}/include/torch/csrc/api/include",
                     "-I/opt/rocm/include", "-I" + pyinc, os.path.join(CSRC, "fastpath.cpp"), "-o", modules[1],
                     f"-L{ti}/lib", "-lc10", "-lc10_hip", "-ltorch", "-ltorch_cpu", "-ltorch_hip", "-ltorch_python", "-ldl",
                     f"-Wl,-rpath,{ti}/lib"])
    if dry_run:
        return cmds
    os.makedirs(obj_dir, exist_ok=True)
    _compile(compiles)
    for argv in cmds[len(compiles):]:
        subprocess.run(argv, check=True)
    if build_fp:
        with open(fp_hash_file, "w") as f:
            f.write(fp_hash + "\n")
    srchash = source_hash(defines)
    with open(out + ".srchash", "w") as f:
        f.write(srchash + "\n")
    print(f"built {out} ({srchash[:12]})")
    return out


def main(argv=None) -> None:
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--out", default=LIB, help="the library to build (default: sdnq_amd/libsdnq_hip.so)")
    p.add_argument("--define", action="append", default=[], metavar="NAME[=VALUE]", help="compile every unit with -DNAME[=VALUE]")
    p.add_argument("--obj-dir", help="object directory (default: build/obj, with -<defines> appended for a variant)")
    p.add_argument("--force", action="store_true", help="recompile every unit")
    p.add_argument("--dry-run", action="store_true", help="print the commands instead of running them")
    a = p.parse_args(argv)
    r = build(a.out, force=a.force, obj_dir=a.obj_dir, defines=a.define, dry_run=a.dry_run)
    if a.dry_run:
        print("\n".join(shlex.join(c) for c in r))


if __name__ == "__main__":
    main()
