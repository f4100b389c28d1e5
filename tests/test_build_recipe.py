"""The build recipe of libsdnq_hip.so (sdnq_amd/_build.py), checked through its dry run: no compiler runs here."""
import os
import subprocess
import sys

import pytest

from sdnq_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("HIPCC", "SDNQ_OBJ_DIR", "SDNQ_EXTRA_FLAGS", "SDNQ_FP_CONTRACT", "SDNQ_PRELOAD_ROWQUANT", "SDNQ_PRELOAD_GEMM", "SDNQ_SKIP_FASTPATH")


@pytest.fixture(autouse=True)
def _product_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _compiles(cmds):
    return [c for c in cmds if "-c" in c]


def test_every_hip_source_is_one_unit():
    names = [u[0] for u in _build.UNITS]
    hips = sorted(f[:-4] for f in os.listdir(_build.CSRC) if f.endswith(".hip"))
    assert sorted(names) == hips and len(set(names)) == len(names)


def test_every_compile_targets_gfx950_without_fp_contraction():
    cmds = _build.build(force=True, dry_run=True)
    compiles = _compiles(cmds)
    assert [c[c.index("-c") + 1] for c in compiles] == [f"{_build.CSRC}/{u[0]}.hip" for u in _build.UNITS]
    for c in compiles:
        assert "--offload-arch=gfx950" in c and "-ffp-contract=off" in c, c
    link = cmds[len(compiles)]
    assert link[link.index("-o") + 1] == _build.LIB and link[-len(_build.UNITS):] == [
        c[c.index("-o") + 1] for c in compiles]
    assert [c[0] for c in cmds[len(compiles) + 1:]] == ["gcc", "g++"]


def test_variant_is_the_product_plus_its_defines(tmp_path):
    out = str(tmp_path / "libsdnq_hip_trace.so")
    product = _compiles(_build.build(force=True, dry_run=True))
    variant = _build.build(out, force=True, defines=["SDNQ_TRACE"], dry_run=True)
    assert all(c[0] not in ("gcc", "g++") for c in variant)  # no host modules next to a library outside the package
    variant = _compiles(variant)
    assert len(variant) == len(product)
    obj_dirs = set()
    for p, v in zip(product, variant):
        assert v.count("-DSDNQ_TRACE") == 1
        v = [a for a in v if a != "-DSDNQ_TRACE"]
        i = p.index("-o") + 1
        assert v[:i] == p[:i] and len(v) == len(p) and os.path.basename(v[i]) == os.path.basename(p[i])
        obj_dirs.add((os.path.dirname(p[i]), os.path.dirname(v[i])))
    (prod_dir, var_dir), = obj_dirs
    assert os.path.normpath(prod_dir) != os.path.normpath(var_dir)
    assert _build.source_hash(("SDNQ_TRACE",)) != _build.source_hash()


def test_skip_fastpath_leaves_the_module_out(monkeypatch):
    cmds = _build.build(force=True, dry_run=True)
    assert any(c[0] == "g++" for c in cmds)
    monkeypatch.setenv("SDNQ_SKIP_FASTPATH", "1")
    assert not any(c[0] == "g++" for c in _build.build(force=True, dry_run=True))


def test_lib_source_hash_is_the_recipes():
    assert _lib.source_hash() == _build.source_hash()


def test_lib_is_current_without_fastpath_when_skipped(tmp_path, monkeypatch):
    """A tree that never had _fastpath.so: with SDNQ_SKIP_FASTPATH=1 the library built there is current."""
    lib = tmp_path / "libsdnq_hip.so"
    for f in (lib, tmp_path / "_binding.so"):
        f.write_bytes(b"")
    (tmp_path / "libsdnq_hip.so.srchash").write_text(_build.source_hash() + "\n")
    monkeypatch.setattr(_build, "HERE", str(tmp_path))
    monkeypatch.setattr(_lib, "LIB_PATH", str(lib))
    assert not _lib.lib_is_current()
    monkeypatch.setenv("SDNQ_SKIP_FASTPATH", "1")
    assert _lib.lib_is_current()


def test_failed_unit_raises_with_its_name_and_stderr(tmp_path, monkeypatch):
    hipcc = tmp_path / "hipcc"
    hipcc.write_text("#!/bin/sh\ncase \"$*\" in *gemm_w4.hip*) echo 'gemm_w4: error: boom' >&2; exit 1;; esac\n")
    hipcc.chmod(0o755)
    monkeypatch.setenv("HIPCC", str(hipcc))
    with pytest.raises(RuntimeError, match=r"(?s)compiling gemm_w4\.hip failed.*gemm_w4: error: boom") as e:
        _build.build(str(tmp_path / "lib.so"), obj_dir=str(tmp_path / "obj"))
    assert "compiling api.hip" not in str(e.value)
    assert sorted(os.listdir(tmp_path / "obj")) == sorted(f"{u[0]}.hash" for u in _build.UNITS if u[0] != "gemm_w4")


def test_runs_as_a_script_without_torch():
    code = ("import sys; sys.path.insert(0, 'sdnq_amd'); import _build; "
            "cmds = _build.build(force=True, dry_run=True, defines=['SDNQ_TRACE']); "
            "assert 'torch' not in sys.modules and all('-DSDNQ_TRACE' in c for c in cmds if '-c' in c)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    r = subprocess.run([sys.executable, os.path.join("sdnq_amd", "_build.py"), "--dry-run", "--force", "--out", "build/x.so"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == len(_build.UNITS) + 1, r.stdout + r.stderr
