#!/usr/bin/env python3
"""Write a tiny transformers checkpoint quantized with DYNAMIC quantization by the REAL reference's transformers plugin
-> tests/golden/checkpoint_hf_dyn_tiny/.

Build container only; the pattern of make_golden_hf_embedding.py.  A 2-layer untied LlamaForCausalLM whose projections have different
weight spreads is loaded through `AutoModelForCausalLM.from_pretrained(..., quantization_config=sdnq.SDNQConfig(
use_dynamic_quantization=True, weights_dtype="int4", ...))`: the reference searches a dtype per layer while loading, so the saved
`quantization_config` carries `use_dynamic_quantization: true` and a `modules_dtype_dict` that lists several dtypes.  The re-loaded
model's logits on one batch are stored next to it (`io.npz`).

    python tests/golden/make_golden_hf_dynamic.py [out_dir]
    python tests/golden/make_golden_hf_dynamic.py --verify        # the reference re-loads the stored checkpoint: same logits bit for bit
    python tests/golden/make_golden_hf_dynamic.py --regen-check   # regenerate into a temp dir, compare with the tracked files
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402,F401  (environment switches of the reference, the stand-in `diffusers`, `import sdnq` = the reference)
import numpy as np  # noqa: E402
import torch  # noqa: E402

CKPT = os.path.join(HERE, "checkpoint_hf_dyn_tiny")


def _ids():
    return torch.randint(0, 128, (2, 24), generator=torch.Generator().manual_seed(7))


def write(out):
    import tempfile
    import transformers
    import sdnq
    assert "reference" in sdnq.__file__, sdnq.__file__
    torch.manual_seed(20261015)
    cfg = transformers.LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                                   vocab_size=128, max_position_embeddings=64, tie_word_embeddings=False)
    model = transformers.LlamaForCausalLM(cfg).to(torch.float32)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.dim() != 2:
                continue
            w = torch.randn(p.shape, generator=g) * 0.08
            if "mlp" in name:  # heavy tails: these layers need more bits than the attention projections
                w = w / (torch.rand(p.shape, generator=g) + 0.05) * 0.1
            p.copy_(w)
    with tempfile.TemporaryDirectory() as tmp:
        model.save_pretrained(tmp)
        qcfg = sdnq.SDNQConfig(weights_dtype="int4", use_dynamic_quantization=True, dynamic_loss_threshold=3e-3, use_quantized_matmul=True,
                               minimum_allowed_numel=4096, minimum_allowed_channel_size=32, modules_to_not_convert=["lm_head"])
        qmodel = transformers.AutoModelForCausalLM.from_pretrained(tmp, quantization_config=qcfg, dtype=torch.float32)
    os.makedirs(out, exist_ok=True)
    for f in os.listdir(out):
        os.remove(os.path.join(out, f))
    qmodel.save_pretrained(out)
    qc = json.load(open(os.path.join(out, "config.json")))["quantization_config"]
    assert qc["use_dynamic_quantization"] is True, qc
    assert len([k for k, v in qc["modules_dtype_dict"].items() if v]) >= 2, qc["modules_dtype_dict"]
    loaded = transformers.AutoModelForCausalLM.from_pretrained(out, dtype=torch.float32)
    ids = _ids()
    with torch.no_grad():
        logits = loaded(input_ids=ids).logits
        logits_q = qmodel(input_ids=ids).logits
    assert torch.equal(logits, logits_q), "the re-loaded model differs from the model that was saved"
    kinds = {n: m.sdnq_dequantizer.weights_dtype for n, m in loaded.named_modules() if hasattr(m, "sdnq_dequantizer")}
    np.savez_compressed(os.path.join(out, "io.npz"), input_ids=ids.numpy(), logits=logits.float().numpy(),
                        sdnq_layers=np.array(sorted(kinds), dtype=object).astype(str))
    print("wrote", out, sorted(os.listdir(out)), len(kinds), "SDNQ layers", sorted(set(kinds.values())))


def verify():
    import transformers
    loaded = transformers.AutoModelForCausalLM.from_pretrained(CKPT, dtype=torch.float32)
    io = np.load(os.path.join(CKPT, "io.npz"))
    with torch.no_grad():
        y = loaded(input_ids=torch.from_numpy(io["input_ids"])).logits.float().numpy()
    ok = np.array_equal(y, io["logits"])
    print("verify", "OK" if ok else "MISMATCH")
    return 0 if ok else 1


def regen_check():
    import tempfile
    tmp = tempfile.mkdtemp(prefix="sdnq_golden_hf_dyn_")
    write(tmp)
    bad = 0
    for fn in sorted(set(os.listdir(tmp)) | set(os.listdir(CKPT))):
        a, b = os.path.join(tmp, fn), os.path.join(CKPT, fn)
        if not (os.path.exists(a) and os.path.exists(b)):
            bad += 1
            print("regen-check", fn, "missing on one side")
            continue
        if fn.endswith(".npz"):
            za, zb = np.load(a), np.load(b)
            same = sorted(za.files) == sorted(zb.files) and all(
                za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes() for k in za.files)
        else:
            same = open(a, "rb").read() == open(b, "rb").read()
        bad += not same
        print("regen-check", fn, "identical" if same else "DIFFERS")
    print("regen-check done, differing files:", bad, "(temp dir", tmp + ")")
    return 1 if bad else 0


if __name__ == "__main__":
    if os.environ.get("PYTHONHASHSEED") != "0":
        # the reference collects its default skip keys in a set: the order of modules_to_not_convert in config.json follows the string
        # hash, so the files are only reproducible with a fixed hash seed (a fresh child interpreter; nothing has touched a GPU here)
        import subprocess
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env={**os.environ, "PYTHONHASHSEED": "0"}).returncode)
    if "--verify" in sys.argv[1:]:
        sys.exit(verify())
    if "--regen-check" in sys.argv[1:]:
        sys.exit(regen_check())
    write(sys.argv[1] if len(sys.argv) > 1 else CKPT)
