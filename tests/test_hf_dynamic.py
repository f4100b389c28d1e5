"""Dynamic quantization through the transformers plugin.  tests/golden/checkpoint_hf_dyn_tiny was written by the REFERENCE's plugin with
`use_dynamic_quantization=True` (make_golden_hf_dynamic.py): its config carries the option and a mixed `modules_dtype_dict`.  It loads
through THIS build's plugin without searching again, and `from_pretrained(..., quantization_config=SDNQConfig(use_dynamic_quantization=True))`
runs the search.  Fresh interpreters, as in test_hf_plugin.py: the Auto* tables are process-global."""
import json
import os

import pytest

from tests.test_hf_plugin import run_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "checkpoint_hf_dyn_tiny")


def test_from_dict_accepts_the_reference_config():
    """The stored quantization_config (use_dynamic_quantization: true, mixed modules_dtype_dict) builds a config, through the plain
    class and the plugin's QuantizationConfigMixin form, and keeps every key."""
    qc = json.load(open(os.path.join(CKPT, "config.json")))["quantization_config"]
    assert qc["use_dynamic_quantization"] is True and len(qc["modules_dtype_dict"]) >= 2
    out = run_py(f"""
import json
import sdnq, sdnq_amd
qc = json.load(open({CKPT + '/config.json'!r}))['quantization_config']
for cls in (sdnq_amd.SDNQConfig, sdnq.SDNQConfig):
    c = cls.from_dict(dict(qc))
    assert c.use_dynamic_quantization is True and c.dynamic_loss_threshold == qc['dynamic_loss_threshold']
    assert c.modules_dtype_dict == qc['modules_dtype_dict'] and c.weights_dtype == qc['weights_dtype']
print('ok')
""")
    assert out.strip().splitlines()[-1] == "ok"


def test_from_pretrained_builds_the_mixed_dtypes_without_searching():
    """CPU: every stored layer gets the dtype the reference chose (modules_dtype_dict), its tensors bit for bit, and no search runs."""
    out = run_py(f"""
import json, torch, transformers, sdnq, sdnq_amd
from safetensors.torch import load_file
import sdnq_amd.quantizer as Q
def no_search(*a, **k):
    raise AssertionError('a stored checkpoint was searched again')
Q.sdnq_quantize_layer_weight_dynamic = no_search
qc = json.load(open({CKPT + '/config.json'!r}))['quantization_config']
want = {{n[:-len('.weight')]: d for d, names in qc['modules_dtype_dict'].items() for n in names}}
m = transformers.AutoModelForCausalLM.from_pretrained({CKPT!r}, dtype=torch.float32)
got = {{n: mod.sdnq_dequantizer.weights_dtype for n, mod in m.named_modules() if hasattr(mod, 'sdnq_dequantizer')}}
assert got == want, (got, want)
sd = load_file({CKPT + '/model.safetensors'!r})
for n in got:
    mod = m.get_submodule(n)
    for k in ('weight', 'scale'):
        a, b = sd[n + '.' + k], getattr(mod, k)
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), (n, k)
print('ok', len(got), sorted(set(got.values())))
""")
    assert out.strip().splitlines()[-1].startswith("ok")


def test_from_pretrained_with_dynamic_config_searches(tmp_path):
    """CPU: `from_pretrained(..., quantization_config=sdnq.SDNQConfig(use_dynamic_quantization=True))` quantizes every layer with the
    search: the choices land in modules_dtype_dict, the layers carry them, and save_pretrained / from_pretrained round-trips them."""
    out = run_py(f"""
import torch, transformers, sdnq
torch.manual_seed(3)
cfg = transformers.LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4,
                               vocab_size=128, max_position_embeddings=64, tie_word_embeddings=False)
m = transformers.LlamaForCausalLM(cfg)
with torch.no_grad():
    for n, p in m.named_parameters():
        if p.dim() == 2:
            w = torch.randn_like(p) * 0.08
            p.copy_(w / (torch.rand_like(p) + 0.05) * 0.1 if 'mlp' in n else w)
m.save_pretrained({str(tmp_path / 'float')!r})
q = sdnq.SDNQConfig(weights_dtype='int4', use_dynamic_quantization=True, dynamic_loss_threshold=3e-3, minimum_allowed_numel=4096,
                    modules_to_not_convert=['lm_head'])
qm = transformers.AutoModelForCausalLM.from_pretrained({str(tmp_path / 'float')!r}, quantization_config=q, dtype=torch.float32)
chosen = {{n: mod.sdnq_dequantizer.weights_dtype for n, mod in qm.named_modules() if hasattr(mod, 'sdnq_dequantizer')}}
assert len(chosen) == 7 and len(set(chosen.values())) >= 2, chosen
listed = {{n[:-len('.weight')]: d for d, names in qm.quantization_config.modules_dtype_dict.items() for n in names}}
assert listed == chosen, (listed, chosen)
qm.save_pretrained({str(tmp_path / 'q')!r})
back = transformers.AutoModelForCausalLM.from_pretrained({str(tmp_path / 'q')!r}, dtype=torch.float32)
again = {{n: mod.sdnq_dequantizer.weights_dtype for n, mod in back.named_modules() if hasattr(mod, 'sdnq_dequantizer')}}
assert again == chosen, (again, chosen)
print('ok', sorted(set(chosen.values())))
""")
    assert out.strip().splitlines()[-1].startswith("ok")


@pytest.mark.gpu
def test_loaded_model_reproduces_the_reference_logits_on_the_gpu():
    """The reference-written mixed-dtype checkpoint on the GPU (every Linear on the HIP matmuls) gives the logits the REFERENCE computed
    from it on the CPU (io.npz), at test_hf_plugin.py's bound: relative L2 <= 2e-4."""
    out = run_py(f"""
import numpy as np, torch, transformers, sdnq, sdnq_amd
io = np.load({CKPT + '/io.npz'!r})
m = transformers.AutoModelForCausalLM.from_pretrained({CKPT!r}, dtype=torch.float32, device_map='cuda:0')
mods = [mod for mod in m.modules() if hasattr(mod, 'sdnq_dequantizer')]
n_hip = sum(1 for mod in mods if getattr(mod.forward_func, '__module__', '').startswith('sdnq_amd'))
assert n_hip == len(mods) == len(io['sdnq_layers']), (n_hip, len(mods))
assert len({{mod.sdnq_dequantizer.weights_dtype for mod in mods}}) >= 2
with torch.no_grad():
    y = m(input_ids=torch.from_numpy(io['input_ids']).cuda()).logits.float().cpu().numpy()
ref = io['logits']
rel = float(np.linalg.norm(y - ref) / np.linalg.norm(ref))
assert rel <= 2e-4, rel
print('ok', rel)
""")
    assert out.strip().splitlines()[-1].startswith("ok")
