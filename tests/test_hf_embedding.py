"""A transformers checkpoint whose embedding the REFERENCE's plugin quantized (tests/golden/checkpoint_hf_emb_tiny, written by
make_golden_hf_embedding.py: `quant_embedding=True`, `add_skip_keys=False`, only `lm_head` kept in float, `model.embed_tokens` as uint4),
loaded by `AutoModelForCausalLM.from_pretrained` through THIS build's plugin and no reference.  Fresh interpreters, as in
test_hf_plugin.py: the Auto* tables are process-global."""
import os

import pytest

from tests.test_hf_plugin import run_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CKPT = os.path.join(ROOT, "tests", "golden", "checkpoint_hf_emb_tiny")


def test_from_pretrained_builds_the_quantized_embedding():
    """CPU: the skeleton conversion + tensor assignment.  The embedding becomes an SDNQEmbedding on this package's forward, with
    every stored tensor bit for bit and the record the reference's loader rebuilds; no float embedding is left behind."""
    out = run_py(f"""
import torch, transformers, sdnq, sdnq_amd
from safetensors.torch import load_file
from sdnq_amd.support import unsupported_reason
m = transformers.AutoModelForCausalLM.from_pretrained({CKPT!r}, dtype=torch.float32)
e = m.model.embed_tokens
assert type(e) is sdnq_amd.layers.SDNQEmbedding, type(e)
assert e.forward_func is sdnq_amd.embedding.quantized_embedding_forward and unsupported_reason(e) is None
dq = e.sdnq_dequantizer
assert dq.weights_dtype == 'uint4' and dq.layer_class_name == 'Embedding' and not dq.use_quantized_matmul, dq
sd = load_file({CKPT + '/model.safetensors'!r})
for k in ('weight', 'scale', 'zero_point'):
    want, got = sd['model.embed_tokens.' + k], getattr(e, k)
    assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), k
assert type(m.lm_head) is torch.nn.Linear
print('ok')
""")
    assert out.strip().splitlines()[-1] == "ok"


@pytest.mark.gpu
def test_loaded_model_reproduces_the_reference_logits_on_the_gpu():
    """The reference-written checkpoint on the GPU (the embedding on sdnq_hip_embedding, the Linears on the HIP matmuls) gives the logits
    the REFERENCE computed from it on the CPU (io.npz), at test_hf_plugin.py's bound: relative L2 <= 2e-4."""
    out = run_py(f"""
import numpy as np, torch, transformers, sdnq, sdnq_amd
io = np.load({CKPT + '/io.npz'!r})
m = transformers.AutoModelForCausalLM.from_pretrained({CKPT!r}, dtype=torch.float32, device_map='cuda:0')
n_hip = sum(1 for mod in m.modules() if hasattr(mod, 'sdnq_dequantizer') and getattr(mod.forward_func, '__module__', '').startswith('sdnq_amd'))
assert n_hip == 15, n_hip
assert m.model.embed_tokens.forward_func is sdnq_amd.embedding.quantized_embedding_forward
with torch.no_grad():
    y = m(input_ids=torch.from_numpy(io['input_ids']).cuda()).logits.float().cpu().numpy()
ref = io['logits']
rel = float(np.linalg.norm(y - ref) / np.linalg.norm(ref))
assert rel <= 2e-4, rel
print('ok', rel)
""")
    assert out.strip().splitlines()[-1].startswith("ok")
