"""sdnq_hip_aq_slab_pack (csrc/gemm_aq.hip): the fragment-ordered copy of an int8 weight that the direct form of the one-launch Linear's
32 x 256 tile reads.  The copy is compared with its definition (include/sdnq_hip.h), evaluated in numpy on position-coded bytes: for
32-row block g, K stage j, sub-step ks and lane l the 16 bytes W[32 g + (l & 31)][128 j + 32 ks + 16 (l >> 5) ..] lie at
((g nk + j) 4 + ks) 1024 + 16 l, rows past N repeating row N - 1.

Shapes: N = 32 (one block), 40 (a second block of 8 live rows), 256, 288 (a block past a full tile); K = 128 (one stage), 640, 1280;
a row stride larger than K."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sdnq_amd import ops  # noqa: E402

NS = [32, 40, 256, 288]
KS = [128, 640, 1280]


def _coded(n, ld):
    """Bytes that name their position: an integer hash of (row, column) over the whole int8 range."""
    with np.errstate(over="ignore"):
        r = np.arange(n, dtype=np.uint32)[:, None]
        c = np.arange(ld, dtype=np.uint32)[None, :]
        h = (r * np.uint32(0x9E3779B1)) ^ (c * np.uint32(0x85EBCA77) + np.uint32(0x27D4EB2F))
        h ^= h >> np.uint32(13)
        h *= np.uint32(0x2C1B3C6D)
        h ^= h >> np.uint32(16)
    return (h & np.uint32(0xFF)).astype(np.uint8).view(np.int8)


def _expected(w, n, k):
    nk, nblk = k // 128, (n + 31) // 32
    g, j, ks, l, e = np.meshgrid(np.arange(nblk), np.arange(nk), np.arange(4), np.arange(64), np.arange(16), indexing="ij")
    rows = np.minimum(32 * g + (l & 31), n - 1)
    cols = 128 * j + 32 * ks + 16 * (l >> 5) + e
    return w[rows, cols].reshape(-1)  # C order of (g, j, ks, l, e) = offset ((g nk + j) 4 + ks) 1024 + 16 l + e


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_copy_is_the_index_formula(n, k, gpu_device):
    for ld in (k, k + 48):
        w = _coded(n, ld)
        b = torch.from_numpy(w).to(gpu_device)[:, :k]
        assert b.stride(0) == ld
        slab = ops.aq_slab_pack(b)
        torch.cuda.synchronize()
        assert slab.numel() == ops.aq_slab_bytes(n, k) == ((n + 31) // 32) * 32 * k
        got = slab.cpu().numpy()
        want = _expected(w, n, k)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (n, k, ld, bad.size, bad[:8].tolist())


def test_null_slab_is_the_plain_entry(gpu_device):
    """sdnq_hip_linear_w8a8_fused_slab with b_slab NULL is sdnq_hip_linear_w8a8_fused: the same bits, whatever tile runs."""
    from sdnq_amd import _lib
    from sdnq_amd.ops import float_code
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    for (m, n, k) in ((70, 512, 1280), (96, 320, 640), (1024, 1280, 1280)):
        x = torch.randn(m, k, generator=g).to(torch.bfloat16).to(gpu_device)
        b = torch.randint(-128, 128, (n, k), dtype=torch.int8, generator=g).to(gpu_device)
        sb = (torch.rand(n, generator=g) * 0.02 + 1e-4).to(gpu_device)
        bias = torch.randn(n, generator=g).to(torch.bfloat16).to(gpu_device)
        ref = ops.linear_w8a8_fused(ops.MM_I8, x, b, sb, bias, torch.bfloat16)
        out = torch.empty_like(ref)
        st = lib.sdnq_hip_linear_w8a8_fused_slab(ops.MM_I8, x.data_ptr(), float_code(x.dtype), m, k, x.stride(0), b.data_ptr(), sb.data_ptr(),
                                                 bias.data_ptr(), float_code(bias.dtype), out.data_ptr(), float_code(out.dtype), n, None,
                                                 ops._stream(x))
        torch.cuda.synchronize()
        assert st == 0
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), (m, n, k)
