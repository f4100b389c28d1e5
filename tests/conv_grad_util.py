"""A torch restatement of the index maps behind the input gradient of a quantized conv (include/sdnq_hip.h: sdnq_hip_im2col_bwd,
sdnq_amd/training.py: QuantizedConvInputGrad), shared by the host and the GPU tests:

    U[(b, ih, iw)][(g, i * kw + j, co_local)] = dY[b][g * C_g + co_local][oh][ow]   with ih + p_h - i * d_h = oh * s_h (likewise w), else 0
    operand_g[ci_local][(i * kw + j, co_local)] = W[g * C_g + co_local][ci_local][i][j]   (the [K][N] transposed weight viewed [C_in][kprod N])
    grad_x (NHWC rows) = cat over g of U[:, group g's columns] @ operand_g^T

Pure indexing and one matmul; nothing here calls the library."""
import torch

# (nd, kernel, stride, padding, dilation, input size); the cases of the issue: partial coverage of the last row / column under stride 2, an
# input row that no window reaches (stride 3), 1 x 1, an output larger than the input (1 x 1 with padding), unequal kernel / padding /
# dilation per axis, an even kernel with stride 2, and two Conv1d layers
GEOMETRIES = [
    (2, (3, 3), (1, 1), (1, 1), (1, 1), (10, 13)),
    (2, (3, 3), (2, 2), (1, 1), (1, 1), (16, 16)),
    (2, (3, 3), (3, 3), (0, 0), (1, 1), (10, 10)),
    (2, (1, 1), (1, 1), (0, 0), (1, 1), (7, 9)),
    (2, (1, 1), (1, 1), (1, 1), (1, 1), (6, 6)),
    (2, (3, 2), (1, 1), (2, 1), (2, 1), (12, 11)),
    (2, (4, 4), (2, 2), (1, 1), (1, 1), (12, 12)),
    (1, (16,), (8,), (4,), (1,), (64,)),
    (1, (3,), (1,), (1,), (1,), (17,)),
]
C_OUTS = (24, 40, 64)
BATCH = 2


def geometry_id(g) -> str:
    nd, k, s, p, d, size = g
    j = lambda t: "x".join(str(e) for e in t)  # noqa: E731
    return f"conv{nd}d_k{j(k)}_s{j(s)}_p{j(p)}_d{j(d)}_in{j(size)}"


def as_2d(g):
    """(kernel, stride, padding, dilation, (H, W)) of a geometry as the 2-D problem: Conv1d is H = 1, kh = 1."""
    nd, k, s, p, d, size = g
    if nd == 1:
        return (1, k[0]), (1, s[0]), (0, p[0]), (1, d[0]), (1, size[0])
    return k, s, p, d, size


def out_hw(in_hw, kernel, stride, padding, dilation):
    return tuple((in_hw[a] + 2 * padding[a] - dilation[a] * (kernel[a] - 1) - 1) // stride[a] + 1 for a in range(2))


def unfold_bwd(dy: torch.Tensor, in_hw, kernel, stride, padding, dilation, groups: int = 1) -> torch.Tensor:
    """U [B * H * W][kh * kw * C_out] from dy [B][C_out][H_out][W_out], the same bits moved."""
    b, c, ho, wo = dy.shape
    (h, w), (kh, kw) = in_hw, kernel
    cg = c // groups
    u = dy.new_zeros(b, h, w, groups, kh * kw, cg)
    ih, iw = torch.arange(h), torch.arange(w)
    for i in range(kh):
        th = ih + padding[0] - i * dilation[0]
        oh = torch.div(th, stride[0], rounding_mode="floor")
        okh = (th >= 0) & (th % stride[0] == 0) & (oh < ho)
        for j in range(kw):
            tw = iw + padding[1] - j * dilation[1]
            ow = torch.div(tw, stride[1], rounding_mode="floor")
            okw = (tw >= 0) & (tw % stride[1] == 0) & (ow < wo)
            if not bool(okh.any()) or not bool(okw.any()):
                continue
            src = dy[:, :, oh[okh]][:, :, :, ow[okw]]                      # [B, C, nh, nw]
            tap = u[:, :, :, :, i * kw + j, :]                             # a view: [B, H, W, G, C_g]
            tap[:, ih[okh][:, None], iw[okw][None, :]] = src.permute(0, 2, 3, 1).reshape(b, src.shape[2], src.shape[3], groups, cg)
    return u.reshape(b * h * w, groups * kh * kw * cg)


def weight_operands(weight: torch.Tensor, groups: int = 1):
    """[per group] [C_in / groups][kprod * C_out / groups]: the rows g N_g .. (g + 1) N_g of the flattened weight [N][K], transposed to
    [K][N_g] (k = ci * kprod + kpos) and viewed with the kernel positions moved to the columns."""
    n = weight.shape[0]
    cg = weight.shape[1]
    w2 = weight.reshape(n, -1)
    ng, kprod = n // groups, w2.shape[1] // cg
    return [w2[g * ng:(g + 1) * ng].t().contiguous().view(cg, kprod * ng) for g in range(groups)]


def grad_input_restated(dy: torch.Tensor, weight: torch.Tensor, in_hw, kernel, stride, padding, dilation, groups: int = 1) -> torch.Tensor:
    """grad_x [B][C_in][H][W] by the gather and the per-group matmul."""
    b = dy.shape[0]
    u = unfold_bwd(dy, in_hw, kernel, stride, padding, dilation, groups)
    per = u.shape[1] // groups
    g2d = torch.cat([u[:, g * per:(g + 1) * per] @ op.t() for g, op in enumerate(weight_operands(weight, groups))], dim=1)
    return g2d.view(b, in_hw[0], in_hw[1], -1).permute(0, 3, 1, 2).contiguous()


def library_grad_input(g, dy: torch.Tensor, weight: torch.Tensor, groups: int = 1) -> torch.Tensor:
    """torch.nn.grad.conv1d_input / conv2d_input on the geometry `g` as given (Conv1d tensors are 3-D)."""
    nd, k, s, p, d, size = g
    shape = (dy.shape[0], weight.shape[1] * groups, *size)
    fn = torch.nn.grad.conv1d_input if nd == 1 else torch.nn.grad.conv2d_input
    return fn(shape, weight, dy, stride=s, padding=p, dilation=d, groups=groups)
