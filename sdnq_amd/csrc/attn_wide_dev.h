// What the two units for head dims 136 .. 256 share -- attention_wide.hip (prepare pass and forward) and attention_wide_bwd.hip (lse, dQ,
// dK / dV): the padded head dim and the layout of the workspace that sdnq_hip_attn_wide fills and the backward entry points read.  Host
// code only; anonymous namespace as attn_dev.h.
#pragma once
#include "attn_dev.h"

namespace {

constexpr int WIDE_KMEAN_SPLITS = 32;
constexpr int WIDE_SLOTS = 256;  // a token row is spread over 32 lanes of 8 channels: 256 channel slots, those at or past DP are never stored

// the kernels' head dim: head_dim rounded up to 32 (0: not a head dim of this unit)
inline int wide_dim(int64_t head_dim) { return (head_dim < 136 || head_dim > 256 || head_dim % 8) ? 0 : (int)((head_dim + 31) / 32 * 32); }

inline int64_t up256(int64_t n) { return (n + 255) / 256 * 256; }
struct WideWs { int64_t qq, qs, kq, ks, vt, kmean, total; };
// workspace slices (bytes, 256-byte aligned).  The backward reads qq, qs, kq and ks only: they come first, [0, vt)
inline WideWs wide_ws(int64_t batch, int64_t q_heads, int64_t kv_heads, int64_t q_len, int64_t kv_len, int64_t dp) {
    WideWs w{};
    const int64_t knp = (kv_len + 31) / 32 * 32;
    int64_t off = 0;
    w.qq = off; off += up256(batch * q_heads * q_len * dp);
    w.qs = off; off += up256(batch * q_heads * q_len * 4);
    w.kq = off; off += up256(batch * kv_heads * knp * dp);
    w.ks = off; off += up256(batch * kv_heads * knp * 4);
    w.vt = off; off += up256(batch * kv_heads * knp * dp * 2);
    w.kmean = off; off += up256(batch * kv_heads * WIDE_KMEAN_SPLITS * WIDE_SLOTS * 4);
    w.total = off;
    return w;
}

}  // namespace
