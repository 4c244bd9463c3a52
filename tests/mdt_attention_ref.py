"""Host-side references and case generators for the biased flash attention (csrc/attention.hip, BW > 0) and the
unfused softmax_rows_bias: softmax(q k^T + bias[h]) v with bias[h][i][j] = table[h][rel_index(i, j)] on a W x W grid.

Plain torch on the CPU, shared by tests/test_mdt_host.py (no GPU) and tests/test_gpu_mdt_ops.py; the operand packing
and the unbiased pieces come from tests/attention_ref.py.

* rel_index(W): (iy - jy + W - 1)(2W - 1) + (ix - jx + W - 1), the closed form the kernels use.
* kernel_table(table): what the engine hands the flash kernel -- [heads][(2W - 1)^2] float32 of table * log2(e),
  the product formed in float64 and rounded once (dit_exec.hip dit_create).
* case(shape, dist): operands on decoded fp16x2 planes, a float32 table in natural units, the float64 reference
  `ref`, torch float32's error `e32` on the same operands and table, and bound = 2 e32 + 2^-21 max|ref| -- the
  project's bound for fp16x2 against fp32 arithmetic (tests/attention_ref.py).
* flash_bias_emulation: the BIAS kernel's arithmetic restated in fp32 (s' = fma(S, sl2, table log2e) BEFORE the running
  maximum, x = exp2(s' + (ep - m))): validates cases and margins on the CPU.

Distributions (scores x table):
  rand        flat scores, table ~ N(0, 1)
  up40/down40 flat scores, bias linear in the key index, rising / falling by 40 nats across the keys (the maximum
              moves to a later key block every block / sits in the first)
  cross       scores rising by 40 nats across the keys (ramp40), bias falling by 80: the biased maximum is in the
              first key block while the raw scores' maximum is in the last -- a maximum taken before the bias
              overflows exp2 here
  cross_rev   scores falling by 40, bias rising by 80
  select      q = 0; per head the table is 128 * (a random permutation of 0 .. (2W - 1)^2 - 1): each query's winner,
              the key with the highest-ranked relative offset, is ahead by >= 128 nats; v rows are integers, so the
              exact output is v[pi(i)]
"""
import functools
import zlib

import torch

from tests import attention_ref as ar

LOG2E = 1.4426950408889634074

# (B, heads, L, Dh) -> W = sqrt(L)
SHAPES = [(2, 3, 64, 32), (1, 2, 256, 72), (2, 2, 256, 64), (1, 2, 1024, 64)]
DISTS = ['rand', 'up40', 'down40', 'cross', 'cross_rev']


def grid_w(L):
    W = int(round(L ** 0.5))
    assert W * W == L
    return W


def rel_index(W):
    p = torch.arange(W * W)
    py, px = p // W, p % W
    return (py[:, None] - py[None, :] + W - 1) * (2 * W - 1) + (px[:, None] - px[None, :] + W - 1)


def bias_matrix(table, W):
    """table [heads, (2W - 1)^2] -> bias [heads, L, L]."""
    return table[:, rel_index(W)]


def kernel_table(table, stride=None):
    """[heads, n] float32 natural units -> [heads, stride] float32 of table * log2(e) (float64 product, one rounding),
    zero padded."""
    H, n = table.shape
    stride = stride or n
    out = torch.zeros((H, stride), dtype=torch.float32)
    out[:, :n] = (table.double() * LOG2E).float()
    return out


def attention_bias_f64(q, k, v, bias):
    s = q.double() @ k.double().transpose(-1, -2) + bias.double()[None]
    return torch.softmax(s, dim=-1) @ v.double()


def attention_bias_f32(q, k, v, bias):
    s = q.float() @ k.float().transpose(-1, -2) + bias.float()[None]
    return torch.softmax(s, dim=-1) @ v.float()


def _seed(shape, dist):
    return zlib.crc32(repr(('mdt', tuple(shape), dist)).encode()) & 0x7fffffff


def linear_table(W, heads, gap):
    """bias[i][j] = -gap (j - i) / (L - 1) for every head: linear in the key index (falling for gap > 0), which a
    relative-position table can express since j - i = -(dy W + dx)."""
    L = W * W
    n = torch.arange((2 * W - 1) ** 2)
    dy, dx = n // (2 * W - 1) - (W - 1), n % (2 * W - 1) - (W - 1)   # qy - ky, qx - kx
    t = (gap * (dy * W + dx).float() / (L - 1)).float()
    return t[None].repeat(heads, 1).contiguous()


def generate(shape, dist):
    """(q, k, v, table, pi): fp32 [B, heads, L, Dh] operands, a float32 table [heads, (2W - 1)^2] in natural units,
    pi [heads, L] (the winning key of each query) for 'select', else None."""
    B, H, L, Dh = shape
    W = grid_w(L)
    n = (2 * W - 1) ** 2
    g = torch.Generator().manual_seed(_seed(shape, dist))
    if dist == 'select':
        q = torch.zeros((B, H, L, Dh))
        k = torch.randn((B, H, L, Dh), generator=g)
        v = torch.randint(-8, 9, (B, H, L, Dh), generator=g).float()
        table = torch.stack([torch.randperm(n, generator=g) for _ in range(H)]).float() * 128.0
        pi = bias_matrix(table, W).argmax(dim=-1)
        return q, k, v, table, pi
    if dist == 'rand':
        q, k, v, _ = ar.generate(shape, 'flat')
        return q, k, v, torch.randn((H, n), generator=g), None
    if dist in ('up40', 'down40'):
        q, k, v, _ = ar.generate(shape, 'flat')
        return q, k, v, linear_table(W, H, 40.0 if dist == 'down40' else -40.0), None
    if dist == 'cross':
        q, k, v, _ = ar.generate(shape, 'ramp40')
        return q, k, v, linear_table(W, H, 80.0), None
    if dist == 'cross_rev':
        q, k, v, _ = ar.generate(shape, 'desc40')
        return q, k, v, linear_table(W, H, -80.0), None
    raise ValueError(dist)


@functools.lru_cache(maxsize=None)
def case(shape, dist):
    """One (shape, distribution), computed once and shared; callers must not modify the tensors."""
    q, k, v, table, pi = generate(shape, dist)
    W = grid_w(shape[2])
    pq, pk, pv, (qd, kd, vd) = ar.pack_planes(q, k, v)
    bias = bias_matrix(table, W)
    ref = attention_bias_f64(qd, kd, vd, bias)
    e32 = (attention_bias_f32(qd, kd, vd, bias).double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    return dict(q=q, k=k, v=v, pi=pi, table=table, W=W, pq=pq, pk=pk, pv=pv, dec=(qd, kd, vd), ref=ref, e32=e32,
                scale=scale, bound=2.0 * e32 + 2.0 ** -21 * scale)


def selected_rows(v, pi):
    """v[:, h, pi[h]]: the exact answer of a 'select' case, [B, heads, L, Dh]."""
    B, H, L, Dh = v.shape
    return torch.gather(v, 2, pi[None, :, :, None].expand(B, H, L, Dh))


def flash_bias_emulation(pq, pk, pv, ktable, W, ea=ar.EA, eb=ar.EB, ep=ar.EP, ev=ar.EV):
    """attn_flash_kernel<.., BW > 0> in fp32 on the planes, ktable = kernel_table(table): per 64-key block
    S = k1 q0 + k0 q1 + k0 q0, s' = fma(S, sl2, ktable[rel]) (one rounding), m = max(m, max s'),
    corr = exp2(m_old - m), x = exp2(s' + (ep - m)), l = l corr + sum x, P = fp16x2(x), O = O corr + P v; the output
    O 2^-ev / l. Returns float32 [B, heads, L, Dh]."""
    f32 = torch.float32
    q0, q1 = pq[:, :, 0].to(f32), pq[:, :, 1].to(f32)
    k0, k1 = pk[:, :, 0].to(f32), pk[:, :, 1].to(f32)
    v0, v1 = pv[:, :, 0].to(f32), pv[:, :, 1].to(f32)
    B, H, L, Dh = q0.shape
    kbias = bias_matrix(ktable[:, :(2 * W - 1) ** 2], W)   # [H, L, L] log2 units
    sl2 = (torch.tensor(2.0 ** -(ea + eb), dtype=f32) * torch.tensor(1.4426950408889634, dtype=f32))
    m = torch.full((B, H, L), float('-inf'), dtype=f32)
    l = torch.zeros((B, H, L), dtype=f32)
    O = torch.zeros((B, H, L, Dh), dtype=f32)
    for kb in range(L // ar.KB):
        ks = slice(kb * ar.KB, (kb + 1) * ar.KB)
        kt0, kt1 = k0[:, :, ks].transpose(-1, -2), k1[:, :, ks].transpose(-1, -2)
        S = q0 @ kt1 + q1 @ kt0 + q0 @ kt0
        sp = (S.double() * sl2.double() + kbias[None, :, :, ks].double()).to(f32)   # the FMA: one rounding
        m_new = torch.maximum(m, sp.amax(dim=-1))
        corr = torch.exp2(m - m_new)
        mb = float(ep) - m_new
        x = torch.exp2(sp + mb[..., None])
        l = l * corr + x.sum(dim=-1)
        p0 = x.to(torch.float16).to(f32)
        p1 = (x - p0).to(torch.float16).to(f32)
        vt0, vt1 = v0[:, :, :, ks].transpose(-1, -2), v1[:, :, :, ks].transpose(-1, -2)
        O = O * corr[..., None] + (p0 @ vt1 + p1 @ vt0 + p0 @ vt0)
        m = m_new
    return O * (torch.tensor(2.0 ** -ev, dtype=f32) / l)[..., None]
