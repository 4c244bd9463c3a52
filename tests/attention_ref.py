"""Host-side references, operand packing and score generators for the attention kernels (csrc/attention.hip).

Plain torch on the CPU, shared by tests/test_attention_host.py (no GPU) and tests/test_gpu_attention_ops.py.

* split_planes / pack_planes: the fp16x2 operand planes the qkv projection's epilogue writes (ConvArgs::ap_*):
  q, k [B][heads][2][L][Dh], v transposed [B][heads][2][Dh][L], plane 0 = fp16(x 2^e), plane 1 = fp16(x 2^e - plane 0).
  pack_planes also returns the DECODED operands (hi + lo) 2^-e in float64: the references run on those, so the
  operand rounding (the producer's, not the attention kernel's) is not charged to the kernel.
* pack_o_split / decode_o_split: the pre-split A image [M][o_ld / 32][piece][4][8] (AttnArgs::o_split).
* attention_f64 / attention_f32: softmax(q k^T) v; the float32 one is the yardstick the kernel's error is held to.
* flash_emulation: attn_flash_kernel's arithmetic restated in fp32 (three-term fp16x2 products, per-64-key online
  maximum / sum in the log2 domain, the 2^ep fold, the fp16x2 split of P); it validates inputs and margins on the CPU.
* generate / case: the seeded score distributions (flat, peaked, ramp, desc, offset, select) and a cache of each
  (shape, distribution)'s planes and references, computed once per session.
"""
import functools
import zlib

import torch

EA, EB, EP, EV = 6, 6, 14, 6   # the plans' exponents (unet_exec.hip / dit_exec.hip: at.ea .. at.ev)
KB = 64                        # keys per block of attn_flash_kernel
FP16_MAX = 65504.0

# (B, heads, L, Dh): the smallest shapes at which each mechanism of attn_flash_kernel exists
FLASH_SHAPES = [
    (1, 3, 64, 32),     # 3 blocks: the remainder branch of xcd_remap_p; one key block
    (2, 2, 128, 32),    # Dh = 32 with a rescale
    (1, 2, 128, 64),
    (1, 3, 128, 72),    # the smallest with a rescale and the 16-row tail
    (1, 2, 192, 80),    # nqb = 3, a whole 16-row tail
    (2, 1, 256, 72),    # 8-wave blocks
    (1, 2, 512, 64),    # two 8-wave query blocks
    (1, 1, 1024, 64),   # ADM's own shape
]
FLASH_DISTS = ['flat', 'peaked', 'ramp8', 'ramp40', 'ramp200', 'desc8', 'desc40', 'desc200', 'offset']
# attn_presplit_kernel<64> / <256> (planes) and attn_fused_kernel (fp32 qkv rows), L = 256
L256_SHAPES = [(2, 2, 256, 64), (1, 1, 256, 256)]
L256_DISTS = ['flat', 'ramp40', 'select']


def split_planes(x, e):
    """s = float32(x) 2^e, hi = fp16(s), lo = fp16(s - hi) (Split<2>::split4; the subtraction is exact in fp32)."""
    s = torch.ldexp(x.to(torch.float32), torch.tensor(e))
    hi = s.to(torch.float16)
    lo = (s - hi.to(torch.float32)).to(torch.float16)
    return hi, lo


def _decode(hi, lo, e):
    return torch.ldexp(hi.to(torch.float64) + lo.to(torch.float64), torch.tensor(-e))


def pack_planes(q, k, v, ea=EA, eb=EB, ev=EV):
    """[B, heads, L, Dh] tensors -> (pq, pk, pv, (qd, kd, vd)): the kernel's fp16 planes (pq, pk
    [B][heads][2][L][Dh], pv [B][heads][2][Dh][L]) and the decoded float64 operands, [B, heads, L, Dh]."""
    qh, ql = split_planes(q, ea)
    kh, kl = split_planes(k, eb)
    vh, vl = split_planes(v, ev)
    pq = torch.stack([qh, ql], dim=2).contiguous()
    pk = torch.stack([kh, kl], dim=2).contiguous()
    pv = torch.stack([vh.transpose(-1, -2), vl.transpose(-1, -2)], dim=2).contiguous()
    return pq, pk, pv, (_decode(qh, ql, ea), _decode(kh, kl, eb), _decode(vh, vl, ev))


def unpack_planes(pq, pk, pv, ea=EA, eb=EB, ev=EV):
    """The inverse of pack_planes' layouts: the decoded float64 operands [B, heads, L, Dh]."""
    return (_decode(pq[:, :, 0], pq[:, :, 1], ea), _decode(pk[:, :, 0], pk[:, :, 1], eb),
            _decode(pv[:, :, 0], pv[:, :, 1], ev).transpose(-1, -2))


def pack_o_split(x, o_ld, ea):
    """[M, C] (C <= o_ld) -> the pre-split A image [M][o_ld / 32][piece][4][8] fp16 of x 2^ea (zero beyond C)."""
    M, C = x.shape
    xp = torch.zeros((M, o_ld), dtype=torch.float32)
    xp[:, :C] = x
    hi, lo = split_planes(xp, ea)
    return torch.stack([hi.view(M, o_ld // 32, 32), lo.view(M, o_ld // 32, 32)], dim=2).contiguous().view(-1)


def decode_o_split(img, M, o_ld, ea):
    """The image [M][o_ld / 32][piece][4][8] -> float64 [M, o_ld]: (hi + lo) 2^-ea."""
    g = img.view(M, o_ld // 32, 2, 32)
    return _decode(g[:, :, 0].reshape(M, o_ld), g[:, :, 1].reshape(M, o_ld), ea)


def attention_f64(q, k, v):
    q, k, v = q.double(), k.double(), v.double()
    return torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v


def attention_f32(q, k, v):
    q, k, v = q.float(), k.float(), v.float()
    return torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v


def flash_emulation(pq, pk, pv, ea=EA, eb=EB, ep=EP, ev=EV):
    """attn_flash_kernel in fp32 on the planes: per 64-key block S = k1 q0 + k0 q1 + k0 q0 (fp32 accumulation of
    exact fp16 products), m = max(m, fl(max S * sl2)) with sl2 = fl(2^-(ea + eb) log2 e), corr = exp2(m_old - m),
    x = exp2(fma(S, sl2, ep - m)), l = l corr + sum x, P = fp16x2(x), O = O corr + v1 p0 + v0 p1 + v0 p0; the
    output O 2^-ev / l. Returns float32 [B, heads, L, Dh]."""
    f32 = torch.float32
    q0, q1 = pq[:, :, 0].to(f32), pq[:, :, 1].to(f32)
    k0, k1 = pk[:, :, 0].to(f32), pk[:, :, 1].to(f32)
    v0, v1 = pv[:, :, 0].to(f32), pv[:, :, 1].to(f32)   # [B, heads, Dh, L]
    B, H, L, Dh = q0.shape
    sl2 = (torch.tensor(2.0 ** -(ea + eb), dtype=f32) * torch.tensor(1.4426950408889634, dtype=f32))
    m = torch.full((B, H, L), float('-inf'), dtype=f32)
    l = torch.zeros((B, H, L), dtype=f32)
    O = torch.zeros((B, H, L, Dh), dtype=f32)
    for kb in range(L // KB):
        ks = slice(kb * KB, (kb + 1) * KB)
        kt0, kt1 = k0[:, :, ks].transpose(-1, -2), k1[:, :, ks].transpose(-1, -2)
        S = q0 @ kt1 + q1 @ kt0 + q0 @ kt0                       # [B, H, L, 64]
        m_new = torch.maximum(m, S.amax(dim=-1) * sl2)
        corr = torch.exp2(m - m_new)
        mb = float(ep) - m_new
        arg = (S.double() * sl2.double() + mb.double()[..., None]).to(f32)   # the FMA: one rounding
        x = torch.exp2(arg)
        l = l * corr + x.sum(dim=-1)
        p0 = x.to(torch.float16).to(f32)
        p1 = (x - p0).to(torch.float16).to(f32)
        vt0, vt1 = v0[:, :, :, ks].transpose(-1, -2), v1[:, :, :, ks].transpose(-1, -2)   # [B, H, 64, Dh]
        O = O * corr[..., None] + (p0 @ vt1 + p1 @ vt0 + p0 @ vt0)
        m = m_new
    return O * (torch.tensor(2.0 ** -ev, dtype=f32) / l)[..., None]


def _seed(shape, dist):
    return zlib.crc32(repr((tuple(shape), dist)).encode()) & 0x7fffffff


def generate(shape, dist):
    """Seeded fp32 (q, k, v) [B, heads, L, Dh] of one score distribution, plus pi ([B, heads, L] winning key of
    each query) for 'select', else None.

    flat: q ~ N(0, 1 / Dh), k, v ~ N(0, 1).  peaked: q x 4.  ramp<gap> / desc<gap>: with a shared unit direction u,
    q + u sqrt(gap), k_j + r_j u sqrt(gap), r_j rising (ramp) or falling (desc) from 0 to 1 across the keys.
    offset: q + 4 u, k + 60 u (every score shifted by about 250 nats).  select: k rows distinct random +-1 vectors,
    q_i = 64 k_pi(i) for a random permutation pi, v integers in [-8, 8]: the winning score beats every other by
    at least 128 nats and the exact answer is v[pi(i)]."""
    B, H, L, Dh = shape
    g = torch.Generator().manual_seed(_seed(shape, dist))
    if dist == 'select':
        k = (torch.randint(0, 2, (B, H, L, Dh), generator=g) * 2 - 1).float()
        for b in range(B):
            for h in range(H):
                assert torch.unique(k[b, h], dim=0).shape[0] == L, 'select: the key rows must be distinct'
        pi = torch.stack([torch.stack([torch.randperm(L, generator=g) for _ in range(H)]) for _ in range(B)])
        q = 64.0 * torch.gather(k, 2, pi[..., None].expand(B, H, L, Dh))
        v = torch.randint(-8, 9, (B, H, L, Dh), generator=g).float()
        return q, k, v, pi
    q = torch.randn((B, H, L, Dh), generator=g) / Dh ** 0.5
    k = torch.randn((B, H, L, Dh), generator=g)
    v = torch.randn((B, H, L, Dh), generator=g)
    u = torch.randn((Dh, ), generator=g)
    u = u / u.norm()
    if dist == 'flat':
        pass
    elif dist == 'peaked':
        q = q * 4.0
    elif dist.startswith('ramp') or dist.startswith('desc'):
        gap = float(dist[4:])
        r = torch.arange(L, dtype=torch.float32) / (L - 1)
        if dist.startswith('desc'):
            r = 1.0 - r
        q = q + u * gap ** 0.5
        k = k + r[:, None] * u * gap ** 0.5
    elif dist == 'offset':
        q = q + 4.0 * u
        k = k + 60.0 * u
    else:
        raise ValueError(dist)
    return q, k, v, None


@functools.lru_cache(maxsize=None)
def case(shape, dist):
    """One (shape, distribution): the fp32 inputs, the planes, the decoded operands' float64 result `ref`, its
    max |ref| `scale`, the float32 yardstick's error `e32`, and the bound 2 e32 + 2^-21 scale. Cached: computed
    once and shared; callers must not modify the tensors."""
    q, k, v, pi = generate(shape, dist)
    pq, pk, pv, (qd, kd, vd) = pack_planes(q, k, v)
    ref = attention_f64(qd, kd, vd)
    e32 = (attention_f32(qd, kd, vd).double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    return dict(q=q, k=k, v=v, pi=pi, pq=pq, pk=pk, pv=pv, dec=(qd, kd, vd), ref=ref, e32=e32, scale=scale,
                bound=2.0 * e32 + 2.0 ** -21 * scale)


def selected_rows(v, pi):
    """v[pi]: the exact answer of a 'select' case, [B, heads, L, Dh]."""
    return torch.gather(v, 2, pi[..., None].expand(*v.shape))


def out_rows(o, heads, Dh):
    """The kernel's out rows [B, L, >= heads Dh] -> [B, heads, L, Dh]."""
    B, L = o.shape[:2]
    return o[..., :heads * Dh].reshape(B, L, heads, Dh).permute(0, 2, 1, 3)
