"""Host-side references, operand generators and an fp32 emulation for the DiT token path: the linear_k32 / gemm.hip
forms of the token GEMMs (csrc/linear_k32.hip, csrc/gemm.hip), the row kernels (csrc/dit_kernels.hip) and
embed_add_silu.

Plain torch on the CPU, shared by tests/test_token_host.py (no GPU) and tests/test_gpu_token_ops.py. The fp16x2
packers (split_planes, unpack_planes, pack_o_split / decode_o_split: the pre-split A image and c_split share the
[M][K / 32][piece][4][8] layout) are tests/attention_ref.py's.

* split_exact: operands whose fp16x2 split loses nothing, for the bit-for-bit permutation and range-flag tests.
* ln_modulate / epilogue / gemm_refs: the float64 reference and the float32 yardstick (torch CPU fp32 prologue,
  matmul, epilogue) of one GEMM spec, from LayerNorm statistics the caller provides (the GPU tests pass the
  device's own, so a 1-ulp difference in float(mean) -- amplified by mean / std -- is not charged to the GEMM).
* gemm_emulation: the fp16x2 arithmetic restated in fp32 (A split after 2^ea, W after its power-of-two row scale,
  acc = a1 w0 + a0 w1 + a0 w0 unscaled, then the fp32 epilogue); EmuBackend wraps it (and the row kernels) behind
  the interface the GPU tests' device backend has, so their checking functions are dry-run on the CPU.
* row_stats_f64, the seeded case generators and a per-session cache of each case's operands (lru_cache: computed
  once and shared; callers must not modify the tensors). The references of the LayerNorm cases depend on the
  statistics passed in, so a check computes them once per case and shares them among its arms.

Bounds (tests/test_gpu_token_ops.py holds the kernels to them, tests/test_token_host.py the emulation):
  fp32 outputs   |out - ref64| <= 2 e32 + 2^-21 max|ref64|        (REL = 2^-21, test_gpu_attention_ops.py's constant)
  activations    the same times 1.13 (max |GELU'|) + 4 ulp of the output
  fp16x2 images  + 2^-22 |y| + 2^-(24 + e)                           (the representation: two fp16 roundings)
Measured on the CPU (tests/test_token_host.py test_gemm_emulation_meets_the_bound_in_every_case, K = 64 .. 1536):
the emulation stays below 2 e32 alone in every GEMM case (worst err / e32 1.64, the gated residual at T = 16,
N = 192), so REL stands as the attention tests have it; it is the kernels' margin for their summation order.
"""
import functools
import math
import zlib

import torch

from tests import attention_ref as ar

FP16_MAX = ar.FP16_MAX
HALF_RANGE = FP16_MAX / 2     # every non-flag case keeps |operand 2^e| below this
REL = 2.0 ** -21
EA = 6                        # the plans' activation exponent (dit_exec.hip: 2^6 for tokens, q, k, v, MLP outputs)
LN_EPS = float(torch.tensor(1e-6, dtype=torch.float32))   # the plans' 1e-6f, as the kernels see it
SENT16 = 0x7e2a               # an fp16 NaN pattern no kernel writes (as the attention tests')
PAD = 8                       # sentinel columns after N in every C row
TILE = 128                    # sentinel rows past M (one M tile)
PLANE_TAIL = 2048             # sentinel fp16 elements past the end of each plane buffer
F32, F64 = torch.float32, torch.float64


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def split_exact(x, e):
    """x rounded so that x 2^e = hi + lo exactly (hi, lo the fp16x2 pieces): fp32."""
    hi, lo = ar.split_planes(x, e)
    return torch.ldexp(hi.to(F32) + lo.to(F32), torch.tensor(-e))


# --------------------------------------------------------------------------------------------- rows and tables
LN_DISTS = ['std', 'offset', 'mixed']
ROW_DISTS = ['std', 'offset', 'mixed', 'spike', 'const']


def token_rows(dist, M, K, g):
    """Seeded fp32 token rows [M, K] of one distribution (the LayerNorm forms' inputs)."""
    z = torch.randn((M, K), generator=g)
    if dist == 'std':
        return z
    if dist == 'offset':
        return 50.0 + 0.05 * z
    if dist == 'mixed':
        means = torch.tensor([0.0, 30.0, -30.0, 300.0])[torch.randint(0, 4, (M, ), generator=g)]
        stds = torch.tensor([1e-2, 1.0, 10.0])[torch.randint(0, 3, (M, ), generator=g)]
        return means[:, None] + stds[:, None] * z
    if dist == 'spike':
        x = 1e-2 * z
        x[torch.arange(M), torch.randint(0, K, (M, ), generator=g)] = 1e3
        return x
    if dist == 'const':
        return torch.full((M, K), 3.0)
    raise ValueError(dist)


def mod_tables(B, width, g, names=('shift', 'scale', 'gate')):
    """The modulation tables inside a wider [B][pitch] buffer (as `mods` with ada_total): every float outside the
    addressed tables is NaN, the column offsets are multiples of 4 (16-byte rows) and differ per table.
    scale ~ U(-0.5, 1.5) + 0.25 img, shift ~ U(-2, 2) + img, gate ~ U(-2, 2) - 0.5 img: a row looked up in the wrong
    image's table is off by O(1). -> (buffer [B, pitch], {name: column offset})."""
    off, at = {}, 4
    for n in names:
        off[n] = at
        at += width + 4
    pitch = at + 4
    buf = torch.full((B, pitch), float('nan'))
    img = torch.arange(B, dtype=F32)[:, None]
    for n in names:
        u = torch.rand((B, width), generator=g)
        if n == 'scale':
            t = -0.5 + 2.0 * u + 0.25 * img
        elif n == 'shift':
            t = -2.0 + 4.0 * u + img
        else:
            t = -2.0 + 4.0 * u - 0.5 * img
        buf[:, off[n]:off[n] + width] = t
    return buf, off


def table(buf, off, name, width):
    return buf[:, off[name]:off[name] + width]


def row_stats_f64(x, eps=LN_EPS):
    """float64 (mean, 1 / sqrt(var + eps)) of each row, the variance around the float64 mean: [rows, 2]."""
    x = x.to(F64)
    mean = x.mean(dim=1)
    var = ((x - mean[:, None]) ** 2).mean(dim=1)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], dim=1)


def row_stats_f32(x, eps=LN_EPS):
    """row_stats_kernel's roundings of the float64 statistics: (float(mean), 1.0f / sqrtf(float(var) + eps))."""
    x64 = x.to(F64)
    mean = x64.mean(dim=1)
    var = ((x64 - mean[:, None]) ** 2).mean(dim=1).to(F32)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))
    return torch.stack([mean.to(F32), rstd], dim=1)


def ln_modulate(x, stats32, scale, shift, rows_per_image, dtype=F64):
    """((x - mean) rstd) (1 + scale[img]) + shift[img], img = row // rows_per_image, in `dtype` (float64: the
    reference; float32: the kernels' own expression, separately rounded) from fp32 statistics [rows, 2]."""
    M = x.shape[0]
    img = torch.arange(M) // rows_per_image
    st = stats32.to(dtype)
    one = torch.tensor(1.0, dtype=dtype)
    return ((x.to(dtype) - st[:, 0:1]) * st[:, 1:2]) * (one + scale.to(dtype)[img]) + shift.to(dtype)[img]


def activation(y, act):
    if act == 1:
        return torch.nn.functional.silu(y)
    if act == 2:
        return torch.nn.functional.gelu(y, approximate='tanh')
    return y


def epilogue(y, s, dtype):
    """bias, residual with res_mod / gated residual res + gate[img] (acc + bias), activation, in `dtype`."""
    M = y.shape[0]
    if s.get('bias') is not None:
        y = y + s['bias'].to(dtype)
    if s.get('res') is not None:
        rows = torch.arange(M)
        r = s['res'].to(dtype)[rows % s['res_mod'] if s.get('res_mod', 0) > 0 else rows]
        if s.get('gate') is not None:
            y = r + s['gate'].to(dtype)[rows // s['gate_rows']] * y
        else:
            y = y + r
    return activation(y, s.get('act', 0))


def prologue(s, stats32, dtype):
    a = s['A']
    if s.get('ln'):
        a = ln_modulate(a, stats32, s['ln_scale'], s['ln_shift'], s['ln_rows'], dtype)
    else:
        a = a.to(dtype)
    if s.get('alpha', 1.0) != 1.0:
        a = a * torch.tensor(s['alpha'], dtype=F32).to(dtype)
    return a


def gemm_refs(s, stats32=None, a64=None):
    """One GEMM spec -> dict(ref float64 [M, N], e32, scale = max|ref|, bound (elementwise tensor or float)).
    a64: the float64 A after the prologue when the caller has it already (a decoded pre-split image)."""
    out = {}
    for dt in (F64, F32):
        a = prologue(s, stats32, dt) if a64 is None else a64.to(dt)
        out[dt] = epilogue(a @ s['W'].to(dt).T, s, dt)
    ref = out[F64]
    e32 = (out[F32].to(F64) - ref).abs().max().item()
    scale = ref.abs().max().item()
    base = 2.0 * e32 + REL * scale
    if s.get('act', 0):
        bound = 1.13 * base + 4.0 * 2.0 ** -23 * ref.abs()
    else:
        bound = torch.full_like(ref, base)
    return dict(ref=ref, e32=e32, scale=scale, base=base, bound=bound)


def image_term(y, e):
    """The fp16x2 representation of y 2^e, as an error of y: 2^-22 |y| + 2^-(24 + e)."""
    return 2.0 ** -22 * y.abs() + 2.0 ** -(24 + e)


# ------------------------------------------------------------------------------------------------- emulation
def weight_row_exponents(W):
    """e[n] with max|W[n]| 2^e in [2^13, 2^14) (0 for a zero row), as split_conv_weights' row scales."""
    m = W.abs().amax(dim=1)
    _, ex = torch.frexp(m)
    return torch.where(m > 0, 14 - ex, torch.zeros_like(ex)).to(torch.int32)


def weight_exponent(W):
    """split_weight_exponent: one exponent for the whole matrix (gemm.hip's fp16x2 path)."""
    m = W.abs().max().item()
    return 0 if m == 0 else 14 - math.frexp(m)[1]


def a_pieces(s, stats32):
    """The prologue'd, alpha- and 2^ea-scaled A rows and their fp16x2 pieces, in the kernels' fp32 expressions."""
    a = prologue(s, stats32, F32)
    hi, lo = ar.split_planes(a, s['ea'])
    return torch.ldexp(a, torch.tensor(s['ea'])), hi, lo


def _acc(a0, a1, w0, w1):
    f = lambda t: t.to(F32)  # noqa: E731
    return (f(a1) @ f(w0).T + f(a0) @ f(w1).T) + f(a0) @ f(w0).T


def gemm_emulation(s, stats32=None, a_img=None):
    """The GEMM of spec s in the device's arithmetic restated in fp32. path 0 (linear_k32): W split after its row
    scale; 1 (gemm.hip fp16x2): after one matrix-wide scale; 2: plain fp32. a_img: a pre-split A image to use
    instead of the prologue (a_form 2 and the second GEMM of a chain). -> dict(acc: the unscaled accumulator
    [M, N] before the epilogue, y: fp32 after it, flag: an A element beyond fp16 at 2^ea)."""
    M, N, K = s['A'].shape[0] if a_img is None else s['M'], s['W'].shape[0], s['W'].shape[1]
    path = s.get('path', 0)
    flag = 0
    if path == 2:
        y = prologue(s, stats32, F32) @ s['W'].T
    else:
        if a_img is None:
            sa, a0, a1 = a_pieces(s, stats32)
            flag |= int((sa.abs() > FP16_MAX).any())
        else:
            g = a_img.view(M, K // 32, 2, 32)
            a0, a1 = g[:, :, 0].reshape(M, K), g[:, :, 1].reshape(M, K)
        if path == 0:
            e = weight_row_exponents(s['W'])
            w0, w1 = ar.split_planes(torch.ldexp(s['W'], e[:, None]), 0)
            y = _acc(a0, a1, w0, w1) * torch.ldexp(torch.ones(N), -e - s['ea'])[None, :]
        else:
            e = weight_exponent(s['W'])
            w0, w1 = ar.split_planes(s['W'], e)
            y = _acc(a0, a1, w0, w1) * 2.0 ** -(e + s['ea'])
    return dict(acc=y, y=epilogue(y, s, F32), flag=flag)


# ------------------------------------------------------------------------------------- attention plane geometry
def plane_columns(ap):
    """Column n of the qkv GEMM -> (part, head, d) index tensors, for the q | k | v block order, the per-head
    [q; k; v] order (legacy) and the all-v form (vonly)."""
    H, Dh = ap['heads'], ap['Dh']
    C = H * Dh
    n = torch.arange(C if ap.get('vonly') else 3 * C)
    if ap.get('vonly'):
        return torch.full_like(n, 2), n // Dh, n % Dh
    if ap.get('legacy'):
        h = n // (3 * Dh)
        r = n - h * 3 * Dh
        return r // Dh, h, r % Dh
    part = n // C
    r = n - part * C
    return part, r // Dh, r % Dh


def plane_scales(ap):
    """(q, k, v) factors applied before 2^e: ap_alpha (unless 1), ap_bscale (unless 0 or 1), 1."""
    bs = ap.get('bscale', 0.0)
    return (ap['alpha'], bs if bs not in (0.0, 1.0) else 1.0, 1.0)


def rows_to_heads(y, ap, B):
    """GEMM output rows [B L, N] -> (q, k, v) [B, heads, L, Dh] (None for the parts the form does not have)."""
    part, h, d = plane_columns(ap)
    L, H, Dh = ap['L'], ap['heads'], ap['Dh']
    out = []
    for p in range(3):
        sel = part == p
        if not sel.any():
            out.append(None)
            continue
        t = torch.zeros((B, H, L, Dh), dtype=y.dtype)
        t[:, h[sel], :, d[sel]] = y[:, sel].reshape(B, L, -1).permute(2, 0, 1)   # (the indexed dims come first)
        out.append(t)
    return out


def heads_from_rows(y, ap, B):
    """Plain-loop form of rows_to_heads (the layouts' definition; the host tests compare the two)."""
    part, h, d = plane_columns(ap)
    L, H, Dh = ap['L'], ap['heads'], ap['Dh']
    out = [None, None, None]
    yr = y.reshape(B, L, -1)
    for n in range(yr.shape[2]):
        p = int(part[n])
        if out[p] is None:
            out[p] = torch.zeros((B, H, L, Dh), dtype=y.dtype)
        out[p][:, int(h[n]), :, int(d[n])] = yr[:, :, n]
    return out


# ------------------------------------------------------------------------------------------------ the backend
def sentinel_image(n):
    return torch.full((n, ), SENT16, dtype=torch.int16)


class EmuBackend:
    """The GPU tests' backend interface on the CPU: every call answered by the fp32 emulation, with the same output
    buffers (NaN / sentinel prefill, pad columns, a sentinel tile of rows past M) the device backend allocates."""
    name = 'emulation'

    def row_stats(self, x, eps=LN_EPS, mod=None, img=False, ea=EA):
        """-> (stats fp32 [rows, 2], image int16 [(rows + 4) 2 D] or None, flag). mod: dict(buf, shift, scale
        (column offsets), rows (per image))."""
        st = row_stats_f32(x, eps)
        if not img:
            return st, None, 0
        rows, D = x.shape
        y = ln_modulate(x, st, mod['buf'][:, mod['scale']:mod['scale'] + D], mod['buf'][:, mod['shift']:mod['shift'] + D],
                        mod['rows'], F32)
        out = sentinel_image((rows + 4) * 2 * D)
        out[:rows * 2 * D] = ar.pack_o_split(y, D, ea).view(torch.int16)
        return st, out, int((torch.ldexp(y, torch.tensor(ea)).abs() > FP16_MAX).any())

    def gemm(self, s, stats32=None):
        """-> dict(C [M + TILE, N + PAD] fp32 | None, as_img, c_img (int16, sentinel rows past M), planes (q, k, v
        int16 with PLANE_TAIL sentinels), flag, rc)."""
        M, N, K = s['M'], s['W'].shape[0], s['W'].shape[1]
        a_form, path = s.get('a_form', 0), s.get('path', 0)
        out = dict(C=None, as_img=None, c_img=None, planes=None, flag=0, rc=0)
        if a_form == 1:
            out['as_img'] = sentinel_image((M + TILE) * 2 * K)
        if s.get('ap'):
            n = (M // s['ap']['L']) * s['ap']['heads'] * 2 * s['ap']['L'] * s['ap']['Dh']
            out['planes'] = tuple(sentinel_image(n + PLANE_TAIL) for _ in range(3))
        elif s.get('c_split'):
            out['c_img'] = sentinel_image((M + TILE) * 2 * N)
        else:
            out['C'] = torch.full((M + TILE, N + PAD), float('nan'))
        # what the hook refuses (DM_ERR_UNSUPPORTED, nothing launched): gemm.hip has no linear_k32-only form;
        # linear_k32_ok's shape rules
        refused = path != 0 and (a_form == 2 or s.get('c_split') or s.get('ap'))
        if path == 0:
            refused = (K % 64 != 0 or N % 4 != 0 or (s.get('c_split') and N % 64 != 0)
                       or (s.get('ln') and a_form == 0 and s['ln_rows'] < TILE) or (s.get('ln') and a_form == 2))
        if refused:
            out['rc'] = -4
            return out
        a_img = None
        if a_form == 1:
            sa, a0, a1 = a_pieces(s, stats32)
            out['flag'] |= int((sa.abs() > FP16_MAX).any())
            img = out['as_img']
            img[:M * 2 * K] = torch.stack([a0.view(M, K // 32, 32), a1.view(M, K // 32, 32)], dim=2).reshape(-1).view(torch.int16)
            if path == 0:
                a_img = img[:M * 2 * K].view(torch.float16)
        elif a_form == 2:
            a_img = s['as_img'][:M * 2 * K].view(torch.float16)
        e = gemm_emulation(s, stats32, a_img)
        out['flag'] |= e['flag']
        if s.get('ap'):
            ap = s['ap']
            B = M // ap['L']
            parts = rows_to_heads(e['y'], ap, B)
            sc = plane_scales(ap)
            exps = (ap['ea'], ap['eb'], ap['ev'])
            planes = out['planes']
            for p in range(3):
                n = B * ap['heads'] * 2 * ap['L'] * ap['Dh']
                buf = planes[p]
                if parts[p] is not None:
                    y = parts[p] * torch.tensor(sc[p], dtype=F32) if sc[p] != 1.0 else parts[p]
                    out['flag'] |= int((torch.ldexp(y, torch.tensor(exps[p])).abs() > FP16_MAX).any())
                    hi, lo = ar.split_planes(y, exps[p])
                    if p == 2:
                        hi, lo = hi.transpose(-1, -2), lo.transpose(-1, -2)
                    buf[:n] = torch.stack([hi, lo], dim=2).contiguous().view(-1).view(torch.int16)
        elif s.get('c_split'):
            img = out['c_img']
            img[:M * 2 * N] = ar.pack_o_split(e['y'], N, s['c_split_ea']).view(torch.int16)
            out['flag'] |= int((torch.ldexp(e['y'], torch.tensor(s['c_split_ea'])).abs() > FP16_MAX).any())
        else:
            out['C'][:M, :N] = e['y']
        return out

    def attention(self, shape, pq, pk, pv):
        return ar.flash_emulation(pq, pk, pv), 0

    def patchify(self, x, p, inverse=False, C=None, S=None):
        if not inverse:
            B, C, S, _ = x.shape
            return x.reshape(B, C, S // p, p, S // p, p).permute(0, 2, 4, 1, 3, 5).reshape(B * (S // p) ** 2, C * p * p).contiguous()
        B = x.shape[0] // (S // p) ** 2
        return x.reshape(B, S // p, S // p, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, S, S).contiguous()

    def embed_add_silu(self, temb, y, tab, null_row):
        v = temb.clone()
        for b in range(temb.shape[0]):
            cls = -1 if y is None else int(y[b])
            row = cls if cls >= 0 else null_row
            if row >= 0:
                v[b] = v[b] + tab[row]
        return torch.nn.functional.silu(v)


# ------------------------------------------------------------------------------------------------------ cases
def _weights(N, K, g):
    return torch.randn((N, K), generator=g) / K ** 0.5


PERM_SHAPES = [(128, 128, 64), (200, 192, 192), (432, 32, 320), (144, 384, 128)]   # (M, N, K)


@functools.lru_cache(maxsize=None)
def perm_case(M, N, K):
    """Split-exact A, W a selection matrix (one 1.0 per row: output column n = A column perm[n]), no bias: the exact
    output is A[:, perm]. Rows are distinct multiples of 2^-10 plus a column ramp, so any mis-indexed row, column,
    K stage or fragment changes the result."""
    g = torch.Generator().manual_seed(_seed('perm', M, N, K))
    A = split_exact(torch.randn((M, K), generator=g) * 4.0, EA)
    perm = torch.randperm(K, generator=g)[:N] if N <= K else torch.randint(0, K, (N, ), generator=g)
    W = torch.zeros((N, K))
    W[torch.arange(N), perm] = 1.0
    return dict(M=M, A=A, W=W, perm=perm, ea=EA)


LN_BT = [(2, 128), (3, 144), (2, 192)]      # one image per tile; two per tile + a 48-row last tile; a boundary at 64
LN_BT_SMALL = [(9, 16), (3, 64)]            # ln_rows < 128: the plan's own routing at those T
LN_K = [64, 192, 320]
LN_N = [32, 192]


@functools.lru_cache(maxsize=None)
def ln_case(B, T, K, N, dist):
    """qkv / fc1 / final form: LayerNorm + modulate prologue with per-image tables, bias."""
    g = torch.Generator().manual_seed(_seed('ln', B, T, K, N, dist))
    M = B * T
    buf, off = mod_tables(B, K, g, names=('shift', 'scale'))
    return dict(M=M, A=token_rows(dist, M, K, g), W=_weights(N, K, g), bias=torch.randn((N, ), generator=g),
                ln=True, ln_rows=T, mod=buf, mod_off=off, ln_scale=table(buf, off, 'scale', K),
                ln_shift=table(buf, off, 'shift', K), ea=EA)


GATE_CASES = [(16, 64), (16, 192), (144, 64), (144, 192), (128, 64), (128, 192)]   # (gate_rows = T, N), K = 128


@functools.lru_cache(maxsize=None)
def gate_case(T, N, kind='gate'):
    """proj / fc2 form (kind 'gate': C = res + gate[img] (acc + bias), three images), the patch embedding (kind
    'res_mod': a pos_embed-like residual table of T rows, M = 3 T, no gate) and kind 'alpha' (alpha = 0.5, plain
    residual). K = 128."""
    K, B = 128, 3
    g = torch.Generator().manual_seed(_seed('gate', T, N, kind))
    M = B * T
    buf, off = mod_tables(B, N, g, names=('gate', ))
    s = dict(M=M, A=torch.randn((M, K), generator=g), W=_weights(N, K, g), bias=torch.randn((N, ), generator=g), ea=EA)
    if kind == 'gate':
        s.update(res=torch.randn((M, N), generator=g), gate=table(buf, off, 'gate', N), gate_rows=T, gmod=buf, gmod_off=off)
    elif kind == 'res_mod':
        s.update(res=torch.randn((T, N), generator=g) + torch.arange(T, dtype=F32)[:, None], res_mod=T)
    else:
        s.update(res=torch.randn((M, N), generator=g), alpha=0.5)
    return s


ACT_SHAPES = [(256, 64, 64), (432, 192, 192)]   # (M, N, K): fc1 form; M = 2 x 128 and 3 x 144


@functools.lru_cache(maxsize=None)
def act_case(M, N, K, act=2):
    """fc1 form: LN prologue, activation. The bias pushes eight columns of the pre-activation to about +40 and eight
    to about -40 (tanhf / expf saturate there); the rest are N(0, 2). Also the second GEMM of the fc1 -> fc2 chain
    (gate + residual, N2 = 64 columns) on the c_split image."""
    g = torch.Generator().manual_seed(_seed('act', M, N, K, act))
    T = 128 if M % 128 == 0 else 144
    B = M // T
    buf, off = mod_tables(B, K, g, names=('shift', 'scale'))
    A = token_rows('std', M, K, g)
    W = _weights(N, K, g) * 0.5    # LN-modulated rows are O(2): pre-activations about N(0, 2)
    bias = torch.randn((N, ), generator=g)
    cols = torch.randperm(N, generator=g)[:16]
    bias[cols[:8]] = 40.0
    bias[cols[8:]] = -40.0
    s = dict(M=M, A=A, W=W, bias=bias, act=act, ln=True, ln_rows=T, mod=buf, mod_off=off,
             ln_scale=table(buf, off, 'scale', K), ln_shift=table(buf, off, 'shift', K), ea=EA, sat_cols=cols)
    N2 = 64
    gbuf, goff = mod_tables(B, N2, g, names=('gate', ))
    s['fc2'] = dict(M=M, W=_weights(N2, N, g), bias=torch.randn((N2, ), generator=g), res=torch.randn((M, N2), generator=g),
                    gate=table(gbuf, goff, 'gate', N2), gate_rows=T, gmod=gbuf, gmod_off=goff, ea=EA)
    return s


# (B, heads, L, Dh), flags: which plane writer / column order each reaches
PLANE_CASES = [
    ((2, 2, 128, 64), {}),                  # plane_block
    ((1, 4, 256, 72), {}),                  # plane_block, 8-column groups crossing heads
    ((3, 4, 64, 72), {}),                   # plane_slab: two images per tile and a partial third
    ((2, 2, 192, 80), {}),                  # plane_slab: an image boundary mid-tile
    ((2, 4, 64, 32), {'legacy': 1}),
    ((1, 1, 256, 256), {'vonly': 1}),
]


@functools.lru_cache(maxsize=None)
def plane_case(shape, legacy=0, vonly=0, bscale_on=0):
    """qkv form: A [B L, K] N(0, 1) (K = heads Dh rounded up to 64, the weights zero beyond heads Dh), bias,
    ap_alpha = Dh^-0.5, ap_bscale 0 or Dh^-0.25, ea = eb = ev = 6."""
    B, H, L, Dh = shape
    C = H * Dh
    K = (C + 63) // 64 * 64
    N = C if vonly else 3 * C
    g = torch.Generator().manual_seed(_seed('plane', shape, legacy, vonly, bscale_on))
    W = _weights(N, K, g)
    W[:, C:] = 0.0
    ap = dict(L=L, heads=H, Dh=Dh, legacy=legacy, vonly=vonly, alpha=float(torch.tensor(Dh ** -0.5, dtype=F32)),
              bscale=float(torch.tensor(Dh ** -0.25, dtype=F32)) if bscale_on else 0.0, ea=6, eb=6, ev=6)
    return dict(M=B * L, B=B, A=torch.randn((B * L, K), generator=g), W=W, bias=torch.randn((N, ), generator=g) * 0.5,
                ea=EA, ap=ap)


ROWK_ROWS = [5, 64]
ROWK_D = [64, 320, 1152, 1280, 1344, 2048]


@functools.lru_cache(maxsize=None)
def rows_case(rows, D, dist):
    """Row-kernel case: rows of one distribution and per-image modulation tables (3 / 16 rows per image)."""
    g = torch.Generator().manual_seed(_seed('rows', rows, D, dist))
    per = 3 if rows == 5 else 16
    B = (rows + per - 1) // per
    buf, off = mod_tables(B, D, g, names=('shift', 'scale'))
    return dict(x=token_rows(dist, rows, D, g), mod=dict(buf=buf, shift=off['shift'], scale=off['scale'], rows=per),
                ln_scale=table(buf, off, 'scale', D), ln_shift=table(buf, off, 'shift', D), per=per)


def max_scaled_operands(s, stats32):
    """max |A 2^ea| of spec s after the prologue: what the A split sees (tests/test_token_host.py adds the c_split
    image and the planes from the emulation's outputs)."""
    sa, _, _ = a_pieces(s, stats32)
    return sa.abs().max().item()
