"""Host-side references and an emulation of the half-precision token GEMM (DM_MATH_FP16, csrc/linear_h16.hip), on top
of tests/token_ref.py (case builders, distributions, sentinels, REL = 2^-21, EA = 6 are that module's).

The arithmetic: a' = fp16_rne(prologue(a) alpha 2^ea) as ONE plane [M][K]; w' = fp16_rne(w 2^er(row)),
er the per-row power of two of split_conv_weights (token_ref.weight_row_exponents), i.e. piece 0 of the fp16x2 weight
image; acc = sum_k a' w' in fp32, times 2^-(ea + er), then linear_k32's fp32 epilogue.

* exact_case: integer operands in [-8, 8]; a 2^6 and w 2^er are fp16-exact and every partial sum is an integer
  multiple of 2^(6 + er) below 2^24 of them, so the result is exact in fp32 in ANY summation order: the GPU test
  compares bit for bit with float64.
* a_image / w_image / gemm_emulation: the device's roundings restated with .half() and fp32 accumulation in the
  kernel's K order (32 channels per MFMA, the steps in sequence); H16Emu wraps them behind the interface the GPU
  tests' device backend has (tests/test_gpu_token_h16.py), so the checks are dry-run on the CPU
  (tests/test_token_h16_host.py).
* image_bound: what an element of the device's A image may differ from the float64 prologue by -- half an fp16 ulp
  (the one rounding) plus the fp32 prologue's own error, 2 e32 + 2^-21 max|y| as everywhere in the token tests.
* image_refs: the float64 reference and fp32 yardstick of a GEMM ON A GIVEN IMAGE (the device's own a', the host's
  w'): the rounding is in the operands, so the GEMM is held to the fp32 bound of the existing token tests.
* sum_abs: sum_k |a_k w_k| of the unrounded operands, the scale of the distance between the fp16 and the fp16x2 results.
"""
import functools

import torch

from tests import token_ref as tr

F32, F64 = tr.F32, tr.F64
PATH = 3                       # dm_debug_token_gemm's path of linear_h16
H16_REL = 2.0 ** -10 + 2.0 ** -20   # (1 + 2^-11)^2 - 1 rounded up: both operands off by at most 2^-11 relative


# -------------------------------------------------------------------------------------------------------- cases
EXACT_SHAPES = [(128, 128, 64), (200, 192, 192), (432, 32, 320), (144, 384, 128)]   # (M, N, K)


@functools.lru_cache(maxsize=None)
def exact_case(M, N, K):
    """A, W seeded integers in [-8, 8] (fp32). |sum| <= 64 K < 2^24, so A W^T is exact in fp32 in any order. Rows of
    A and rows of W are pairwise distinct (tests/test_token_h16_host.py asserts it, and that no two rows / columns of
    the result agree), so a wrong row, column, K group or fragment lane changes the output."""
    g = torch.Generator().manual_seed(tr._seed('h16-exact', M, N, K))
    A = torch.randint(-8, 9, (M, K), generator=g).float()
    W = torch.randint(-8, 9, (N, K), generator=g).float()
    return dict(M=M, A=A, W=W, ea=tr.EA)


GN_BT = [(3, 144), (2, 192)]   # an image boundary mid-tile
GN_K = [64, 192]


@functools.lru_cache(maxsize=None)
def gn_case(B, T, K, N=32):
    """GroupNorm-affine prologue a * scale[img] + shift[img] with tables [B][K] that differ by O(1) per image."""
    g = torch.Generator().manual_seed(tr._seed('h16-gn', B, T, K, N))
    M = B * T
    img = torch.arange(B, dtype=F32)[:, None]
    scale = 0.5 + torch.rand((B, K), generator=g) + 0.25 * img
    shift = -2.0 + 4.0 * torch.rand((B, K), generator=g) + img
    return dict(M=M, A=torch.randn((M, K), generator=g), W=tr._weights(N, K, g), bias=torch.randn((N, ), generator=g),
                pro=True, pro_scale=scale, pro_shift=shift, pro_rows=T, ea=tr.EA)


WIDE_SHAPES = [(144, 192, 1280), (144, 1280, 64)]   # D = 1280 as K (20 stages) and as N (10 column tiles)


@functools.lru_cache(maxsize=None)
def wide_case(M, N, K):
    g = torch.Generator().manual_seed(tr._seed('h16-wide', M, N, K))
    return dict(M=M, A=torch.randn((M, K), generator=g), W=tr._weights(N, K, g), bias=torch.randn((N, ), generator=g),
                res=torch.randn((M, N), generator=g), ea=tr.EA)


# ------------------------------------------------------------------------------------------------- arithmetic
def prologue(s, stats32, dtype):
    """token_ref.prologue plus the GroupNorm affine (h16_image_kernel<1>: a * scale + shift, separately rounded)."""
    if s.get('pro'):
        img = torch.arange(s['A'].shape[0]) // s['pro_rows']
        a = s['A'].to(dtype) * s['pro_scale'].to(dtype)[img] + s['pro_shift'].to(dtype)[img]
        if s.get('alpha', 1.0) != 1.0:
            a = a * torch.tensor(s['alpha'], dtype=F32).to(dtype)
        return a
    return tr.prologue(s, stats32, dtype)


def a_image(s, stats32=None):
    """-> (a' fp16 [M, K], flag): the fp32 prologue in the kernels' expressions, 2^ea, one rounding."""
    sa = torch.ldexp(prologue(s, stats32, F32), torch.tensor(s['ea']))
    return sa.to(torch.float16), int((sa.abs() > tr.FP16_MAX).any())


def w_image(W):
    """-> (w' fp16 [N, K], er int32 [N]): piece 0 of split_conv_weights' fp16x2 image."""
    e = tr.weight_row_exponents(W)
    return torch.ldexp(W, e[:, None]).to(torch.float16), e


def w_rounded(W):
    """w' 2^-er as fp32 (exact): the weights the half-precision GEMM actually multiplies by."""
    w16, e = w_image(W)
    return torch.ldexp(w16.to(F32), -e[:, None])


def acc_h16(a16, w16):
    """sum_k a' w' in fp32, 32 channels per MFMA step, the steps in sequence."""
    M, K = a16.shape
    acc = torch.zeros((M, w16.shape[0]), dtype=F32)
    a, w = a16.to(F32), w16.to(F32)
    for k in range(0, K, 32):
        acc = acc + a[:, k:k + 32] @ w[:, k:k + 32].T
    return acc


def gemm_emulation(s, stats32=None, a16=None):
    """-> dict(y fp32 [M, N] after the epilogue, a16, flag)."""
    flag = 0
    if a16 is None:
        a16, flag = a_image(s, stats32)
    w16, e = w_image(s['W'])
    y = acc_h16(a16, w16) * torch.ldexp(torch.ones(w16.shape[0]), -e - s['ea'])[None, :]
    return dict(y=tr.epilogue(y, s, F32), a16=a16, flag=flag)


def ulp16(x):
    """The spacing of fp16 at |x| (float64; the subnormal spacing 2^-24 below 2^-14)."""
    _, ex = torch.frexp(x.abs().clamp_min(2.0 ** -14))
    return torch.ldexp(torch.ones_like(x), ex - 11)


def image_bound(s, stats32):
    """-> (y64 [M, K] the float64 prologue (alpha included), bound [M, K] on |decoded image - y64|, e32, scale)."""
    y = prologue(s, stats32, F64)
    e32 = (prologue(s, stats32, F32).double() - y).abs().max().item()
    scale = y.abs().max().item()
    pro = 2.0 * e32 + tr.REL * scale
    ea = s['ea']
    # the ulp at |y| + the prologue error: a value just below a binade may be rounded in the one above
    half = 0.5 * ulp16((y.abs() + pro) * 2.0 ** ea) * 2.0 ** -ea
    return y, half + pro, e32, scale


def decode_image(img16, M, K, ea):
    """int16 bits of the plane [M][K] -> float64 a' 2^-ea."""
    return torch.ldexp(img16[:M * K].view(torch.float16).view(M, K).double(), torch.tensor(-ea))


def image_refs(s, a64):
    """The GEMM of spec s on the image a64 (float64 [M, K], a' 2^-ea) against the host's w': token_ref.gemm_refs'
    dict (ref, e32, scale, base, bound)."""
    return tr.gemm_refs(dict(s, W=w_rounded(s['W'])), a64=a64)


def sum_abs(s, stats32=None):
    """sum_k |a_k w_k| [M, N] of the unrounded operands (float64 prologue, fp32 weights)."""
    return prologue(s, stats32, F64).abs() @ s['W'].double().abs().T


def epilogue_slope(s):
    """|d out / d acc| of the epilogue, per element broadcastable to [M, N]: the gate, 1.13 behind an activation."""
    f = torch.ones((s['M'], 1), dtype=F64)
    if s.get('gate') is not None:
        f = s['gate'].double()[torch.arange(s['M']) // s['gate_rows']].abs()
    return f * (1.13 if s.get('act', 0) else 1.0)


# ------------------------------------------------------------------------------------------------ the backend
class H16Emu(tr.EmuBackend):
    """token_ref.EmuBackend with path 3 answered by the half-precision emulation: the images are single planes
    ((M + TILE) K and (M + TILE) N int16, sentinel past row M)."""
    name = 'h16-emulation'

    def gemm(self, s, stats32=None):
        if s.get('path', 0) != PATH:
            return super().gemm(s, stats32)
        M, (N, K) = s['M'], s['W'].shape
        a_form = s.get('a_form', 0)
        out = dict(C=None, as_img=None, c_img=None, planes=None, flag=0, rc=0)
        if a_form == 1:
            out['as_img'] = tr.sentinel_image((M + tr.TILE) * K)
        if s.get('ap'):
            ap = s['ap']
            n = (M // ap['L']) * ap['heads'] * 2 * ap['L'] * ap['Dh']
            out['planes'] = tuple(tr.sentinel_image(n + tr.PLANE_TAIL) for _ in range(3))
        elif s.get('c_split'):
            out['c_img'] = tr.sentinel_image((M + tr.TILE) * N)
        else:
            out['C'] = torch.full((M + tr.TILE, N + tr.PAD), float('nan'))
        # linear_h16_ok: K % 64, N % 4, a 16-byte aligned image, c_split only onto a K % 64 plane; no split-K
        if (K % 64 != 0 or N % 4 != 0 or s.get('sk') or s.get('as_misalign') or (s.get('c_split') and N % 64 != 0)):
            out['rc'] = -4
            return out
        a16 = None
        if a_form == 2:
            a16 = s['as_img'][:M * K].view(torch.float16).view(M, K)
        e = gemm_emulation(s, stats32, a16)
        out['flag'] |= e['flag']
        if a_form == 1:
            out['as_img'][:M * K] = e['a16'].reshape(-1).view(torch.int16)
        if s.get('ap'):
            import tests.attention_ref as ar
            ap = s['ap']
            B = M // ap['L']
            parts = tr.rows_to_heads(e['y'], ap, B)
            sc = tr.plane_scales(ap)
            exps = (ap['ea'], ap['eb'], ap['ev'])
            for p in range(3):
                if parts[p] is None:
                    continue
                n = B * ap['heads'] * 2 * ap['L'] * ap['Dh']
                y = parts[p] * torch.tensor(sc[p], dtype=F32) if sc[p] != 1.0 else parts[p]
                out['flag'] |= int((torch.ldexp(y, torch.tensor(exps[p])).abs() > tr.FP16_MAX).any())
                hi, lo = ar.split_planes(y, exps[p])
                if p == 2:
                    hi, lo = hi.transpose(-1, -2), lo.transpose(-1, -2)
                out['planes'][p][:n] = torch.stack([hi, lo], dim=2).contiguous().view(-1).view(torch.int16)
        elif s.get('c_split'):
            sc = torch.ldexp(e['y'], torch.tensor(s['c_split_ea']))
            out['flag'] |= int((sc.abs() > tr.FP16_MAX).any())
            out['c_img'][:M * N] = sc.to(torch.float16).reshape(-1).view(torch.int16)
        else:
            out['C'][:M, :N] = e['y']
        return out


# ------------------------------------------------------------------------------------ model-level emulation
COVERED = ('.attn.qkv.weight', '.attn.proj.weight', '.mlp.fc1.weight', '.mlp.fc2.weight', '.skip_linear.weight',
           'final_layer.linear.weight')   # the layers the plan covers (the adaLN GEMM is left: dit_exec.hip)


def round_a(x, ea=tr.EA):
    """fp16_rne(x 2^ea) 2^-ea, in x's dtype (the fp32 rounding of x first: the engine's prologue is fp32)."""
    s = torch.ldexp(x.to(F32), torch.tensor(ea)).to(torch.float16)
    return torch.ldexp(s.to(F64), torch.tensor(-ea)).to(x.dtype)


class h16_linear:
    """Context manager that replaces torch.nn.functional.linear while a HOST forward runs (oracle/dit.py's, or
    mdt_forward below): on the layers of `sd` whose names end in COVERED the input and the weight are rounded to
    fp16 as the engine rounds them (2^6 / the per-row power of two) and multiplied in the forward's own dtype
    (float64 for the emulation); every other layer is untouched. The oracle's code is not edited."""

    def __init__(self, sd):
        self.rounded = {id(v): w_rounded(v.to(F32)).to(v.dtype) for k, v in sd.items() if k.endswith(COVERED)}
        self.calls = 0

    def __enter__(self):
        import torch.nn.functional as F
        self._F, self._orig = F, F.linear

        def linear(x, w, b=None):
            r = self.rounded.get(id(w))
            if r is None:
                return self._orig(x, w, b)
            self.calls += 1
            return self._orig(round_a(x), r, b)

        F.linear = linear
        return self

    def __exit__(self, *exc):
        self._F.linear = self._orig
        return False


def mdt_forward(sd, x, t, y, arch):
    """Host MDTv2 inference forward over a state_dict (models/mdt/model.py's parameter names; the topology of
    csrc/dit_exec.hip's plan: en_inblocks keep their outputs as skips, en_outblocks pop them last in first out,
    + decoder_pos_embed, de_blocks take the embedded input as their skip), built from oracle/dit.py's pieces. Checked
    against the reference fixture tests/golden/mdt.npz in tests/test_token_h16_host.py."""
    import torch.nn.functional as F
    from models.mdt.model import relative_position_index
    from oracle import dit as od
    heads, p, D = arch['num_heads'], arch['patch_size'], arch['hidden_size']
    hd = (arch['depth'] - arch['decode_layer']) // 2
    if y is None:
        y = torch.full((x.shape[0], ), arch['num_classes'], dtype=torch.long)
    h = F.conv2d(x, sd['x_embedder.proj.weight'], sd['x_embedder.proj.bias'], stride=p).flatten(2).transpose(1, 2)
    h = h + sd['pos_embed']
    te = od._lin(sd, 't_embedder.mlp.2', F.silu(od._lin(sd, 't_embedder.mlp.0', od.timestep_embedding(t, 256).to(h.dtype))))
    c = te + F.embedding(y, sd['y_embedder.embedding_table.weight'])
    T = h.shape[1]
    index = relative_position_index(int(T ** 0.5))

    def attention(pre, z):
        B, N, C = z.shape
        d = C // heads
        qkv = od._lin(sd, pre + '.qkv', z).reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
        q, k, v = qkv.unbind(0)
        bias = sd[pre + '.rel_pos_bias.relative_position_bias_table'][index.reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)
        a = ((q * d ** -0.5) @ k.transpose(-2, -1) + bias.unsqueeze(0)).softmax(dim=-1)
        return od._lin(sd, pre + '.proj', (a @ v).transpose(1, 2).reshape(B, N, C))

    def block(pre, z, skip=None):
        if skip is not None:
            z = od._lin(sd, pre + '.skip_linear', torch.cat([z, skip], dim=-1))
        m = od._lin(sd, pre + '.adaLN_modulation.1', F.silu(c)).chunk(6, dim=1)
        z = z + m[2].unsqueeze(1) * attention(pre + '.attn', od.modulate(F.layer_norm(z, (D, ), eps=1e-6), m[0], m[1]))
        return z + m[5].unsqueeze(1) * od.mlp(sd, pre + '.mlp', od.modulate(F.layer_norm(z, (D, ), eps=1e-6), m[3], m[4]))

    x0, skips = h, []
    for i in range(hd):
        h = block(f'en_inblocks.{i}', h)
        skips.append(h)
    for i in range(hd):
        h = block(f'en_outblocks.{i}', h, skips.pop())
    h = h + sd['decoder_pos_embed']
    for i in range(arch['decode_layer']):
        h = block(f'de_blocks.{i}', h, x0)
    shift, scale = od._lin(sd, 'final_layer.adaLN_modulation.1', F.silu(c)).chunk(2, dim=1)
    h = od._lin(sd, 'final_layer.linear', od.modulate(F.layer_norm(h, (D, ), eps=1e-6), shift, scale))
    n, oc = h.shape[0], arch['in_channels'] * (2 if arch['learn_sigma'] else 1)
    s = int(T ** 0.5)
    return torch.einsum('nhwpqc->nchpwq', h.reshape(n, s, s, p, p, oc)).reshape(n, oc, s * p, s * p)


def host_forward(kind, sd, arch, x, t, y, dtype=F64, h16=False):
    """The host forward of a 'dit' (oracle/dit.py) or 'mdt' (mdt_forward) model in `dtype`; h16: under h16_linear.
    -> (output float64, the number of covered GEMMs that ran)."""
    from oracle import dit as od
    sdd = {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in sd.items()}
    x = x.detach().cpu().to(dtype)
    t, y = t.detach().cpu(), None if y is None else y.detach().cpu()

    def run():
        with torch.no_grad():
            if kind == 'mdt':
                return mdt_forward(sdd, x, t, y, arch)
            return od.dit_forward(sdd, x, t, y, arch['patch_size'], arch['num_heads'], arch['depth'], arch['num_classes'],
                                  arch['in_channels'] * (2 if arch['learn_sigma'] else 1))
    if not h16:
        return run().double(), 0
    with h16_linear(sdd) as ctx:
        out = run()
    return out.double(), ctx.calls


def covered_gemms(kind, arch):
    """The number of GEMMs DM_MATH_FP16 covers in one forward: 4 per block, one per skip_linear, the final layer."""
    if kind == 'mdt':
        hd = (arch['depth'] - arch['decode_layer']) // 2
        blocks = 2 * hd + arch['decode_layer']
        return 4 * blocks + (hd + arch['decode_layer']) + 1
    return 4 * arch['depth'] + 1
