"""Operands that make the split convolutions bit-exact with every piece non-zero, CPU emulations of the splits and
transforms, the exactness budget, and the case table of tests/test_gpu_conv_split_pieces.py. Host only.

The integer-exact conv tests use operands in [-2, 3): their low pieces are zero, so the addressing of the low
pieces (LDS piece slots, the piece planes of split_conv_weights_kernel, the Winograd loader's low halves, the a[1] /
b[1] MFMA operands) is not pinned by them. The families here keep exactness and fill the low pieces:

G16   x = a + b 2^-14, a a non-zero integer with |a| <= 2, b a non-zero integer with |b| <= 3. fp16(x) = a and the
      low piece is b 2^-14 exactly (Split<2>::split). Sums and differences of a few such values (the Winograd
      V = B^T d, U = G g, the sub-pixel weight sums) stay A + B 2^-14 with small A, B and split exactly too, under
      any power-of-two row scale.
G3    x = a + b 2^-11 (two bf16 pieces) or a + b 2^-11 + c 2^-22 (three), b != 0: Split<3>::split returns them.
P16   x = hi + lo with hi any normal fp16 and |lo| <= 0.45 ulp_fp16(hi) on fp16's grid: arbitrary significands.
      With |x| < 2^-3 the low piece is an fp16 subnormal (the absolute floor conv_patch3.hip's header speaks of).

Budget. A case is admissible only if, for every fp32 accumulation the kernel performs, the sum of |terms| times 2^s
is below 2^24, s the finest bit in play (14 for G16 against integers, 15 through the Winograd halves, 11 for two-piece
G3) -- taken relative to the output row's unit where the weights carry a row scale 2^k. Every term is a multiple of
2^-s and every partial sum, in any order, is below 2^(24 - s): each is representable, no addition rounds, and the
result equals the float64 reference bit for bit. A condition on the inputs (asserted per case by
tests/test_split_operands_host.py), not a tolerance."""
import functools
import types

import torch
import torch.nn.functional as F

S16, S3, SWINO = 14, 11, 15


# ------------------------------------------------------------------------------------------------ split emulations
def split2(x):
    """Split<2>::split: (fp16(x), fp16(x - fp16(x)))."""
    h = x.half()
    return h, (x - h.float()).half()


def split3(x):
    """Split<3>::split: three bf16 roundings of the running remainder."""
    b0 = x.bfloat16()
    r1 = x - b0.float()
    b1 = r1.bfloat16()
    return b0, b1, (r1 - b1.float()).bfloat16()


def pieces(x, kind):
    return split2(x) if kind == 'fp16x2' else split3(x)


def row_scale(w):
    """split_row_scale_kernel: w [nmat, rows, K] -> 2^e per row with max |w| 2^e in [2^13, 2^14) over all matrices
    (1 for an all-zero row)."""
    m = w.abs().amax(dim=(0, 2))
    ex = torch.frexp(m).exponent  # m in [2^(ex - 1), 2^ex)
    e = (14 - ex).clamp(-126, 126)
    return torch.where(m > 0, torch.ldexp(torch.ones_like(m), e), torch.ones_like(m))


# the products Split<NP>::mma issues, as (activation piece, weight piece)
PRODUCTS = {'fp16x2': [(1, 0), (0, 1), (0, 0)], 'bf16x3': [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]}


def emulate_conv(x, w, kind, drop=None):
    """fp32 emulation of the 3x3 (padding 1) split contraction: per tap the piece products Split<NP>::mma issues,
    summed in fp32 (exact under the budget in any order). drop = ('x' | 'w', tap, channel) zeroes the low piece (piece
    1) of that operand for that tap and input channel -- the planted error of the host tests."""
    B, C, H, W = x.shape
    xp = [F.pad(p.float(), (1, 1, 1, 1)) for p in pieces(x, kind)]
    if kind == 'fp16x2':
        sc = row_scale(w.reshape(1, w.shape[0], -1))
        wp = [p.float() for p in pieces(w * sc[:, None, None, None], kind)]
    else:
        sc = torch.ones(w.shape[0])
        wp = [p.float() for p in pieces(w, kind)]
    acc = torch.zeros((B, w.shape[0], H, W))
    for tap in range(9):
        dy, dx = divmod(tap, 3)
        for ia, ib in PRODUCTS[kind]:
            a = xp[ia][:, :, dy:dy + H, dx:dx + W]
            b = wp[ib][:, :, dy, dx]
            if drop is not None and drop[1] == tap:
                if drop[0] == 'x' and ia == 1:
                    a = a.clone()
                    a[:, drop[2]] = 0
                if drop[0] == 'w' and ib == 1:
                    b = b.clone()
                    b[:, drop[2]] = 0
            acc = acc + torch.einsum('bchw,oc->bohw', a, b)
    return acc / sc[None, :, None, None]


# ---------------------------------------------------------------------------------------- Winograd F(2,3) along x
def wino_V(x):
    """V = B^T d per pixel pair: x [B, C, H, W] -> [4, B, C, H, W / 2] (zero padding outside the map)."""
    W = x.shape[-1]
    xp = F.pad(x, (1, 1))
    d0, d1, d2, d3 = xp[..., 0:W:2], xp[..., 1:W + 1:2], xp[..., 2:W + 2:2], xp[..., 3:W + 2:2]
    return torch.stack([d0 - d2, d1 + d2, d2 - d1, d1 - d3])


def wino_U(w):
    """U = G g in float64 per tap row: w [Cout, Cin, 3, 3] -> [4, Cout, Cin, 3]."""
    g0, g1, g2 = w.double().unbind(-1)
    return torch.stack([g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2])


def wino_m(V, U):
    """m_nu = sum over (c, dy) of V_nu U_nu: [4, B, Cout, H, W / 2] (float64)."""
    return torch.stack([F.conv2d(V[n].double(), U[n].double()[..., None], padding=(1, 0)) for n in range(4)])


def wino_out(m):
    """y0 = m0 + m1 + m2, y1 = m1 - m2 - m3, interleaved back to pixels."""
    y0, y1 = m[0] + m[1] + m[2], m[1] - m[2] - m[3]
    return torch.stack([y0, y1], dim=-1).flatten(-2)


def wino_shortcut_m(x2, ws):
    """The 1x1 shortcut in the pair domain (wino_pack_kernel): channels in halves H1, H2; nu 0 takes Ws_H1 x2[2j], nu 3
    -Ws_H1 x2[2j + 1], nu 1 / 2 Ws_H2 / 2 against x2[2j] +/- x2[2j + 1]. Returns ([4] V, [4] U)."""
    hh = x2.shape[1] // 2
    e, o = x2[..., 0::2], x2[..., 1::2]
    w = ws.double()[:, :, 0, 0]
    V = [e[:, :hh], e[:, hh:] + o[:, hh:], e[:, hh:] - o[:, hh:], o[:, :hh]]
    U = [w[:, :hh], 0.5 * w[:, hh:], 0.5 * w[:, hh:], -w[:, :hh]]
    return V, U


# ------------------------------------------------------------------------------------------------ operand families
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nonzero_ints(shape, amax, g):
    a = torch.randint(1, amax + 1, shape, generator=g)
    return (a * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def g16(shape, seed, amax=2, bmax=3):
    g = _gen(seed)
    return _nonzero_ints(shape, amax, g) + _nonzero_ints(shape, bmax, g) * 2.0 ** -14


def g3(shape, seed, npieces=2, amax=2, bmax=3):
    g = _gen(seed)
    x = _nonzero_ints(shape, amax, g) + _nonzero_ints(shape, bmax, g) * 2.0 ** -11
    if npieces == 3:
        x = x + _nonzero_ints(shape, bmax, g) * 2.0 ** -22
    return x


def grid(kind, shape, seed):
    return g16(shape, seed) if kind == 'fp16x2' else g3(shape, seed)


def sparse_ints(shape, seed, density):
    """Integers in {-1, 0, 1}, non-zero with probability `density`."""
    g = _gen(seed)
    v = _nonzero_ints(shape, 1, g)
    return v * (torch.rand(shape, generator=g) < density).float()


def p16(shape, seed, lo_exp=-2, hi_exp=3):
    """hi + lo: hi an fp16 with a random 11-bit significand and exponent in [lo_exp, hi_exp), lo = k grid with
    |lo| <= 0.45 ulp(hi), grid = max(ulp 2^-11, 2^-24) (fp16's subnormal spacing): both pieces exact in fp16 and the sum
    exact in fp32. hi_exp <= -3: every low piece is an fp16 subnormal."""
    g = _gen(seed)
    e = torch.randint(lo_exp, hi_exp, shape, generator=g)
    sig = torch.randint(1025, 2048, shape, generator=g).double() / 1024  # not 1.0: the ulp halves just below it
    sign = (2 * torch.randint(0, 2, shape, generator=g) - 1).double()
    hi = sign * torch.ldexp(sig, e)
    ulp = torch.ldexp(torch.ones(shape, dtype=torch.float64), e - 10)
    grd = torch.maximum(ulp * 2.0 ** -11, torch.full_like(ulp, 2.0 ** -24))
    kmax = torch.floor(0.45 * ulp / grd)
    k = torch.floor((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * kmax)
    k = torch.where(k == 0, torch.ones_like(k), k)
    x = hi + k * grd
    assert torch.equal(x.float().double(), x)
    return x.float()


def p16_rows(Cout, K, seed):
    """P16-style weight rows already in the row-scaled domain: per row one element in [2^13, 2^14), the others spread
    down to 2^-3 (more than 2^16 below the maximum: their low pieces are fp16 subnormals), then the row times a power
    of two in [2^-30, 2^-4] so the packer's row scale has to undo it. Row 1 is all zero."""
    g = _gen(seed)
    e = torch.randint(-3, 13, (Cout, K), generator=g)
    e[torch.arange(Cout), torch.randint(0, K, (Cout, ), generator=g)] = 13
    w = torch.empty((Cout, K), dtype=torch.float64)
    for lo in range(-3, 14):  # one p16 draw per binade
        v = p16((Cout, K), seed + 100 + lo, lo, lo + 1).double()
        w = torch.where(e == lo, v, w)
    k = torch.linspace(-30, -4, Cout).round()
    w = w * torch.ldexp(torch.ones(Cout, dtype=torch.float64), k.int())[:, None]
    w[1] = 0
    assert torch.equal(w.float().double(), w)
    return w.float()


# ------------------------------------------------------------------------------------------------------- the cases
def _label_patch3(tile, form, np_, maxp=None):
    dims = {4: '128,128,64,64', 5: '128,64,64,32', 6: '64,64,32,32', 7: '256,256,128,128', 8: '512,128,128,128',
            9: '128,128,64,64'}[tile]
    mode = {'plain': 0, 'seg': 0, 'up1': 1, 'sub': 2, 's2': 4}[form]
    mp = 384 if form == 's2' else {6: 160, 7: 352, 8: 656, 9: 392}.get(tile, 208)
    return f'conv_patch3_kernel<{dims},{mode},{mp},false,false,{np_}>'


def _label_k32(tile, form, pro=False):
    p, sub = ('true' if pro else 'false'), ('true' if form == 'sub' else 'false')
    return {10: f'conv_k32_kernel<128,128,64,64,{p},false,{sub}>', 11: f'conv_k32_kernel<128,64,64,32,{p},false,{sub}>',
            12: f'conv_k32_kernel<64,64,32,32,{p},true,false>', 13: f'conv_k32_kernel<64,128,32,64,{p},true,false>',
            14: f'conv_k32_kernel<64,128,32,64,{p},false,{sub}>', 15: f'conv_k32s_kernel<{p},8>',
            16: f'conv_k32_kernel<128,128,64,32,{p},false,{sub},512>',
            17: f'conv_k32_kernel<128,128,64,64,{p},false,{sub},256,208,8192>',
            18: f'conv_k32_kernel<64,128,32,32,{p},false,false,512,392,2048,true>',
            19: f'conv_k32_kernel<128,128,64,64,{p},false,{sub},256,208,2048,false,true>',
            22: f'conv_k32_kernel<64,128,32,32,{p},false,false,512,392,2048,true>'}[tile]


def _label_wino(W, pro, sc):
    s = 'true' if sc else 'false'
    return f'conv_wino_wide_kernel<{int(pro)},{s}>' if W > 32 else f'conv_wino_kernel<{W},{int(pro)},{s}>'


def _case(kernel, tile, kind, form, B, C1, Cout, H, W=None, C2=0, ksplit=0, pro=False, pitch=False, label=None):
    W = W or H
    cid = f'{kernel}-t{tile}-{kind}-{form}-{B}x{C1}' + (f'+{C2}' if C2 else '') + f'x{Cout}x{H}x{W}' + \
        (f'-ks{ksplit}' if ksplit else '') + ('-pro' if pro else '') + ('-pitch' if pitch else '')
    return dict(id=cid, kernel=kernel, tile=tile, kind=kind, form=form, B=B, C1=C1, C2=C2, Cout=Cout, H=H, W=W,
                ksplit=ksplit, pro=pro, pitch=pitch, label=label)


def _direct_cases():
    cs = []
    for kind, np_ in (('fp16x2', 2), ('bf16x3', 3)):
        for tile in (4, 5, 6):
            lab = functools.partial(_label_patch3, tile, np_=np_)
            cs.append(_case('patch3', tile, kind, 'plain', 2, 32, 64, 8, label=lab('plain')))
            cs.append(_case('patch3', tile, kind, 'plain', 3, 32, 96, 16, label=lab('plain')))
            cs.append(_case('patch3', tile, kind, 'seg', 3, 64, 64, 8, C2=32, pitch=True, label=lab('seg')))
            if tile != 5:
                cs.append(_case('patch3', tile, kind, 'up1', 2, 32, 64, 8, label=lab('up1')))
                cs.append(_case('patch3', tile, kind, 'sub', 2, 32, 64, 8, label=lab('sub')))
        cs.append(_case('patch3', 6, kind, 'plain', 5, 64, 64, 4, label=_label_patch3(6, 'plain', np_)))
        # the automatic pick (bf16x3 stays on conv_patch3; fp16x2 moves to conv_k32 where it takes the shape)
        cs.append(_case('auto', 0, kind, 'plain', 2, 32, 64, 8))
        cs.append(_case('auto', 0, kind, 'seg', 3, 64, 64, 8, C2=32, pitch=True))
    k = 'fp16x2'
    cs.append(_case('patch3', 7, k, 'plain', 1, 32, 64, 16, label=_label_patch3(7, 'plain', 2)))
    cs.append(_case('patch3', 8, k, 'plain', 2, 32, 64, 16, label=_label_patch3(8, 'plain', 2)))
    cs.append(_case('patch3', 9, k, 'plain', 1, 32, 64, 4, 256, label=_label_patch3(9, 'plain', 2)))
    cs.append(_case('patch3', 9, k, 'plain', 1, 32, 32, 2, 512, label=_label_patch3(9, 'plain', 2)))
    cs.append(_case('patch3', 9, k, 'seg', 2, 64, 64, 3, 256, C2=32, label=_label_patch3(9, 'seg', 2)))
    cs.append(_case('patch3', 6, k, 's2', 2, 32, 64, 32, label=_label_patch3(6, 's2', 2)))
    cs.append(_case('patch3', 6, k, 's2', 5, 64, 64, 8, label=_label_patch3(6, 's2', 2)))
    pw = 'conv_patch3_kernel<128,64,64,32,3,128,false,false,2>'
    cs.append(_case('patch3', 0, k, 'pw', 2, 64, 96, 16, pitch=True, label=pw))
    cs.append(_case('patch3', 0, k, 'pw', 3, 96, 40, 5, pitch=True, label=pw))
    for tile in (10, 11):
        lab = functools.partial(_label_k32, tile)
        cs.append(_case('k32', tile, k, 'plain', 2, 32, 64, 16, label=lab('plain')))
        cs.append(_case('k32', tile, k, 'plain', 1, 96, 96, 32, label=lab('plain')))
        cs.append(_case('k32', tile, k, 'plain', 3, 64, 64, 8, label=lab('plain')))
        cs.append(_case('k32', tile, k, 'seg', 3, 64, 64, 16, C2=32, pitch=True, label=lab('seg')))
    cs.append(_case('k32', 10, k, 'sub', 3, 64, 64, 16, label=_label_k32(10, 'sub')))
    for tile in (12, 13):
        for ks in (2, 4):
            cs.append(_case('k32', tile, k, 'plain', 3, 128, 64, 4, ksplit=ks, label=_label_k32(tile, 'plain')))
    for tile in (14, 16):
        cs.append(_case('k32', tile, k, 'plain', 2, 64, 128, 64, label=_label_k32(tile, 'plain')))
        cs.append(_case('k32', tile, k, 'plain', 1, 32, 64, 128, label=_label_k32(tile, 'plain')))
    cs.append(_case('k32', 15, k, 'plain', 3, 128, 64, 4, ksplit=2, label=_label_k32(15, 'plain')))
    cs.append(_case('k32', 15, k, 'plain', 5, 256, 256, 4, ksplit=2, label=_label_k32(15, 'plain')))
    cs.append(_case('k32', 17, k, 'plain', 3, 128, 64, 16, label=_label_k32(17, 'plain')))
    cs.append(_case('k32', 18, k, 's2', 2, 32, 64, 32, label=_label_k32(18, 's2')))
    cs.append(_case('k32', 18, k, 's2', 1, 96, 160, 32, label=_label_k32(18, 's2')))
    cs.append(_case('k32', 19, k, 'plain', 2, 64, 96, 8, 64, label=_label_k32(19, 'plain')))
    cs.append(_case('k32', 19, k, 'plain', 3, 32, 128, 4, 96, label=_label_k32(19, 'plain')))
    cs.append(_case('k32', 19, k, 'sub', 1, 32, 64, 4, 64, label=_label_k32(19, 'sub')))
    cs.append(_case('k32', 19, k, 'seg', 2, 64, 64, 8, 128, C2=32, pitch=True, label=_label_k32(19, 'seg')))
    cs.append(_case('k32', 22, k, 's2pad0', 1, 32, 64, 4, 256, pitch=True, label=_label_k32(22, 's2')))
    cs.append(_case('k32', 22, k, 's2pad0', 2, 64, 160, 8, 256, pitch=True, label=_label_k32(22, 's2')))
    return cs


def _wino_cases():
    k, cs = 'fp16x2', []
    w = lambda *a, **kw: cs.append(_case('wino', 21, k, *a, **kw))  # noqa: E731
    w('plain', 2, 32, 128, 32, label=_label_wino(32, 0, 0))
    w('plain', 3, 64, 256, 16, label=_label_wino(16, 0, 0))
    w('plain', 3, 64, 128, 8, label=_label_wino(8, 0, 0))
    w('epi', 3, 64, 128, 16, pitch=True, label=_label_wino(16, 0, 0))
    for pro in (False, True):  # wide 4 x 32 tiles: the halo columns at the tile seams come from the edge buffer
        w('plain', 1, 64, 128, 8, 64, pro=pro, label=_label_wino(64, pro, 0))
        w('plain', 2, 32, 128, 12, 96, pro=pro, label=_label_wino(96, pro, 0))
        w('plain', 11, 128, 256, 4, ksplit=4, pro=pro, label=_label_wino(4, pro, 0))
    w('epi', 3, 64, 128, 4, 96, pitch=True, label=_label_wino(96, 0, 0))
    w('plain', 1, 64, 128, 4, ksplit=2, label=_label_wino(4, 0, 0))
    w('seg', 2, 64, 128, 32, C2=64, label=_label_wino(32, 0, 1))
    w('seg', 2, 64, 128, 32, C2=128, pro=True, label=_label_wino(32, 1, 1))
    w('seg', 2, 128, 256, 8, C2=128, pro=True, label=_label_wino(8, 1, 1))
    w('seg', 2, 64, 128, 8, 64, C2=64, label=_label_wino(64, 0, 1))
    w('seg', 10, 64, 128, 4, C2=64, ksplit=2, pro=True, label=_label_wino(4, 1, 1))
    return cs


DIRECT = _direct_cases()
WINO = _wino_cases()
# (case, side): 'act' = low pieces in the activations, 'wgt' = in the weights (row scales 2^k), 'both' = both (the
# fp16x2 direct kernels only: bf16x3 keeps its a1 b1 term, which breaks the budget; Winograd: U, V products)
CASES = [(c, s) for c in DIRECT for s in ('act', 'wgt') + (('both', ) if c['kind'] == 'fp16x2' and c['form'] in
                                                           ('plain', 'seg', 's2') and c['C1'] <= 64 else ())]
CASES += [(c, s) for c in WINO for s in ('act', 'wgt')]
CASE_IDS = [f"{c['id']}-{s}" for c, s in CASES]

ZERO_ROW, SUB_ROW, ZERO_CH = 1, 2, 5  # 'wgt': an all-zero row; a row 2^-17 below its maximum, which meets x[:, 5] = 0


def _conv_ref(form, x, w, bias=None, stride=1):
    if form in ('up1', 'sub'):
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    if form == 's2pad0':
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, bias, stride=2)
    if form == 'pw':
        return F.conv2d(x, w, bias)
    return F.conv2d(x, w, bias, stride=2 if form == 's2' else 1, padding=1)


@functools.lru_cache(maxsize=4)
def build(idx):
    """Operands (fp32, NCHW), float64 reference, fp32 reference and the budget figure of CASES[idx]."""
    c, side = CASES[idx]
    kind, form, wino = c['kind'], c['form'], c['kernel'] == 'wino'
    B, C1, C2, Cout, H, W = c['B'], c['C1'], c['C2'], c['Cout'], c['H'], c['W']
    taps = 1 if form == 'pw' else 9
    kh = 1 if form == 'pw' else 3
    seed = 1000 + 17 * idx
    s = SWINO if wino else (S16 if kind == 'fp16x2' else S3)
    # non-zero terms per accumulation: near 288 on the direct kernels (limit 2^10 at mean |term| 1.5); per Winograd
    # m_nu (limit 2^9, |V| up to 4, three m_nu per output) near 48, 16 where the prologue x -> 2 x - 1 doubles |V|
    kterms = (3 if wino else taps) * C1 + (C2 // 2 if wino else C2)
    nterm = 288 if not wino else 40 if side == 'wgt' else 16 if c['pro'] else 48
    dens = min(1.0, nterm / kterms)
    o = types.SimpleNamespace(case=c, side=side, s=s, x2=None, ws=None, rv=None, res=None, pro=None)
    G = functools.partial(grid, kind)
    unit = torch.ones(Cout, dtype=torch.float64)
    if side == 'act':
        o.x = G((B, C1, H, W), seed)
        o.w = sparse_ints((Cout, C1, kh, kh), seed + 1, dens)
        if C2:
            o.x2, o.ws = G((B, C2, H, W), seed + 2), sparse_ints((Cout, C2, 1, 1), seed + 3, dens)
    else:
        lowx = side == 'both'
        o.x = G((B, C1, H, W), seed) if lowx else sparse_ints((B, C1, H, W), seed, dens)
        o.w = G((Cout, C1, kh, kh), seed + 1)
        if lowx:
            o.w = o.w * (torch.rand(o.w.shape, generator=_gen(seed + 9)) < dens * 0.75).float()
        if C2:
            o.x2 = G((B, C2, H, W), seed + 2) if lowx else sparse_ints((B, C2, H, W), seed + 2, dens)
            o.ws = G((Cout, C2, 1, 1), seed + 3)
            if lowx:
                o.ws = o.ws * (torch.rand(o.ws.shape, generator=_gen(seed + 8)) < dens * 0.75).float()
    if side == 'wgt':  # row scales 2^k, k over [-20, 10]; an all-zero row; a row whose low pieces go subnormal
        k = torch.linspace(-20, 10, Cout).round()
        unit = torch.ldexp(torch.ones(Cout, dtype=torch.float64), k.int())
        o.x[:, ZERO_CH] = 0
        if c['pro']:  # sparse after the prologue: x in {0, 1/2, 1} -> 2 x - 1 in {-1, 0, 1}
            o.x = (o.x + 1) / 2
        if kind == 'fp16x2':
            unit[SUB_ROW] *= 2.0 ** -17
        o.w = (o.w.double() * unit[:, None, None, None]).float()
        if kind == 'fp16x2':
            o.w[SUB_ROW, ZERO_CH] = 0
            o.w[SUB_ROW, ZERO_CH, kh // 2, kh // 2] = float(2.0 * unit[SUB_ROW] * 2.0 ** 17)
        o.w[ZERO_ROW] = 0
        if C2:
            o.ws = (o.ws.double() * unit[:, None, None, None]).float()
            o.ws[ZERO_ROW] = 0
    o.unit = unit
    u4 = unit[None, :, None, None]
    o.bias = (G((Cout, ), seed + 4).double() * unit).float()
    xin = o.x
    if c['pro']:  # GroupNorm-affine tables 2 x - 1, no SiLU: the low pieces pass through the prologue
        o.pro = (torch.full((B, C1), 2.0), torch.full((B, C1), -1.0))
        xin = o.x * 2 - 1
    ref = _conv_ref(form, xin.double(), o.w.double(), o.bias.double())
    if side == 'both':  # the three products Split<2>::mma issues: a0 b0 + a0 b1 + a1 b0
        xl, wl = split2(xin)[1].double(), split2(o.w)[1].double()
        ref = ref - _conv_ref(form, xl, wl)
    Ho, Wo = ref.shape[-2:]
    if C2:
        ref = ref + F.conv2d(o.x2.double(), o.ws.double())
        if side == 'both':
            ref = ref - F.conv2d(split2(o.x2)[1].double(), split2(o.ws)[1].double())
    if form in ('seg', 'epi'):
        o.rv = (G((B, Cout), seed + 5).double() * unit).float()
        ref = ref + o.rv.double()[:, :, None, None]
    if form in ('seg', 'epi', 'pw'):
        o.res = (G((B, Cout, Ho, Wo), seed + 6).double() * u4).float()
        ref = ref + o.res.double()
    o.ref64 = ref
    o.ref = ref.float()
    # ---- the budget: per accumulation, sum |terms| in the row's unit
    wn = o.w.double().abs() / unit[:, None, None, None]
    if side == 'wgt' and kind == 'fp16x2':
        wn[SUB_ROW, ZERO_CH] = 0  # meets x = 0: contributes no term
    epi = o.bias.double().abs()[None, :, None, None] / u4
    if o.rv is not None:
        epi = epi + o.rv.double().abs()[:, :, None, None] / u4
    if o.res is not None:
        epi = epi + o.res.double().abs() / u4
    if wino:
        Un = wino_U(o.w.double() / unit[:, None, None, None])
        if side == 'wgt':
            Un[:, SUB_ROW, ZERO_CH] = 0
        M = wino_m(wino_V(xin.double()).abs(), Un.abs())
        if C2:
            Vs, Us = wino_shortcut_m(o.x2.double(), o.ws.double() / unit[:, None, None, None])
            M = M + torch.stack([torch.einsum('bchw,oc->bohw', v.abs(), u.abs()) for v, u in zip(Vs, Us)])
        yb = torch.stack([M[0] + M[1] + M[2], M[1] + M[2] + M[3]], dim=-1).flatten(-2)  # |y0|, |y1| bounds
        o.accs = [M[n] for n in range(4)] + [yb + epi]
    else:
        acc = _conv_ref(form, xin.double().abs(), wn)
        if C2:
            acc = acc + F.conv2d(o.x2.double().abs(), o.ws.double().abs() / unit[:, None, None, None])
        o.accs = [acc + epi]
    o.budget = max(float(a.abs().max()) for a in o.accs) * 2.0 ** s
    return o


# ------------------------------------------------------------------------------------------------------- impulses
IMPULSE_TILES = [('bf16x3', 4), ('bf16x3', 6), ('fp16x2', 4), ('fp16x2', 6), ('fp16x2', 10), ('fp16x2', 11)]
IMPULSE_PIX = [(0, 0), (0, 5), (7, 15), (9, 6)]  # corner, edge, last row / column of a 128-pixel tile, interior


def impulse_label(kind, tile):
    return _label_patch3(tile, 'plain', 2 if kind == 'fp16x2' else 3) if tile < 10 else _label_k32(tile, 'plain')


@functools.lru_cache(maxsize=2)
def onehot_weights_case(kind, small):
    """Output channel 32 tap + c selects input channel c at that tap (taps that leave the map read the zero padding):
    the output is the shifted input bit for bit. fp16x2: P16 activations (small: every low piece an fp16 subnormal);
    bf16x3: random fp32 over 16 binades (any normal fp32 splits exactly into three bf16 pieces)."""
    B, C, H = 2, 32, 16
    w = torch.zeros((9 * C, C, 3, 3))
    for tap in range(9):
        w[tap * C + torch.arange(C), torch.arange(C), tap // 3, tap % 3] = 1.0
    if kind == 'fp16x2':
        x = p16((B, C, H, H), 7001, -8, -3) if small else p16((B, C, H, H), 7002, -2, 3)
    else:
        g = _gen(7003)
        x = torch.randn((B, C, H, H), generator=g) * torch.ldexp(torch.ones(1), torch.randint(-8, 8, (B, C, H, H),
                                                                                              generator=g))
    ref = F.conv2d(x.double(), w.double(), padding=1)
    return x, w, ref


@functools.lru_cache(maxsize=2)
def impulse_acts_case(kind):
    """One pixel of one channel per image set to 1: the output around it is the flipped kernel of that channel bit for
    bit. fp16x2: P16-style weight rows under row scales (p16_rows); bf16x3: three-piece G3 values times 2^k per row."""
    B, C, Cout, H = 4, 32, 64, 16
    x = torch.zeros((B, C, H, H))
    for b, (py, px) in enumerate(IMPULSE_PIX):
        x[b, (7 * b + 3) % C, py, px] = 1.0
    if kind == 'fp16x2':
        w = p16_rows(Cout, 9 * C, 7100).view(Cout, C, 3, 3)
    else:
        k = torch.linspace(-20, 10, Cout).round().int()
        w = g3((Cout, C, 3, 3), 7101, 3) * torch.ldexp(torch.ones(Cout), k)[:, None, None, None]
    ref = F.conv2d(x.double(), w.double(), padding=1)
    return x, w, ref
