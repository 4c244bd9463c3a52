"""Host-side references, bounds and an emulation of the conv-half option's 3x3 conv (csrc/conv_h16.hip, DESIGN.md
4.19), shared by tests/test_conv_h16_host.py (the checks dry-run on the emulation) and tests/test_gpu_conv_h16.py /
tests/test_gpu_unet_h16.py (the same checks on the device).

The arithmetic: a' = fp16_rne(prologue(x1)) and a2' = fp16_rne(x2) as planes [B][H][W][C] (unscaled); w' = piece 0 of
split_conv_weights' fp16x2 image, fp16_rne(w 2^er(row)) with er the power of two of the packed row [9 Cin1 + Cin2]
(token_ref.weight_row_exponents; token_h16_ref.w_rounded is w' 2^-er); acc = sum_k a' w' in fp32 over both K segments,
times 2^-er, then the fp32 epilogue (bias, per-image row vector, residual).

* covered(): the rule of the covered convs. exact_case(): integer operands in [-8, 8]: a', w' 2^er are fp16-exact and
  every partial sum is an integer below 2^24 (64 K <= 2^17), so the result is exact in fp32 in ANY order.
* image_check: a decoded plane within half an fp16 ulp of the float64 prologue plus 2 e32 + 2^-21 scale for the fp32
  prologue's own error (token_h16_ref.image_bound's terms, without an exponent).
* conv_on_image_check: the conv on a GIVEN image against float64 a' (*) w', bound 2 e32 + 2^-21 max|ref64| with e32 the
  error of an fp32 host conv on the same rounded operands (check (3) of tests/test_gpu_token_h16.py).
* distance_check: |C_h16 - C_fp16x2| <= (2^-10 + 2^-20) sum_k |a_k w_k| + 2^-25 sum_k |w_k| + the bound above; the
  second term covers unscaled activations below fp16's normal range (spacing 2^-24: half of it per element).
* Emu: the kernel restated with .half() operands and fp32 accumulation behind the interface of the GPU tests' device
  backend. h16_conv2d: the model-level emulation -- F.conv2d replaced on exactly the covered layers of a host forward.
"""
import functools

import torch
import torch.nn.functional as F

from tests import token_h16_ref as hr
from tests import token_ref as tr

F32, F64 = tr.F32, tr.F64
H16_REL = hr.H16_REL
REL = tr.REL
PAD = 8          # sentinel columns after Cout where a case asks for a pitched output
TILE_FORMS = (1, 2)   # dm_debug_conv_h16's forced forms: whole rows (8 / 16 / 32 wide), 2-D tiles (64 .. 256 wide)


# ------------------------------------------------------------------------------------------------------ the rule
def covered(Cin1, Cin2, Cout, H, W, taps=9, stride=1, upsample=0):
    """The covered convs of DESIGN.md 4.19 (conv_h16_ok's shape part; H: whole 128-pixel tiles of rows)."""
    if taps != 9 or stride != 1 or upsample != 0:
        return False
    if Cin1 <= 0 or Cin1 % 32 or Cin2 % 32 or Cout <= 0 or Cout % 32 or H * W < 64:
        return False
    if W in (8, 16, 32):
        rows = 128 // W
        return H % rows == 0 or rows % H == 0
    return 64 <= W <= 256 and W % 32 == 0 and H % 4 == 0


def form_of(H, W):
    return 1 if W in (8, 16, 32) else 2


# ------------------------------------------------------------------------------------------------------- cases
def _gen(*key):
    return torch.Generator().manual_seed(tr._seed('conv-h16', *key))


def _ints(shape, g, lo=-8, hi=9):
    return torch.randint(lo, hi, shape, generator=g).float()


EXACT_SHAPES = [(3, 64, 64, 8), (2, 32, 64, 16), (1, 96, 96, 32), (1, 160, 160, 16), (2, 64, 128, 32), (1, 32, 64, 64),
                (1, 64, 32, 128), (1, 32, 32, 256)]   # (B, Cin, Cout, H), square maps


@functools.lru_cache(maxsize=None)
def exact_case(B, Cin, Cout, H):
    g = _gen('exact', B, Cin, Cout, H)
    return dict(x=_ints((B, Cin, H, H), g), w=_ints((Cout, Cin, 3, 3), g), bias=_ints((Cout, ), g))


SEG_SHAPES = [(64, 32, 16), (96, 64, 32), (32, 128, 8), (32, 64, 64)]   # (C1, C2, H); B = 3 (2 at H = 64), Cout = 64


@functools.lru_cache(maxsize=None)
def segments_case(C1, C2, H):
    g = _gen('seg', C1, C2, H)
    B, Cout = (2 if H >= 64 else 3), 64
    return dict(x=_ints((B, C1, H, H), g), x2=_ints((B, C2, H, H), g), w=_ints((Cout, C1, 3, 3), g),
                ws=_ints((Cout, C2, 1, 1), g), bias=_ints((Cout, ), g), rowvec=_ints((B, Cout), g),
                res=_ints((B, Cout, H, H), g), y_pitch=Cout + 32)


IMAGE_KINDS = ['none', 'affine', 'affine_silu', 'pitched', 'per_image', 'segment2']


@functools.lru_cache(maxsize=None)
def image_case(kind):
    g = _gen('image', kind)
    B, C, H = 3, 64, 8
    s = dict(x=torch.randn((B, C, H, H), generator=g) * 2 + 0.3, w=torch.randn((32, C, 3, 3), generator=g) * 0.05)
    if kind in ('affine', 'affine_silu', 'per_image', 'pitched'):
        img = torch.arange(B, dtype=F32)[:, None] if kind == 'per_image' else torch.zeros((B, 1))
        s['pro'] = (0.5 + torch.rand((B, C), generator=g) + 0.25 * img, -2.0 + 4.0 * torch.rand((B, C), generator=g) + img)
        s['nosilu'] = 1 if kind == 'affine' else 0
    if kind == 'pitched':
        s['x_pitch'] = C + 32
    if kind == 'segment2':
        s['x2'] = torch.randn((B, 32, H, H), generator=g) * 3
        s['ws'] = torch.randn((32, 32, 1, 1), generator=g) * 0.1
    return s


RAND_SHAPES = [(4, 128, 128, 32), (2, 256, 256, 16), (5, 256, 256, 8), (1, 128, 128, 128), (2, 2048, 128, 8)]
HOST_SHAPES = [(2, 64, 64, 16), (3, 64, 64, 8), (1, 96, 160, 32), (1, 32, 64, 64)]   # the dry-run's smaller set


@functools.lru_cache(maxsize=None)
def rand_case(B, Cin, Cout, H, seed=90):
    """tests/test_gpu_conv_split._rand_case on the host: GroupNorm + SiLU'd inputs (the tables computed here in
    float64 and rounded to fp32), weights N(0, 1 / K)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, Cin, H, H), generator=g) * 2 + 0.3
    gamma, beta = torch.randn(Cin, generator=g), torch.randn(Cin, generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) * (1.0 / (9 * Cin) ** 0.5)
    b = torch.randn(Cout, generator=g) * 0.01
    xg = x.double().view(B, 32, -1)
    mu, var = xg.mean(dim=2), xg.var(dim=2, unbiased=False)
    rs = (1.0 / torch.sqrt(var + 1e-5)).repeat_interleave(Cin // 32, dim=1)
    sc = rs * gamma.double()[None, :]
    sh = -sc * mu.repeat_interleave(Cin // 32, dim=1) + beta.double()[None, :]
    return dict(x=x, w=w, bias=b, pro=(sc.float(), sh.float()), nosilu=0)


def flag_case(segment, peak):
    """65504 leaves the flag clear, 1e5 sets it: behind the prologue (scale 2, shift 0, no SiLU) or in segment 2."""
    g = _gen('flag', segment)
    B, C, H = 2, 32, 8
    s = dict(x=torch.randn((B, C, H, H), generator=g), w=torch.randn((32, C, 3, 3), generator=g) * 0.01)
    if segment == 1:
        s['pro'] = (torch.full((B, C), 2.0), torch.zeros((B, C)))
        s['nosilu'] = 1
        s['x'][1, 5, 3, 4] = peak / 2.0
    else:
        s['x2'] = torch.randn((B, C, H, H), generator=g)
        s['ws'] = torch.randn((32, C, 1, 1), generator=g) * 0.01
        s['x2'][1, 7, 2, 6] = -peak
    return s


REFUSALS = ['cin48', 'stride2', 'upsample1', 'upsample2', 'taps1', 'map4', 'misaligned']


def refusal_case(kind):
    g = _gen('refuse', kind)
    B, C, H = 2, (48 if kind == 'cin48' else 64), (4 if kind == 'map4' else 8)
    s = dict(x=_ints((B, C, H, H), g), w=_ints((32, C, 3, 3), g), bias=_ints((32, ), g))
    if kind == 'stride2':
        s['stride'] = 2
    if kind in ('upsample1', 'upsample2'):
        s['upsample'] = int(kind[-1])
    if kind == 'taps1':
        s['taps'] = 1
        s['w'] = _ints((32, C, 1, 1), g)
    if kind == 'misaligned':
        s['misalign'] = 1
    return s


# ------------------------------------------------------------------------------------------------- arithmetic
def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def prologue(s, dtype):
    """The conv's segment-1 operand before the rounding, NCHW in `dtype`: x, x sc + sh (separately rounded) or its SiLU."""
    x = s['x'].to(dtype)
    if s.get('pro') is None:
        return x
    sc, sh = (t.to(dtype)[:, :, None, None] for t in s['pro'])
    a = x * sc + sh
    return a if s.get('nosilu') else a * torch.sigmoid(a)


def packed_rows(s):
    """The packed weight rows [Cout][9 Cin1 + Cin2] in (tap, channel) order, the shortcut's after them."""
    w = s['w']
    rows = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    if s.get('ws') is not None:
        rows = torch.cat([rows, s['ws'].reshape(w.shape[0], -1)], dim=1)
    return rows


def w_rounded(s):
    """-> (w' 2^-er [Cout, Cin1, 3, 3], ws' 2^-er [Cout, Cin2, 1, 1] or None) as fp32 (exact): the weights the kernel
    multiplies by; one row exponent over both segments (token_h16_ref.w_rounded on the packed rows)."""
    w = s['w']
    r = hr.w_rounded(packed_rows(s))
    n1 = w.shape[1] * w.shape[2] * w.shape[3]
    w1 = r[:, :n1].reshape(w.shape[0], w.shape[2], w.shape[3], w.shape[1]).permute(0, 3, 1, 2).contiguous()
    ws = r[:, n1:].reshape(w.shape[0], -1, 1, 1) if s.get('ws') is not None else None
    return w1, ws


def images(s):
    """-> (a' fp16 NCHW, a2' fp16 NCHW or None, flag): the fp32 prologue, one rounding."""
    a = prologue(s, F32)
    flag = int((a.abs() > tr.FP16_MAX).any())
    a2 = None
    if s.get('x2') is not None:
        a2 = s['x2'].to(torch.float16)
        flag |= int((s['x2'].abs() > tr.FP16_MAX).any())
    return a.to(torch.float16), a2, flag


def epilogue(acc, s, dtype):
    y = acc
    if s.get('bias') is not None:
        y = y + s['bias'].to(dtype)[None, :, None, None]
    if s.get('rowvec') is not None:
        y = y + s['rowvec'].to(dtype)[:, :, None, None]
    if s.get('res') is not None:
        y = y + s['res'].to(dtype)
    return y


def conv_on(s, a1, a2, w1, ws, dtype):
    """epilogue(a1 (*) w1 + a2 . ws) in `dtype`, NCHW."""
    acc = F.conv2d(a1.to(dtype), w1.to(dtype), padding=1)
    if a2 is not None:
        acc = acc + F.conv2d(a2.to(dtype), ws.to(dtype))
    return epilogue(acc, s, dtype)


def exact_ref(s):
    """float64 conv of the unrounded operands (the integer cases: exact), NCHW fp32."""
    return conv_on(s, s['x'], s.get('x2'), s['w'], s.get('ws'), F64).float()


def ulp16(x):
    return hr.ulp16(x)


# ------------------------------------------------------------------------------------------------------ checks
def image_check(s, plane1, plane2=None):
    """Check (3). plane1 / plane2: the decoded planes NHWC (any float dtype). -> worst err / bound."""
    y = prologue(s, F64)
    e32 = (prologue(s, F32).double() - y).abs().max().item()
    scale = y.abs().max().item()
    pro = 2.0 * e32 + REL * scale
    bound = 0.5 * ulp16(y.abs() + pro) + pro
    worst = float(((nchw(plane1.double()) - y).abs() / bound).max())
    assert worst <= 1.0, f'segment-1 plane: err / bound {worst:.3g}'
    if s.get('x2') is not None:
        y2 = s['x2'].double()
        r2 = float(((nchw(plane2.double()) - y2).abs() / (0.5 * ulp16(y2.abs()))).max())   # no prologue: the rounding alone
        assert r2 <= 1.0, f'segment-2 plane: err / bound {r2:.3g}'
        worst = max(worst, r2)
    return worst


def conv_on_image_bound(s, plane1, plane2=None):
    """-> (ref64 NCHW, bound float, e32): the conv on the GIVEN image against the host's w'."""
    w1, ws = w_rounded(s)
    a1 = nchw(plane1.double())
    a2 = nchw(plane2.double()) if plane2 is not None else None
    ref = conv_on(s, a1, a2, w1, ws, F64)
    e32 = (conv_on(s, a1, a2, w1, ws, F32).double() - ref).abs().max().item()
    return ref, 2.0 * e32 + REL * ref.abs().max().item(), e32


def conv_on_image_check(s, y, plane1, plane2=None):
    """Check (4). y: the result NHWC [.., :Cout]. -> (err / bound, bound, e32)."""
    ref, bound, e32 = conv_on_image_bound(s, plane1, plane2)
    err = (nchw(y.double()) - ref).abs().max().item()
    assert err <= bound, f'conv on its own image: err {err:.3e} bound {bound:.3e} (e32 {e32:.3e})'
    return err / bound, bound, e32


def distance_check(s, y16, yx2, bound4):
    """Check (5): the distance between the conv-half and the fp16x2 results (NHWC), which must differ.
    -> the largest fraction of the bound used."""
    a = prologue(s, F64).abs()
    w = s['w'].double().abs()
    sab = F.conv2d(a, w, padding=1)
    sw = F.conv2d(torch.ones_like(a), w, padding=1)
    if s.get('x2') is not None:
        ws = s['ws'].double().abs()
        sab = sab + F.conv2d(s['x2'].double().abs(), ws)
        sw = sw + F.conv2d(torch.ones_like(s['x2'].double()), ws)
    bound = H16_REL * sab + 2.0 ** -25 * sw + bound4
    d = (nchw(y16.double()) - nchw(yx2.double())).abs()
    used = float((d / bound).max())
    assert used <= 1.0, f'distance to fp16x2: {used:.3g} of the bound'
    assert not torch.equal(y16, yx2), 'the conv-half result equals the fp16x2 one'
    return used


# ------------------------------------------------------------------------------------------------- the backend
class Emu:
    """The kernel on the host: .half() operands, the host row scale, fp32 accumulation (oneDNN's order). Answers what
    the GPU tests' device backend answers: conv(s, tile) -> dict(rc, y NHWC [B, H, W, pitch] (NaN beyond Cout and
    where refused), plane1, plane2 (fp16 NHWC), flag); image(s) -> the planes alone; fp16x2(s) -> NHWC."""
    name = 'h16-conv-emulation'

    def image(self, s):
        a1, a2, flag = images(s)
        return dict(rc=0, plane1=nhwc(a1), plane2=None if a2 is None else nhwc(a2), flag=flag)

    def conv(self, s, tile=0):
        w = s['w']
        B, C1, H, W = s['x'].shape
        Cout = w.shape[0]
        taps, stride, up = s.get('taps', 9), s.get('stride', 1), s.get('upsample', 0)
        Ho, Wo = (2 * H, 2 * W) if up else ((H - 1) // stride + 1, (W - 1) // stride + 1)
        pitch = s.get('y_pitch', Cout)
        out = dict(rc=0, y=torch.full((B, Ho, Wo, pitch), float('nan')), plane1=None, plane2=None, flag=0)
        C2 = s['x2'].shape[1] if s.get('x2') is not None else 0
        if (not covered(C1, C2, Cout, H, W, taps, stride, up) or s.get('misalign')
                or (tile != 0 and tile != form_of(H, W))):
            out['rc'] = -4
            return out
        a1, a2, flag = images(s)
        w1, ws = w_rounded(s)
        out['y'][..., :Cout] = nhwc(conv_on(s, a1.float(), None if a2 is None else a2.float(), w1, ws, F32))
        out.update(plane1=nhwc(a1), plane2=None if a2 is None else nhwc(a2), flag=flag)
        return out

    def fp16x2(self, s):
        """fp16x2 is fp32-accurate: the float64 conv of the fp32 prologue, rounded once."""
        return nhwc(conv_on(s, prologue(s, F32), s.get('x2'), s['w'], s.get('ws'), F64).float())


# ------------------------------------------------------------------------------------ model-level emulation
SHORTCUT_OF = {'.blk2.3.weight': '.shortcut.weight',              # models/unet.py
               '.blk2.2.weight': '.shortcut.weight',              # models/unet_categorial_adagn.py
               '.out_layers.3.weight': '.skip_connection.weight',  # models/adm/unet.py
               '.conv2.weight': '.nin_shortcut.weight'}            # models/pesser/model.py


def round_a(x):
    """fp16_rne of the fp32 rounding of x, in x's dtype (the engine's prologue is fp32; no scale)."""
    return x.to(F32).to(torch.float16).to(x.dtype)


class h16_conv2d:
    """Context manager that replaces torch.nn.functional.conv2d and F.interpolate while a HOST forward runs over the
    state_dict `sd`: on exactly the covered layers (covered() on the call's own shapes; a conv whose input is a
    nearest-upsampled tensor is the engine's upsample conv: not covered) the input and the weight are rounded as the
    engine rounds them and convolved in the forward's dtype; the 1x1 shortcut of a covered conv2 (SHORTCUT_OF) is
    rounded too, under the row scale it shares with conv2 in the packed row. Everything else is untouched."""

    def __init__(self, sd):
        self.sd = sd
        self.names = {id(v): k for k, v in sd.items()}
        self.rounded = {}
        self.calls = 0
        self.upsampled = []

    def _pair(self, name):
        """The (3x3 weight, shortcut weight or None) names of the packed row `name` belongs to, or None."""
        for c2, sc in SHORTCUT_OF.items():
            if name.endswith(c2):
                s = name[:-len(c2)] + sc
                return name, (s if s in self.sd else None)
            if name.endswith(sc):
                c = name[:-len(sc)] + c2
                if c in self.sd:
                    return c, name
        return name, None

    def _weights(self, name):
        if name not in self.rounded:
            c, s = self._pair(name)
            spec = dict(w=self.sd[c].to(F32), ws=None if s is None else self.sd[s].to(F32).reshape(self.sd[s].shape[0], -1, 1, 1))
            w1, ws = w_rounded(spec)
            self.rounded[c] = w1.to(self.sd[c].dtype)
            if s is not None:
                self.rounded[s] = ws.to(self.sd[s].dtype).reshape(self.sd[s].shape)
        return self.rounded[name]

    def __enter__(self):
        self._conv, self._interp = F.conv2d, F.interpolate

        def interpolate(x, *a, **k):
            y = self._interp(x, *a, **k)
            self.upsampled.append(y)
            return y

        def conv2d(x, w, b=None, stride=1, padding=0, *a, **k):
            name = self.names.get(id(w))
            st = stride if isinstance(stride, int) else stride[0]
            Cout, Cin, kh, kw = w.shape
            if name is None or st != 1 or (kh == 3 and any(x is u for u in self.upsampled)):
                return self._conv(x, w, b, stride, padding, *a, **k)
            H, W = x.shape[-2:]
            c, s = self._pair(name)
            if kh == 3 and name == c:
                C2 = self.sd[s].shape[1] if s is not None else 0
                if not covered(Cin, C2, Cout, H, W):
                    return self._conv(x, w, b, stride, padding, *a, **k)
            elif kh == 1 and name == s:
                if not covered(self.sd[c].shape[1], Cin, Cout, H, W):
                    return self._conv(x, w, b, stride, padding, *a, **k)
            else:
                return self._conv(x, w, b, stride, padding, *a, **k)
            self.calls += kh == 3
            return self._conv(round_a(x), self._weights(name), b, stride, padding, *a, **k)

        F.conv2d, F.interpolate = conv2d, interpolate
        return self

    def __exit__(self, *exc):
        F.conv2d, F.interpolate = self._conv, self._interp
        return False


class cast_inputs:
    """F.linear and F.group_norm with their input cast to the weight's dtype, torch.einsum with its operands cast to
    the widest of them, while a host forward runs in float64: the oracles build the sinusoidal timestep embedding in
    float32 and hand it to the first time-MLP layer, and oracle/adm.py's GroupNorm32 and attention softmax cast their
    input to float32 (the softmax then stays a float32 one: 1e-7 against the 1e-3 this emulation measures)."""

    def __enter__(self):
        self._lin, self._gn, self._ein = F.linear, F.group_norm, torch.einsum
        F.linear = lambda x, w, b=None: self._lin(x.to(w.dtype), w, b)
        F.group_norm = lambda x, G, w=None, b=None, eps=1e-5: self._gn(x if w is None else x.to(w.dtype), G, w, b, eps)

        def einsum(eq, *ops):
            dt = F64 if any(o.dtype == F64 for o in ops) else ops[0].dtype
            return self._ein(eq, *[o.to(dt) for o in ops])

        torch.einsum = einsum
        return self

    def __exit__(self, *exc):
        F.linear, F.group_norm, torch.einsum = self._lin, self._gn, self._ein
        return False


def pesser_forward(sd, x, t, ch, ch_mult, num_res_blocks, attn_resolutions, resolution, **_unused):
    """Host forward of the pesser DDPM UNet over a state_dict (models/pesser/model.py's parameter names; the topology
    of the executor's variant 3): GroupNorm(32, eps 1e-6), swish, [sin, cos] timestep embedding, single-head attention,
    stride-2 downsample over the bottom/right-padded map, nearest 2x + 3x3 upsample. Checked against the reference
    fixture tests/golden/pesser.npz in tests/test_conv_h16_host.py."""
    import math

    def gn(p, h):
        return F.group_norm(h, 32, sd[p + '.weight'], sd[p + '.bias'], 1e-6)

    def conv(p, h, stride=1, padding=None):
        w = sd[p + '.weight']
        return F.conv2d(h, w, sd[p + '.bias'], stride=stride, padding=w.shape[-1] // 2 if padding is None else padding)

    def lin(p, h):
        return F.linear(h, sd[p + '.weight'], sd[p + '.bias'])

    def block(p, h, temb):
        r = conv(p + '.conv1', F.silu(gn(p + '.norm1', h)))
        r = r + lin(p + '.temb_proj', F.silu(temb))[:, :, None, None]
        r = conv(p + '.conv2', F.silu(gn(p + '.norm2', r)))
        if (p + '.nin_shortcut.weight') in sd:
            h = conv(p + '.nin_shortcut', h)
        return h + r

    def attn(p, h):
        B, C, H, W = h.shape
        n = gn(p + '.norm', h)
        q, k, v = (conv(p + '.' + s, n).reshape(B, C, H * W) for s in 'qkv')
        a = (torch.bmm(q.permute(0, 2, 1), k) * (int(C) ** -0.5)).softmax(dim=2)
        return h + conv(p + '.proj_out', torch.bmm(v, a.permute(0, 2, 1)).reshape(B, C, H, W))

    half = ch // 2
    f = torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000) / (half - 1)))
    e = t.float()[:, None] * f[None, :]
    temb = lin('temb.dense.1', F.silu(lin('temb.dense.0', torch.cat([e.sin(), e.cos()], dim=1))))
    n_levels = len(ch_mult)
    use_attn = [(resolution >> lvl) in {int(r) for r in attn_resolutions} for lvl in range(n_levels)]
    hs = [conv('conv_in', x)]
    for lvl in range(n_levels):
        for i in range(num_res_blocks):
            h = block(f'down.{lvl}.block.{i}', hs[-1], temb)
            if use_attn[lvl]:
                h = attn(f'down.{lvl}.attn.{i}', h)
            hs.append(h)
        if lvl != n_levels - 1:
            hs.append(conv(f'down.{lvl}.downsample.conv', F.pad(hs[-1], (0, 1, 0, 1)), stride=2, padding=0))
    h = block('mid.block_2', attn('mid.attn_1', block('mid.block_1', hs[-1], temb)), temb)
    for lvl in reversed(range(n_levels)):
        for i in range(num_res_blocks + 1):
            h = block(f'up.{lvl}.block.{i}', torch.cat([h, hs.pop()], dim=1), temb)
            if use_attn[lvl]:
                h = attn(f'up.{lvl}.attn.{i}', h)
        if lvl != 0:
            h = conv(f'up.{lvl}.upsample.conv', F.interpolate(h, scale_factor=2.0, mode='nearest'))
    return conv('conv_out', F.silu(gn('norm_out', h)))


MODELS = {'tiny': ('forward', 'unet'), 'tiny_updown': ('adagn', 'adagn'), 'adm_tiny': ('adm', 'adm'),
          'pesser_a': ('pesser', 'pesser')}   # fixture name -> (golden file, family)


def host_forward(family, sd, arch, x, t, y=None, dtype=F64, h16=False):
    """The host forward of a conv denoiser in `dtype` over state_dict `sd` (oracle/unet.py, oracle/adm.py or
    pesser_forward); h16: under h16_conv2d. -> (output float64, the number of covered 3x3 convs that ran)."""
    from oracle import adm as oa
    from oracle import unet as ou
    sdd = {k: (v.detach().cpu().to(dtype) if v.is_floating_point() else v.detach().cpu()) for k, v in sd.items()}
    x = x.detach().cpu().to(dtype)
    t = t.detach().cpu()
    y = None if y is None else y.detach().cpu()

    def run():
        with torch.no_grad(), cast_inputs():
            if family == 'unet':
                keep = ('dim', 'dim_mults', 'use_attn', 'num_res_blocks', 'n_heads')
                return ou.unet_forward(sdd, x, t, **{k: v for k, v in arch.items() if k in keep})
            if family == 'adagn':
                keep = ('dim', 'dim_mults', 'use_attn', 'num_res_blocks', 'attn_head_dims', 'resblock_updown')
                return ou.unet_categorial_forward(sdd, x, t, y, **{k: v for k, v in arch.items() if k in keep})
            if family == 'adm':
                return oa.unet_model_forward(sdd, x, t, y, **{k: v for k, v in arch.items() if k not in ('image_size', 'in_channels', 'out_channels', 'dropout', 'dims', 'use_checkpoint', 'use_fp16')})
            return pesser_forward(sdd, x, t, **arch)
    if not h16:
        return run().double(), 0
    with h16_conv2d(sdd) as ctx:
        out = run()
    return out.double(), ctx.calls
