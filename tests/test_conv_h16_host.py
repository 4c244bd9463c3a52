"""The conv-half references on the CPU (tests/conv_h16_ref.py): the cases are what they claim to be, and every bound of
tests/test_gpu_conv_h16.py holds for a host emulation of the kernel (.half() operands, the host row scale, fp32
accumulation), so a bound the arithmetic itself would break is caught here and not on the device."""
import pytest
import torch

from tests import conv_h16_ref as cr
from tests import token_ref as tr

EMU = cr.Emu()


def test_covered_rule():
    ok = [(64, 0, 64, 8, 8), (32, 128, 64, 8, 8), (96, 0, 96, 32, 32), (32, 0, 32, 256, 256), (64, 0, 32, 128, 128),
          (32, 0, 64, 64, 96), (32, 0, 32, 16, 8)]
    for c1, c2, co, h, w in ok:
        assert cr.covered(c1, c2, co, h, w), (c1, c2, co, h, w)
    bad = [dict(Cin1=48, Cin2=0, Cout=32, H=8, W=8), dict(Cin1=64, Cin2=16, Cout=32, H=8, W=8),
           dict(Cin1=64, Cin2=0, Cout=48, H=8, W=8), dict(Cin1=64, Cin2=0, Cout=64, H=4, W=4),
           dict(Cin1=64, Cin2=0, Cout=64, H=8, W=8, stride=2), dict(Cin1=64, Cin2=0, Cout=64, H=8, W=8, upsample=1),
           dict(Cin1=64, Cin2=0, Cout=64, H=8, W=8, upsample=2), dict(Cin1=64, Cin2=0, Cout=64, H=8, W=8, taps=1),
           dict(Cin1=32, Cin2=0, Cout=32, H=48, W=48), dict(Cin1=32, Cin2=0, Cout=32, H=8, W=512),
           dict(Cin1=32, Cin2=0, Cout=32, H=24, W=8)]
    for kw in bad:
        assert not cr.covered(**kw), kw
    assert [cr.form_of(h, h) for h in (8, 16, 32, 64, 128, 256)] == [1, 1, 1, 2, 2, 2]


@pytest.mark.parametrize('shape', cr.EXACT_SHAPES)
def test_exact_cases_are_exact(shape):
    """Integer operands: the emulation equals float64 bit for bit, per forced form and automatically; the other form
    is refused and writes nothing."""
    s = cr.exact_case(*shape)
    B, Cin, Cout, H = shape
    assert s['x'].abs().max() <= 8 and s['w'].abs().max() <= 8 and 64 * 9 * Cin < 2 ** 24
    want = cr.nhwc(cr.exact_ref(s))
    assert len({tuple(r.tolist()) for r in want.reshape(-1, Cout)[:64]}) > 32       # rows tell pixels apart
    f = cr.form_of(H, H)
    for tile in (0, f):
        r = EMU.conv(s, tile)
        assert r['rc'] == 0 and torch.equal(r['y'], want)
    r = EMU.conv(s, 3 - f)
    assert r['rc'] != 0 and torch.isnan(r['y']).all()


@pytest.mark.parametrize('shape', cr.SEG_SHAPES)
def test_segment_cases_are_exact(shape):
    s = cr.segments_case(*shape)
    r = EMU.conv(s)
    Cout = s['w'].shape[0]
    assert r['rc'] == 0 and torch.equal(r['y'][..., :Cout], cr.nhwc(cr.exact_ref(s)))
    assert torch.isnan(r['y'][..., Cout:]).all() and r['y'].shape[-1] == s['y_pitch']
    w1, ws = cr.w_rounded(s)
    assert torch.equal(w1, s['w']) and torch.equal(ws, s['ws'])       # integer weights survive the row scale


@pytest.mark.parametrize('kind', cr.IMAGE_KINDS)
def test_image_bound_dry(kind):
    s = cr.image_case(kind)
    r = EMU.image(s)
    used = cr.image_check(s, r['plane1'].double(), None if r['plane2'] is None else r['plane2'].double())
    assert 0.0 < used <= 1.0 and r['flag'] == 0
    # the bound is tight: an fp16 ulp more on one element breaks it
    p = r['plane1'].double().clone()
    i = p.abs().argmax()
    p.view(-1)[i] += 1.01 * cr.ulp16(p.view(-1)[i])
    with pytest.raises(AssertionError):
        cr.image_check(s, p, None if r['plane2'] is None else r['plane2'].double())


@pytest.mark.parametrize('shape', cr.HOST_SHAPES)
def test_conv_and_distance_bounds_dry(shape):
    """Checks (4) and (5) on the emulation: the fp32 accumulation error stays inside 2 e32 + 2^-21 max|ref|, the
    distance to fp16x2 inside its bound with room to spare, and the two results differ."""
    s = cr.rand_case(*shape)
    r = EMU.conv(s)
    Cout = s['w'].shape[0]
    used4, bound4, e32 = cr.conv_on_image_check(s, r['y'][..., :Cout], r['plane1'].double())
    used5 = cr.distance_check(s, r['y'][..., :Cout], EMU.fp16x2(s), bound4)
    print(f'{shape}: check (4) {used4:.3f} of its bound (e32 {e32:.3e}), check (5) {used5:.3f}')
    assert used5 < 0.5        # the rounding noise adds in quadrature; the bound adds it linearly
    # a product dropped from one output breaks check (4)
    y = r['y'][..., :Cout].clone()
    y[0, 0, 0, 0] += 4.0 * bound4
    with pytest.raises(AssertionError):
        cr.conv_on_image_check(s, y, r['plane1'].double())


@pytest.mark.parametrize('segment', [1, 2])
def test_flag_cases(segment):
    assert EMU.conv(cr.flag_case(segment, 65504.0))['flag'] == 0
    assert EMU.conv(cr.flag_case(segment, 1e5))['flag'] == 1


@pytest.mark.parametrize('kind', cr.REFUSALS)
def test_refusal_cases(kind):
    r = EMU.conv(cr.refusal_case(kind), cr.form_of(8, 8))
    assert r['rc'] != 0 and torch.isnan(r['y']).all()


def test_batch_invariance_of_the_emulation():
    """The case slicing of the GPU test's check (9): image i of the batch is the B = 1 case of its own data and table
    rows (the planes bit for bit; the host's fp32 conv may order its sums by batch size, so y to fp32 rounding)."""
    s = cr.rand_case(3, 64, 64, 8)
    full = EMU.conv(s)
    for i in range(3):
        one = dict(s, x=s['x'][i:i + 1], pro=tuple(t[i:i + 1] for t in s['pro']))
        r = EMU.conv(one)
        assert torch.equal(full['plane1'][i:i + 1], r['plane1'])
        assert (full['y'][i:i + 1] - r['y']).abs().max() <= 2.0 ** -20 * r['y'].abs().max()
        assert not torch.equal(full['y'][(i + 1) % 3:(i + 1) % 3 + 1], r['y'])


def test_model_level_rounding_hooks():
    """h16_conv2d rounds exactly the covered layers of a host forward: a tiny ResBlock-shaped graph."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    sd = {'b.blk2.3.weight': torch.randn((64, 32, 3, 3), generator=g, dtype=torch.float64) * 0.1,
          'b.shortcut.weight': torch.randn((64, 32, 1, 1), generator=g, dtype=torch.float64) * 0.1,
          'first.weight': torch.randn((32, 3, 3, 3), generator=g, dtype=torch.float64),
          'up.weight': torch.randn((32, 32, 3, 3), generator=g, dtype=torch.float64)}
    x = torch.randn((1, 3, 8, 8), generator=g, dtype=torch.float64)

    def fwd():
        h = F.conv2d(x, sd['first.weight'], padding=1)
        y = F.conv2d(h, sd['b.blk2.3.weight'], padding=1) + F.conv2d(h, sd['b.shortcut.weight'])
        u = F.conv2d(F.interpolate(h[..., :4, :4], scale_factor=2, mode='nearest'), sd['up.weight'], padding=1)
        return h, y, u

    h0, y0, u0 = fwd()
    with cr.h16_conv2d(sd) as ctx:
        h1, y1, u1 = fwd()
    assert ctx.calls == 1
    assert torch.equal(h0, h1) and torch.equal(u0, u1) and not torch.equal(y0, y1)
    spec = dict(x=h0.float(), x2=h0.float(), w=sd['b.blk2.3.weight'].float(), ws=sd['b.shortcut.weight'].float())
    w1, ws = cr.w_rounded(spec)
    want = F.conv2d(cr.round_a(h0), w1.double(), padding=1) + F.conv2d(cr.round_a(h0), ws.double())
    assert torch.equal(y1, want)
    assert F.conv2d is not None and F.conv2d.__name__ == 'conv2d' and torch.equal(fwd()[1], y0)   # restored
    assert (y1 - y0).abs().max() < 2.0 ** -9 * y0.abs().max() * 8
    assert tr.FP16_MAX == 65504.0


@pytest.mark.parametrize('name,n_covered', [('tiny', 16), ('tiny_updown', 19), ('adm_tiny', 19), ('pesser_a', 16)])
def test_host_forwards_against_the_goldens(golden, name, n_covered):
    """The float64 host forwards the model-level emulation runs on (oracle/unet.py, oracle/adm.py, and
    conv_h16_ref.pesser_forward, which has no oracle module) reproduce the reference fixtures; with the roundings of
    the covered layers they move by the size of an fp16 rounding, not more."""
    from utils.synthetic import init_synthetic_
    gfile, family = cr.MODELS[name]
    g, meta = golden(gfile)
    arch = dict(meta['archs'][name])
    if family == 'unet':
        from models.unet import UNet as M
    elif family == 'adagn':
        from models.unet_categorial_adagn import UNetCategorialAdaGN as M
    elif family == 'adm':
        from models.adm.unet import UNetModel as M
    else:
        from models.pesser.model import Model as M
    m = M(**arch).eval()
    init_synthetic_(m)
    x, t = torch.from_numpy(g[f'{name}_x']), torch.from_numpy(g[f'{name}_t'])
    y = torch.from_numpy(g[f'{name}_labels']) if f'{name}_labels' in g else None
    key = [k for k in (f'{name}_out_y', f'{name}_out', f'{name}_y') if k in g][0]
    want = torch.from_numpy(g[key]).double()
    o64, n0 = cr.host_forward(family, m.state_dict(), arch, x, t, y)
    o16, n = cr.host_forward(family, m.state_dict(), arch, x, t, y, h16=True)
    assert n0 == 0 and n == n_covered
    assert (o64 - want).abs().max().item() <= 1e-5
    emu16 = (o16 - want).abs().max().item()
    assert 1e-4 < emu16 < 2e-2, emu16
