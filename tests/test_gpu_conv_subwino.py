"""The sub-pixel Winograd upsample conv (conv_subwino.hip; models/modules.py:62-65, Upsample: nearest-2x + 3x3 conv)
through the C ABI's conv entry with ConvDesc.tile = 23.

* integer operands bit for bit against the float64 conv of the upsampled map (V, U, their fp16 pieces and the fp32 sums
  are exact): 4^2, 8^2 and 16^2 low-res maps, one / three images (a ragged group of four 4 x 4 images, several tiles),
  one / three 32-channel chunks, one / two 128-column halves, bias, pitched input and output;
* one non-zero pixel against one non-zero tap at every tap and at the corner, edge and inner pixels: no parity, row
  offset or padding mixed up;
* random operands against float64: max and rms errors no larger than the larger of the two existing paths' errors on
  the same operands (conv_k32's sub-pixel kernel with its tile forced, and the fp32 MFMA arithmetic);
* the consumer's GroupNorm partials from the epilogue against sums over the stored output;
* two neighbours inside the fp16 range whose difference is outside: the range flag, never a silent wrong value;
* the CIFAR-10 forward with the kernel on and off (DM_CONV_SUBWINO).
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import dmhip
from tests.test_gpu_ops import _ints, _nhwc, _pack_subpix, _run_conv
from tests.test_gpu_parity import _model

pytestmark = pytest.mark.gpu

SUBWINO = 23  # ConvDesc.tile: force the sub-pixel Winograd kernel
K32 = 10      # ConvDesc.tile: conv_k32's 128 x 128 tiles (the four 4-tap sub-pixel convs)


@contextlib.contextmanager
def _subwino_weights(w, cuda, gn=None):
    """_run_conv builds its descriptor itself: while this is active the conv entry it calls gets the sub-pixel
    Winograd image of the torch weight w in ConvDesc.w_wino (gn = (G, part): and goes through dm_debug_conv2d_gn)."""
    img = dmhip.pack_conv_weight_subwino(w.to(cuda))
    orig = dmhip.conv2d_nhwc

    def call(d, device=None):
        d.w_wino = img.data_ptr()
        if gn is not None:
            return dmhip.conv2d_gn_stats(d, gn[0], gn[1], device=device)
        return orig(d, device)
    dmhip.conv2d_nhwc = call
    try:
        yield
    finally:
        dmhip.conv2d_nhwc = orig
        torch.cuda.synchronize(cuda)  # img is freed on return


def _run_subwino(cuda, x_nhwc, w, Cout, H, bias=None, gn=None, **kw):
    with _subwino_weights(w, cuda, gn):
        return _run_conv(cuda, x_nhwc, _pack_subpix(w, cuda), Cout, 2 * H, 2 * H, 9, 1, 2, bias, tile=SUBWINO,
                         split='fp16x2', **kw)


def _ref(x, w, b=None):
    return F.conv2d(F.interpolate(x.double(), scale_factor=2, mode='nearest'), w.double(),
                    None if b is None else b.double(), padding=1)


@pytest.mark.parametrize('Cout', [128, 256])
@pytest.mark.parametrize('Cin', [32, 96])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('H', [4, 8, 16])
def test_subwino_exact(cuda, H, B, Cin, Cout):
    x = _ints((B, Cin, H, H), -2, 3, seed=300 + H)
    w = _ints((Cout, Cin, 3, 3), -2, 3, seed=301)
    b = _ints((Cout, ), seed=302)
    ref = _ref(x, w, b).float()
    dmhip.launch_log(True)
    y = _run_subwino(cuda, _nhwc(x).to(cuda), w, Cout, H, b.to(cuda))
    log = dmhip.launch_log_read()
    dmhip.launch_log(False)
    assert log == [f'conv_subwino_kernel<{H},0>'], log
    assert torch.equal(y.cpu(), _nhwc(ref))


@pytest.mark.parametrize('H,B', [(4, 5), (8, 2), (16, 2)])
def test_subwino_pitched_input_and_output(cuda, H, B):
    """The input a channel slice of a wider tensor, the output a slice of a wider (concat) buffer whose other columns
    stay untouched."""
    Cin, Cout = 64, 128
    x = _ints((B, Cin, H, H), -2, 3, seed=310)
    w = _ints((Cout, Cin, 3, 3), -2, 3, seed=311)
    b = _ints((Cout, ), seed=312)
    ref = _ref(x, w, b).float()
    xp = torch.full((B, H, H, 96), float('nan'), device=cuda)
    xp[..., :Cin] = _nhwc(x).to(cuda)
    y = _run_subwino(cuda, xp[..., :Cin], w, Cout, H, b.to(cuda), y_pitch=Cout + 32, x_pitch=96)
    assert torch.equal(y[..., :Cout].cpu(), _nhwc(ref))
    assert torch.isnan(y[..., Cout:]).all()


@pytest.mark.parametrize('tap', range(9))
@pytest.mark.parametrize('H', [4, 8, 16])
def test_subwino_single_pixel_single_tap(cuda, H, tap):
    """Image k has one non-zero pixel (the corners, the edge midpoints, an inner pixel; one channel), the weight one
    non-zero tap: each product must land on exactly the output pixels the upsampled conv puts it on."""
    Cin, Cout = 32, 128
    m = H // 2
    pix = [(0, 0), (0, H - 1), (H - 1, 0), (H - 1, H - 1), (0, m), (m, 0), (H - 1, m), (m, H - 1), (m, m - 1)]
    x = torch.zeros((len(pix), Cin, H, H))
    for k, (iy, ix) in enumerate(pix):
        x[k, (5 * k + 3) % Cin, iy, ix] = 2.0 + k
    w = torch.zeros((Cout, Cin, 3, 3))
    wt = _ints((Cout, Cin), -3, 4, seed=320 + tap)
    wt[wt == 0] = 1.0
    w[:, :, tap // 3, tap % 3] = wt
    ref = _ref(x, w).float()
    assert ref.abs().max() > 0
    y = _run_subwino(cuda, _nhwc(x).to(cuda), w, Cout, H)
    assert torch.equal(y.cpu(), _nhwc(ref))


@pytest.mark.parametrize('H', [8, 16])
def test_subwino_fp32_accuracy(cuda, report, H):
    """Random operands: the kernel's max and rms errors against float64 are no larger than the larger of the two
    existing paths' on the same operands -- conv_k32's sub-pixel kernel (tile forced) and the fp32 MFMA arithmetic."""
    B, Cin, Cout = 4, 96, 128
    g = torch.Generator().manual_seed(330 + H)
    x = torch.randn((B, Cin, H, H), generator=g) * 2 + 0.3
    w = torch.randn((Cout, Cin, 3, 3), generator=g) * (1.0 / (9 * Cin) ** 0.5)
    b = torch.randn(Cout, generator=g) * 0.01
    ref = _nhwc(_ref(x, w, b))
    xd, wp, bd = _nhwc(x).to(cuda), _pack_subpix(w, cuda), b.to(cuda)
    errs, rms = {}, {}
    for name in ('fp32', 'k32', 'subwino'):
        if name == 'subwino':
            y = _run_subwino(cuda, xd, w, Cout, H, bd)
        else:
            y = _run_conv(cuda, xd, wp, Cout, 2 * H, 2 * H, 9, 1, 2, bd, tile=K32 if name == 'k32' else 0,
                          split='fp16x2' if name == 'k32' else False)
        d = y.cpu().double() - ref
        errs[name] = d.abs().max().item()
        rms[name] = d.pow(2).mean().sqrt().item()
    scale = ref.abs().max().item()
    for k in errs:
        print(f'subwino accuracy H {H} {k}: max {errs[k] / scale:.3e} rms {rms[k] / scale:.3e} (of the scale)')
        report(f'subwino_accuracy_{H}_{k}_max_rel', errs[k] / scale)
        report(f'subwino_accuracy_{H}_{k}_rms_rel', rms[k] / scale)
    assert errs['subwino'] <= max(errs['fp32'], errs['k32']), errs
    assert rms['subwino'] <= max(rms['fp32'], rms['k32']), rms


@pytest.mark.parametrize('H,B,Cout,G', [(16, 2, 256, 32), (8, 3, 128, 8), (8, 2, 128, 4), (4, 5, 128, 32)])
def test_subwino_gn_partials(cuda, H, B, Cout, G):
    """The epilogue's GroupNorm partials of the stored output, [B][chunks of the output map][G] {sum, sum of squares}:
    summed over an image's chunks (what the consumer's finalize does with any disjoint cover) they equal the sums a
    gn_partial pass over the output gives, within the 1e-6 of the scale that
    tests/test_gpu_presplit.py::test_unet_emitted_gn_stats allows; and so do the finalized mean and variance."""
    Cin = 64
    g = torch.Generator().manual_seed(340 + H)
    x = torch.randn((B, Cin, H, H), generator=g) * 2 + 0.3
    w = torch.randn((Cout, Cin, 3, 3), generator=g) * (1.0 / (9 * Cin) ** 0.5)
    b = torch.randn(Cout, generator=g)
    nchunk = (2 * H) * (2 * H) // 64
    part = torch.full((B, nchunk, G, 2), float('nan'), dtype=torch.float64, device=cuda)
    y = _run_subwino(cuda, _nhwc(x).to(cuda), w, Cout, H, b.to(cuda), gn=(G, part))
    ref = _nhwc(_ref(x, w, b))
    assert (y.cpu().double() - ref).abs().max().item() < 4e-6 * ref.abs().max().item()
    v = y.cpu().double().reshape(B, 4 * H * H, G, Cout // G)
    want = torch.stack([v.sum(dim=(1, 3)), (v * v).sum(dim=(1, 3))], dim=-1)  # [B][G][2]
    got = part.cpu()
    assert torch.isfinite(got).all()
    got = got.sum(dim=1)
    for k in range(2):
        assert (got[..., k] - want[..., k]).abs().max().item() <= 1e-6 * want[..., k].abs().max().item()
    n = 4 * H * H * (Cout // G)
    mean_g, mean_w = got[..., 0] / n, want[..., 0] / n
    var_g, var_w = got[..., 1] / n - mean_g ** 2, want[..., 1] / n - mean_w ** 2
    assert (mean_g - mean_w).abs().max().item() <= 1e-6 * mean_w.abs().max().item()
    assert (var_g - var_w).abs().max().item() <= 1e-6 * var_w.abs().max().item()


def test_subwino_range_flag(cuda):
    """Two neighbours of +-40000, each inside the fp16 range while their difference (a V value) is outside: the range
    flag is raised or the result matches float64 -- never a silent wrong value. In range the flag stays clear."""
    B, Cin, Cout, H = 1, 32, 128, 8
    g = torch.Generator().manual_seed(350)
    x = torch.randn((B, Cin, H, H), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) * 0.05
    for big in (False, True):
        xb = x.clone()
        if big:
            xb[0, 3, 4, 3] = 40000.0
            xb[0, 3, 4, 4] = -40000.0
        flag = torch.zeros(1, dtype=torch.int32, device=cuda)
        y = _run_subwino(cuda, _nhwc(xb).to(cuda), w, Cout, H, range_flag=flag)
        ref = _nhwc(_ref(xb, w))
        ok = bool(torch.isfinite(y).all()) and (y.cpu().double() - ref).abs().max().item() < 4e-6 * ref.abs().max().item()
        if big:
            assert int(flag.item()) == 1 or ok
        else:
            assert int(flag.item()) == 0 and ok


def _forward_logged(meta, cuda, x, t):
    dmhip.launch_log(True)
    model, _ = _model(meta, 'cifar10', cuda)
    out = model(x, t)
    log = dmhip.launch_log_read()
    dmhip.launch_log(False)
    h = model.native_handle(cuda)
    dmhip.unet_profile_enable(h, 1)  # (the plan of the forward above: its op labels)
    return model, out, log, [op['label'] for op in dmhip.unet_profile_read(h)]


def test_subwino_cifar_forward_toggle(cuda, golden, monkeypatch, report):
    """The CIFAR-10 UNet (golden input, B = 2): with the kernel on, the three Upsample convs (4 -> 8, 8 -> 16 and
    16 -> 32) run conv_subwino_kernel -- in the launchers' own log and in the plan's op labels -- with no range
    fallback; DM_CONV_SUBWINO=0 gives the plan without it, the four-conv sub-pixel kernels in their place (conv_patch3
    MODE 2 at 4 -> 8, conv_k32 above); the two outputs agree within 1e-5."""
    g, meta = golden('forward')
    x = torch.from_numpy(g['cifar10_x']).to(cuda)
    t = torch.from_numpy(g['cifar10_t']).to(cuda)
    assert x.shape[0] == 2
    monkeypatch.setenv('DM_CONV_SUBWINO', '1')
    model_on, out_on, log_on, ops_on = _forward_logged(meta, cuda, x, t)
    assert dmhip.range_stats(model_on.native_handle(cuda))[0] == 0
    monkeypatch.setenv('DM_CONV_SUBWINO', '0')
    _, out_off, log_off, ops_off = _forward_logged(meta, cuda, x, t)
    on = [s for s in log_on if s.startswith('conv_subwino_kernel<')]
    assert sorted(on) == ['conv_subwino_kernel<16,0>', 'conv_subwino_kernel<4,0>', 'conv_subwino_kernel<8,0>'], log_on
    assert not any(s.startswith('conv_subwino') for s in log_off), log_off
    assert [s for s in log_on if not s.startswith('conv_subwino')] == log_off
    # op for op the same plan, but for the three Upsample convs -- and for the consumer of the 4 -> 8 one, whose
    # gn_partial pass over the concat goes (conv_patch3 MODE 2 emits no partials, conv_subwino does, so the concat's
    # statistics come from its slices' partials): no consumer gains a pass
    assert len(ops_on) == len(ops_off)
    diff = [(a, b) for a, b in zip(ops_on, ops_off) if a != b]
    convs = [(a, b) for a, b in diff if a.startswith('conv_subwino_kernel<')]
    assert len(convs) == 3 and all(b.startswith(('conv_k32_kernel<', 'conv_patch3_kernel<')) for a, b in convs), diff
    assert [d for d in diff if d not in convs] == [('gn_concat_stats', 'gn_partial')], diff
    assert ops_on.count('gn_partial') == ops_off.count('gn_partial') - 1
    err = (out_on - out_off).abs().max().item()
    report('subwino_cifar_forward_vs_off', err)
    assert err <= 1e-5, err
