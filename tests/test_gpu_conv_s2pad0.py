"""The 3x3 stride-2 conv over an input padded at the bottom and right only (dm_conv2d_nhwc_s2pad0: the KL
autoencoder's Downsample, F.pad(x, (0, 1, 0, 1)) then stride 2 without padding -- output pixel o reads input rows /
columns 2o .. 2o + 2) on its three loaders and on the K = 32 kernel's stride-2 row-segment tile:

* the fp32 im2col kernel (tiles 1..3; tile 0 where no patch tile divides the shape or no split weights are given),
* conv_patch3 MODE 4 (tile 6) and conv_k32 variant 9 (tile 18): whole output rows, Wout <= 64,
* conv_k32 variant 13 (tile 22, and tile 0 for this form): 64-pixel segments of one output row, Wout > 64.

As tests/test_gpu_conv_k32.py / tests/test_gpu_r4.py do for the symmetric form: integer operands (-2..3) compare bit
for bit with the fp64 torch reference, random operands keep the error vs fp64 within 2x the fp32 im2col kernel's on the
same inputs (the project's rule for split convs, here without the 1e-7-of-scale allowance the older tests add)."""
import pytest
import torch
import torch.nn.functional as F

import dmhip
from tests.test_gpu_ops import _ints, _nhwc, _pack

pytestmark = pytest.mark.gpu

SEG_NOTE = 'stride-2 row segments'  # conv2d_k32's launch-log line of variant 13


def _ref(x, w, b=None):
    return F.conv2d(F.pad(x, (0, 1, 0, 1)).double(), w.double(), None if b is None else b.double(), stride=2)


def _desc(cuda, x_nhwc, w_packed, Cout, bias=None, tile=0, split=False, y_pitch=None):
    """(desc, y, keep-alive tensors) of a 3x3 stride-2 conv; the output of an even map is half its size, as the
    bottom/right-padded form and the symmetric one agree there."""
    B, Hin, Win, Cin = x_nhwc.shape
    Hout, Wout = (Hin - 2) // 2 + 1, (Win - 2) // 2 + 1
    y_pitch = y_pitch or Cout
    y = torch.full((B, Hout, Wout, y_pitch), float('nan'), device=cuda)
    d = dmhip.ConvDesc()
    d.x, d.x_pitch, d.Cin, d.Hin, d.Win = x_nhwc.data_ptr(), Cin, Cin, Hin, Win
    d.taps, d.stride, d.upsample = 9, 2, 0
    d.w, d.K = w_packed.data_ptr(), w_packed.shape[1]
    d.y, d.y_pitch, d.Cout, d.B, d.Hout, d.Wout = y.data_ptr(), y_pitch, Cout, B, Hout, Wout
    d.bias = bias.data_ptr() if bias is not None else None
    d.tile = tile
    keep = [x_nhwc, w_packed, bias]
    if split:
        ws = dmhip.pack_conv_weight_split(w_packed, 1, Cin, 9, dmhip.SPLIT_FP16X2)
        d.w_split, d.w_split_kind = ws.data_ptr(), dmhip.SPLIT_FP16X2
        keep.append(ws)
    return d, y, keep


def _run(cuda, x, w, b=None, tile=0, split=False, y_pitch=None):
    d, y, keep = _desc(cuda, _nhwc(x).to(cuda), _pack(w, cuda), w.shape[0], None if b is None else b.to(cuda), tile,
                       split, y_pitch)
    dmhip.conv2d_nhwc_s2pad0(d, cuda)
    torch.cuda.synchronize(cuda)
    return y


# (B, Cin, Cout, Hin, Win), split weights given, tiles: the automatic pick and each forced tile that takes the shape
IM2COL = [((1, 32, 64, 12, 20), False, [0, 1, 2, 3]),   # Wout = 10: no patch tile divides it
          ((2, 64, 32, 8, 8), False, [0, 1, 2, 3])]
ROWS = [((2, 64, 64, 32, 32), True, [0, 6, 18, 3]),
        ((3, 32, 128, 16, 16), True, [0, 6, 18, 3]),
        ((1, 96, 64, 8, 128), True, [0, 18, 3])]        # Wout = 64: one whole-row tile per row (390 patch pixels)
SEGS = [((1, 32, 64, 4, 256), True, [0, 22, 3]),        # Wout = 128: two segments, two rows
        ((2, 64, 160, 8, 256), True, [0, 22, 3]),       # Cout not a multiple of 128
        ((1, 32, 32, 2, 512), True, [0, 22, 3])]        # four segments, a single output row
CASES = [(s, sp, t) for s, sp, ts in IM2COL + ROWS + SEGS for t in ts]


@pytest.mark.parametrize('shape,split,tile', CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_s2pad0_exact(cuda, shape, split, tile):
    B, Cin, Cout, H, W = shape
    x = _ints((B, Cin, H, W), -2, 3, seed=200)
    w = _ints((Cout, Cin, 3, 3), -2, 3, seed=201)
    b = _ints((Cout, ), seed=202)
    ref = _ref(x, w, b).float()
    dmhip.launch_log(True)
    y = _run(cuda, x, w, b, tile, split, y_pitch=Cout + 32)
    log = dmhip.launch_log_read()
    dmhip.launch_log(False)
    assert torch.equal(y[..., :Cout].cpu(), _nhwc(ref))
    assert torch.isnan(y[..., Cout:]).all()  # a pitched view: untouched beyond Cout
    # outputs wider than 64 pixels: tile 22 and, for this form, the automatic pick run the row-segment tile
    seg = W // 2 > 64 and tile in (0, 22)
    assert any(SEG_NOTE in ln for ln in log) == seg, log


@pytest.mark.parametrize('shape,tile', [((2, 64, 64, 32, 32), 6), ((2, 64, 64, 32, 32), 18), ((3, 32, 128, 16, 16), 18),
                                        ((1, 96, 64, 8, 128), 18), ((1, 32, 64, 4, 256), 22),
                                        ((2, 64, 160, 8, 256), 22), ((1, 32, 32, 2, 512), 22)])
def test_s2pad0_fp32_accuracy(cuda, shape, tile):
    """Random operands on the fp16x2 split paths: error vs fp64 within 2x the fp32 im2col kernel's on the same inputs
    (measured: the split paths' error is 0.5 .. 0.95 of the fp32 kernel's on every case)."""
    B, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(203)
    x = torch.randn((B, Cin, H, W), generator=g) * 3
    w = torch.randn((Cout, Cin, 3, 3), generator=g) * (1.0 / (9 * Cin) ** 0.5)
    ref = _nhwc(_ref(x, w))
    errs = []
    for split, t in ((False, 3), (True, tile)):
        y = _run(cuda, x, w, None, t, split)
        errs.append((y.cpu().double() - ref).abs().max().item())
    print(f's2pad0 accuracy {shape} tile {tile}: fp32 {errs[0]:.3e} split {errs[1]:.3e}')
    assert errs[1] <= 2.0 * errs[0], errs


EDGE = [((1, 32, 64, 12, 20), False, 0), ((2, 64, 64, 32, 32), True, 6), ((2, 64, 64, 32, 32), True, 18),
        ((1, 96, 64, 8, 128), True, 18), ((1, 32, 64, 4, 256), True, 22), ((1, 32, 32, 2, 512), True, 22)]


@pytest.mark.parametrize('first', [False, True], ids=['last', 'first'])
@pytest.mark.parametrize('shape,split,tile', EDGE, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_s2pad0_padding_side(cuda, shape, split, tile, first):
    """An input that is non-zero only in its last row and last column pins the bottom / right padding (a loader that
    kept the symmetric origin would read them one output pixel late, or not at all); the mirror case, non-zero only in
    the first row and column, pins that nothing is padded at the top / left."""
    B, Cin, Cout, H, W = shape
    full = _ints((B, Cin, H, W), -2, 3, seed=204)
    full[full == 0] = 1.0
    x = torch.zeros_like(full)
    r = 0 if first else -1
    x[:, :, r, :] = full[:, :, r, :]
    x[:, :, :, r] = full[:, :, :, r]
    w = _ints((Cout, Cin, 3, 3), -2, 3, seed=205)
    ref = _ref(x, w).float()
    assert ref.abs().max() > 0
    y = _run(cuda, x, w, None, tile, split)
    assert torch.equal(y.cpu(), _nhwc(ref))


@pytest.mark.parametrize('shape,G', [((1, 32, 64, 4, 256), 8), ((2, 64, 128, 8, 256), 32)])
def test_s2pad0_segment_tile_gn_stats(cuda, shape, G):
    """The row-segment tile's epilogue emits the consumer's GroupNorm statistics: per (image, 64-pixel chunk, group)
    the sum and sum of squares of the stored output, i.e. gn_partial of it (here restated in float64 torch), within
    the 1e-6 of the scale that tests/test_gpu_presplit.py::test_unet_emitted_gn_stats allows."""
    B, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(206)
    x = torch.randn((B, Cin, H, W), generator=g) * 3
    w = torch.randn((Cout, Cin, 3, 3), generator=g) * (1.0 / (9 * Cin) ** 0.5)
    b = torch.randn((Cout, ), generator=g)
    d, y, keep = _desc(cuda, _nhwc(x).to(cuda), _pack(w, cuda), Cout, b.to(cuda), 22, True)
    HW = (H // 2) * (W // 2)
    part = torch.full((B, HW // 64, G, 2), float('nan'), dtype=torch.float64, device=cuda)
    dmhip.conv2d_gn_stats(d, G, part, s2_pad0=True, device=cuda)
    torch.cuda.synchronize(cuda)
    ref = _nhwc(_ref(x, w, b))
    assert (y.cpu().double() - ref).abs().max().item() < 4e-6 * ref.abs().max().item()
    v = y.cpu().double().reshape(B, HW // 64, 64, G, Cout // G)
    want = torch.stack([v.sum(dim=(2, 4)), (v * v).sum(dim=(2, 4))], dim=-1)
    got = part.cpu()
    for k in range(2):
        assert (got[..., k] - want[..., k]).abs().max().item() <= 1e-6 * want[..., k].abs().max().item()


def test_s2pad0_rejects_other_convs(cuda):
    x = _nhwc(_ints((1, 32, 8, 8))).to(cuda)
    d, y, keep = _desc(cuda, x, _pack(_ints((32, 32, 3, 3)), cuda), 32)
    d.stride = 1
    with pytest.raises(ValueError, match='3x3 stride-2'):
        dmhip.conv2d_nhwc_s2pad0(d, cuda)


@pytest.mark.parametrize('shape', [(1, 32, 64, 4, 256), (2, 64, 160, 8, 256)])
def test_symmetric_form_on_the_forced_segment_tile(cuda, shape):
    """dm_conv2d_nhwc with tile 22: the symmetric (padding 1) stride-2 conv on the row-segment tile, whose column
    origin is then 2 x0 - 1 with x0 > 0 (never the automatic pick for this form): integer operands bit for bit."""
    from tests.test_gpu_ops import _run_conv
    B, Cin, Cout, H, W = shape
    x = _ints((B, Cin, H, W), -2, 3, seed=208)
    w = _ints((Cout, Cin, 3, 3), -2, 3, seed=209)
    b = _ints((Cout, ), seed=210)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1).float()
    dmhip.launch_log(True)
    y = _run_conv(cuda, _nhwc(x).to(cuda), _pack(w, cuda), Cout, H // 2, W // 2, 9, 2, 0, b.to(cuda), split='fp16x2',
                  tile=22)
    torch.cuda.synchronize(cuda)
    log = dmhip.launch_log_read()
    dmhip.launch_log(False)
    assert any(SEG_NOTE in ln for ln in log), log
    assert torch.equal(y.cpu(), _nhwc(ref))


def test_symmetric_wide_downsample_keeps_its_path(cuda):
    """Tripwire: the symmetric entry on a stride-2 conv with a 128-pixel-wide output still runs the fp32 im2col kernel
    under the automatic pick (the row-segment tile is for the bottom/right-padded form only): tile 0 returns bit for
    bit what the forced im2col tile the picker chooses for it (tile 3, 64 x 64) returns, and the segment tile is not
    launched."""
    from tests.test_gpu_ops import _run_conv
    B, Cin, Cout, H, W = 1, 64, 64, 8, 256
    g = torch.Generator().manual_seed(207)
    x = torch.randn((B, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) * 0.05
    xd, wp = _nhwc(x).to(cuda), _pack(w, cuda)
    dmhip.launch_log(True)
    y0 = _run_conv(cuda, xd, wp, Cout, H // 2, W // 2, 9, 2, 0, split='fp16x2', tile=0)
    torch.cuda.synchronize(cuda)
    log = dmhip.launch_log_read()
    dmhip.launch_log(False)
    ys = [_run_conv(cuda, xd, wp, Cout, H // 2, W // 2, 9, 2, 0, split='fp16x2', tile=t) for t in (1, 2, 3)]
    assert not any(SEG_NOTE in ln for ln in log), log
    # M = 512 rows, Cout = 64: conv_choose's im2col choice is the 64 x 64 tile (fewer than 512 blocks of the larger ones)
    assert torch.equal(y0.cpu(), ys[2].cpu())
    ref = _nhwc(F.conv2d(x.double(), w.double(), stride=2, padding=1))
    for yy in [y0] + ys:
        assert (yy.cpu().double() - ref).abs().max().item() < 1e-5 * ref.abs().max().item()
