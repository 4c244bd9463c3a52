"""The low pieces of the split convolutions, bit for bit against float64.

The integer-exact tests of conv_patch3.hip, conv_k32.hip and conv_wino.hip (test_gpu_conv_split / _k32 / _s2pad0 /
_r4 / _r5 / _r6) run operands whose low pieces are zero; the accuracy tests compare one aggregate per tensor, which a
low piece lost for one tap or one halo column passes. Here every low piece is non-zero and the result is still exact
(operand families and the budget: tests/split_operands_ref.py, checked on the host by test_split_operands_host.py),
so torch.equal against the float64 reference holds, and a misplaced low piece flips bits:

a. 'act': G16 (bf16x3: G3) activations against sparse integer weights -- the patch loaders' piece slots and swizzles,
   split_lo4 / dpp_sub4 / sub_f16 and the edge buffer of the Winograd loader, the a[1] operands;
b. 'wgt': sparse integer activations against G16 / G3 weights, each output row times its own 2^k (k over [-20, 10]),
   one all-zero row, one row 2^-17 below its maximum (low pieces subnormal in fp16) -- split_row_scale_kernel,
   split_conv_weights_kernel's slice order and piece planes, wino_pack_kernel, the b[1] operands;
c. 'both' (fp16x2 direct kernels): G16 against G16; the reference conv64(x, w) - conv64(x_lo, w_lo) is exactly the three
   products Split<2>::mma issues;
d. impulses (direct kernels): one-hot weights return the shifted P16 input, impulse activations the flipped P16 kernel.

Every test asserts from the launch log that the kernel it names ran (a forced tile that does not fit falls back
without an error) and that a pitched output stays NaN beyond Cout."""
import pytest
import torch

import dmhip
from tests import split_operands_ref as R
from tests.test_gpu_conv_s2pad0 import SEG_NOTE
from tests.test_gpu_conv_s2pad0 import _run as _run_s2pad0
from tests.test_gpu_ops import _nhwc, _pack, _pack_subpix, _run_conv

pytestmark = pytest.mark.gpu


def _logged(fn):
    dmhip.launch_log(True, convs=True)
    try:
        y = fn()
        torch.cuda.synchronize()
        return y, dmhip.launch_log_read()
    finally:
        dmhip.launch_log(False)


def _launch(cuda, c, x, w, bias, ws=None, x2=None, rv=None, res=None, pro=None, tile=None):
    """Run case `c` (tests/split_operands_ref.py) on NCHW fp32 operands: (y [B, Ho, Wo, y_pitch], launch log)."""
    form, Cout, C1, C2 = c['form'], c['Cout'], c['C1'], c['C2']
    tile = c['tile'] if tile is None else tile
    y_pitch = Cout + 32 if c['pitch'] else None
    if form == 's2pad0':
        return _logged(lambda: _run_s2pad0(cuda, x, w, bias, tile, True, y_pitch))
    B, _, H, W = x.shape
    if form == 'sub':
        wp = _pack_subpix(w, cuda)
    elif C2:
        wp = torch.zeros((Cout, 9 * C1 + C2), device=cuda)
        _pack(w, cuda, 9 * C1 + C2, 0, wp)
        _pack(ws, cuda, 9 * C1 + C2, 9 * C1, wp)
    else:
        wp = _pack(w, cuda)
    up = {'up1': 1, 'sub': 2}.get(form, 0)
    stride = 2 if form == 's2' else 1
    Ho, Wo = (2 * H, 2 * W) if up else (H // 2, W // 2) if stride == 2 else (H, W)
    wino = c['kernel'] == 'wino'
    xd, x_pitch = _nhwc(x).to(cuda), None
    if wino and c['pitch']:  # a pitched input view
        x_pitch = C1 + 32
        xp = torch.full((B, H, W, x_pitch), float('nan'), device=cuda)
        xp[..., :C1] = xd
        xd = xp[..., :C1]
    dev = lambda t: None if t is None else t.to(cuda)  # noqa: E731
    return _logged(lambda: _run_conv(
        cuda, xd, wp, Cout, Ho, Wo, 1 if form == 'pw' else 9, stride, up, dev(bias), rowvec=dev(rv),
        res=None if res is None else _nhwc(res).to(cuda), x2=None if x2 is None else _nhwc(x2).to(cuda), Cin2=C2,
        y_pitch=y_pitch, x_pitch=x_pitch, tile=tile, pro=None if pro is None else (dev(pro[0]), dev(pro[1])),
        pro_nosilu=1 if pro is not None else 0, split=c['kind'], ksplit=c['ksplit'], wino=wino))


def _check_label(c, log):
    assert log, 'empty launch log'
    if c['label'] is None:  # the automatic pick: a split kernel of this kind, whichever tile
        np_ = 2 if c['kind'] == 'fp16x2' else 3
        assert (log[-1].startswith('conv_patch3_kernel<') and log[-1].endswith(f',{np_}>')) or \
            (np_ == 2 and log[-1].startswith('conv_k32')), log
        return
    assert log[-1] == c['label'], log
    if c['kernel'] == 'wino' or c['tile'] == 15:  # these launchers log their instantiation themselves
        assert log[0] == c['label'] and len(log) == 2, log
    if c['tile'] == 22:
        assert any(SEG_NOTE in ln for ln in log), log


def _check(y, ref, Cout, pitched):
    want = _nhwc(ref)
    got = y[..., :Cout].cpu()
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        ch = bad.reshape(-1, Cout).any(0).nonzero().flatten().tolist()
        px = bad.any(-1).nonzero()[:8].tolist()
        raise AssertionError(f'{int(bad.sum())} of {bad.numel()} outputs differ; channels {ch[:16]} ({len(ch)}), '
                             f'first pixels (b, y, x) {px}, max |diff| {float((got - want).abs().nan_to_num().max()):.3e}')
    if pitched:
        assert y.shape[-1] > Cout and torch.isnan(y[..., Cout:]).all()


@pytest.mark.parametrize('idx', range(len(R.CASES)), ids=R.CASE_IDS)
def test_low_pieces_exact(cuda, idx):
    o = R.build(idx)
    c = o.case
    y, log = _launch(cuda, c, o.x, o.w, o.bias, o.ws, o.x2, o.rv, o.res, o.pro)
    _check_label(c, log)
    _check(y, o.ref, c['Cout'], c['pitch'])
    if c['tile'] == 17:  # the big-table instantiation: the same kernel, bit-equal to the 128 x 128 tiles
        y10, log10 = _launch(cuda, c, o.x, o.w, o.bias, tile=10)
        assert log10[-1] == R._label_k32(10, c['form']), log10
        assert torch.equal(y.cpu(), y10.cpu())


def _impulse_case(kind, tile):
    return dict(form='plain', Cout=0, C1=32, C2=0, tile=tile, pitch=False, kind=kind, ksplit=0,
                kernel='patch3' if tile < 10 else 'k32', label=R.impulse_label(kind, tile))


@pytest.mark.parametrize('small', [False, True], ids=['normal', 'subnormal-low'])
@pytest.mark.parametrize('kind,tile', R.IMPULSE_TILES)
def test_onehot_weights_return_the_shifted_input(cuda, kind, tile, small):
    """Output channel 32 tap + c = input channel c seen through that tap, 0 where the tap leaves the map. fp16x2
    'subnormal-low': |x| < 2^-3, every low piece an fp16 subnormal (the absolute floor of the activations' low piece
    that conv_patch3.hip's header relies on); bf16x3 runs random fp32 in both."""
    x, w, ref = R.onehot_weights_case(kind, small)
    c = dict(_impulse_case(kind, tile), Cout=w.shape[0])
    y, log = _launch(cuda, c, x, w, None)
    _check_label(c, log)
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    H = x.shape[-1]
    shifted = torch.cat([xp[:, :, t // 3:t // 3 + H, t % 3:t % 3 + H] for t in range(9)], dim=1)
    assert torch.equal(ref.float(), shifted)  # the reference is the shifted input itself
    _check(y, shifted, c['Cout'], False)


@pytest.mark.parametrize('kind,tile', R.IMPULSE_TILES)
def test_impulse_activations_return_the_flipped_kernel(cuda, kind, tile):
    """One pixel of one channel per image is 1 (a corner, an edge, the last pixel of a 128-pixel tile, an interior
    pixel): the 3 x 3 outputs around it are that channel's kernel flipped, bit for bit; every other output is 0."""
    x, w, ref = R.impulse_acts_case(kind)
    c = dict(_impulse_case(kind, tile), Cout=w.shape[0])
    y, log = _launch(cuda, c, x, w, None)
    _check_label(c, log)
    want = torch.zeros_like(ref, dtype=torch.float32)
    H = x.shape[-1]
    for b, (py, px) in enumerate(R.IMPULSE_PIX):
        ch = int(x[b, :, py, px].argmax())
        for dy in range(3):
            for dx in range(3):
                yy, xx = py + 1 - dy, px + 1 - dx
                if 0 <= yy < H and 0 <= xx < H:
                    want[b, :, yy, xx] = w[:, ch, dy, dx]
    assert torch.equal(ref.float(), want)
    _check(y, want, c['Cout'], False)
