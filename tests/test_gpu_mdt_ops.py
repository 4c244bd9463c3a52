"""Operator-level tests of the biased flash attention (csrc/attention.hip attn_flash_kernel<Dh, NW, BW > 0>), MDT's
softmax(q k^T d^-1/2 + bias[h]) v with the relative-position bias formed arithmetically from a per-head table in LDS.

dm_debug_attention_bias launches attn_flash() on the test's own planes and table (pre-multiplied by log2(e), as the
engine stores it). The cases, their float64 references and the bound 2 e32 + 2^-21 max|ref| come from
tests/mdt_attention_ref.py (validated on the CPU by tests/test_mdt_host.py).
"""
import ctypes

import pytest
import torch

from tests import attention_ref as ar
from tests import mdt_attention_ref as mr

pytestmark = pytest.mark.gpu

PAD = 8            # untouched columns after heads * Dh in every `out` row
SENTINEL = 0x7e2a  # an fp16 NaN pattern no kernel writes


def _id(shape):
    return 'x'.join(map(str, shape))


def _attention(dev, shape, pq, pk, pv, ktable, W, form='out', o_ld=0):
    """dm_debug_attention_bias: ktable [heads, stride] float32 (None: the unbiased kernel). form 'out': fp32 rows of
    pitch heads Dh + PAD prefilled with NaN; 'o_split': the pre-split image of pitch o_ld prefilled with the
    sentinel. Returns (output on the CPU, range flag)."""
    from dmhip import _lib
    f = _lib.load().dm_debug_attention_bias
    vp, ci = ctypes.c_void_p, ctypes.c_int
    f.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, ci, vp, ci, ci, vp, vp, ci, ci, vp]
    B, H, L, Dh = shape
    C = H * Dh
    keep = [t.to(dev) for t in (pq, pk, pv)]
    tab = None if ktable is None else ktable.contiguous().to(dev)
    flag = torch.zeros((1, ), dtype=torch.int32, device=dev)
    out = img = None
    if form == 'out':
        out = torch.full((B, L, C + PAD), float('nan'), device=dev)
    else:
        img = torch.full((B * L * 2 * o_ld, ), SENTINEL, dtype=torch.int16, device=dev)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _lib.check(f(p(keep[0]), p(keep[1]), p(keep[2]), B, H, L, Dh, ar.EA, ar.EB, ar.EP, ar.EV, p(out), C + PAD, p(img),
                 6, o_ld, flag.data_ptr(), p(tab), W, 0 if tab is None else tab.shape[1],
                 torch.cuda.current_stream().cuda_stream), 'dm_debug_attention_bias')
    res = out.cpu() if form == 'out' else img.cpu()
    return res, int(flag.item())


def _checked_out(o, shape):
    """The pad columns are still NaN, everything else finite -> [B, heads, L, Dh] float64."""
    B, H, L, Dh = shape
    assert torch.isnan(o[..., H * Dh:]).all(), 'the kernel wrote beyond heads * Dh'
    assert torch.isfinite(o[..., :H * Dh]).all()
    return ar.out_rows(o, H, Dh).double()


@pytest.mark.parametrize('dist', mr.DISTS)
@pytest.mark.parametrize('shape', mr.SHAPES, ids=_id)
def test_flash_bias_vs_float64(cuda, report, shape, dist):
    """Every shape x distribution against float64 on the decoded operands: error <= 2 e32 + 2^-21 max|ref|. 'up40' /
    'down40' move the running maximum between key blocks in both orders; 'cross' / 'cross_rev' put the raw scores'
    maximum and the biased maximum in different key blocks (a maximum taken before the bias fails them)."""
    c = mr.case(shape, dist)
    o, flag = _attention(cuda, shape, c['pq'], c['pk'], c['pv'], mr.kernel_table(c['table']), c['W'])
    assert flag == 0
    got = _checked_out(o, shape)
    err = (got - c['ref']).abs().max().item()
    ratio = err / c['e32']
    key = f'attn_flash_bias_{_id(shape)}_{dist}'
    print(f'{key}: err {err:.3e} e32 {c["e32"]:.3e} ratio {ratio:.3f} bound {c["bound"]:.3e}')
    report(f'{key}_err_over_e32', ratio)
    assert err <= c['bound'], (key, err, c['e32'], c['scale'], ratio)


@pytest.mark.parametrize('shape', mr.SHAPES, ids=_id)
def test_flash_bias_select(cuda, shape):
    """q = 0: the bias alone picks the key (winner ahead by >= 128 nats, a different permutation per head), integer v
    rows: the output is v[pi(i)] to 2^-20 max|v|. A swapped i / j, a wrong head's table or a wrong W fails."""
    c = mr.case(shape, 'select')
    stride = (c['table'].shape[1] + 63) // 64 * 64    # a padded per-head stride, as the engine's
    o, _ = _attention(cuda, shape, c['pq'], c['pk'], c['pv'], mr.kernel_table(c['table'], stride), c['W'])
    got = _checked_out(o, shape)
    want = mr.selected_rows(c['v'], c['pi']).double()
    err = (got - want).abs().max().item()
    print(f'attn_flash_bias_{_id(shape)}_select: |out - v[pi]| {err:.3e}')
    assert err <= 2.0 ** -20 * c['v'].abs().max().item(), err


def test_flash_bias_head_permutation(cuda):
    """Heads and images are independent: with the same q, k, v in every (image, head), permuting the heads' tables
    permutes the outputs bit for bit, and both images agree."""
    shape = (2, 3, 256, 72)
    c = mr.case((1, 2, 256, 72), 'rand')
    q, k, v = (t[:, :1].expand(2, 3, -1, -1).contiguous() for t in (c['q'], c['k'], c['v']))
    pq, pk, pv, _ = ar.pack_planes(q, k, v)
    g = torch.Generator().manual_seed(9)
    table = torch.randn((3, (2 * 16 - 1) ** 2), generator=g)
    perm = [2, 0, 1]
    a, _ = _attention(cuda, shape, pq, pk, pv, mr.kernel_table(table), 16)
    b, _ = _attention(cuda, shape, pq, pk, pv, mr.kernel_table(table[perm]), 16)
    x, y = _checked_out(a, shape), _checked_out(b, shape)
    assert torch.equal(x[0], x[1]) and torch.equal(y[0], y[1])
    for h in range(3):
        assert torch.equal(y[:, h], x[:, perm[h]]), h
    assert not torch.equal(x[:, 0], x[:, 1])


def test_flash_bias_o_split(cuda):
    """The pre-split A image form (the engine's path into the proj GEMM) decodes to the `out` form of the same inputs
    within the fp16x2 split's 2^-21 |out| + 2^-30; columns in [heads Dh, o_ld) keep the sentinel; no range flag."""
    shape, o_ld = (1, 2, 256, 72), 160
    B, H, L, Dh = shape
    C = H * Dh
    c = mr.case(shape, 'cross')
    kt = mr.kernel_table(c['table'])
    o, _ = _attention(cuda, shape, c['pq'], c['pk'], c['pv'], kt, c['W'])
    rows = _checked_out(o, shape).permute(0, 2, 1, 3).reshape(B * L, C)
    img, flag = _attention(cuda, shape, c['pq'], c['pk'], c['pv'], kt, c['W'], form='o_split', o_ld=o_ld)
    assert flag == 0
    g = img.view(B * L, o_ld // 32, 2, 32)
    cols = torch.stack([g[:, :, 0].reshape(B * L, o_ld), g[:, :, 1].reshape(B * L, o_ld)])
    assert (cols[:, :, C:] == SENTINEL).all(), 'the kernel wrote beyond heads * Dh'
    assert (cols[:, :, :C] != SENTINEL).all()
    dec = ar.decode_o_split(img.view(torch.float16), B * L, o_ld, 6)[:, :C]
    assert torch.isfinite(dec).all()
    assert ((dec - rows).abs() <= 2.0 ** -21 * rows.abs() + 2.0 ** -30).all(), (dec - rows).abs().max().item()


@pytest.mark.parametrize('shape', [(2, 3, 64, 32), (1, 2, 256, 72)], ids=_id)
def test_flash_zero_table_vs_unbiased(cuda, report, shape):
    """A zero table against the unbiased kernel on the same planes. NOT bit for bit, by design: the unbiased kernel
    evaluates each exponent as one FMA, fma(s, sl2, ep - m), while the biased one rounds s' = fma(s, sl2, bias) first
    (the maximum is taken over s') and then adds ep - m: two roundings of exponents of magnitude < 2^7 (<= 2^-18 each)
    where the unbiased kernel has one, so the exponents differ by <= 2^-17 and each probability by a relative
    2^-17 ln 2; numerator and denominator of a convex combination of v rows both move by that, so the outputs differ
    by <= 2 * 2^-17 ln 2 max|v| < 2^-16 max|v|: the documented bound (measured: see the parity report). Both meet
    the float64 bound."""
    c = ar.case(shape, 'peaked')
    W = mr.grid_w(shape[2])
    zero = torch.zeros((shape[1], (2 * W - 1) ** 2))
    a, _ = _attention(cuda, shape, c['pq'], c['pk'], c['pv'], None, 0)
    b, _ = _attention(cuda, shape, c['pq'], c['pk'], c['pv'], zero, W)
    x, y = _checked_out(a, shape), _checked_out(b, shape)
    diff = (x - y).abs().max().item()
    report(f'attn_flash_bias_zero_table_{_id(shape)}_vs_unbiased_over_scale', diff / c['scale'])
    print(f'zero table vs unbiased {_id(shape)}: {diff:.3e} (scale {c["scale"]:.3e})')
    assert diff <= 2.0 ** -16 * c['v'].abs().max().item(), diff
    assert (y - c['ref']).abs().max().item() <= c['bound']


def test_flash_bias_rejects_bad_grid(cuda):
    """L != W^2, W beyond the staged table or a per-head stride shorter than (2W - 1)^2: an argument error, no launch."""
    shape = (1, 2, 256, 64)
    c = mr.case((2, 2, 256, 64), 'rand')
    pq, pk, pv = (t[:1].contiguous() for t in (c['pq'], c['pk'], c['pv']))
    kt = mr.kernel_table(c['table'])
    for W, tab in ((8, kt), (16, kt[:, :900].contiguous())):
        with pytest.raises(ValueError):
            _attention(cuda, shape, pq, pk, pv, tab, W)
