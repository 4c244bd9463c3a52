"""Operator-level tests of the attention kernels (csrc/attention.hip) on adversarial scores.

dm_debug_attention launches attn_fused() on the test's own device buffers, so attn_flash_kernel (every ADM and DiT
attention block), attn_presplit_kernel and attn_fused_kernel are compared directly with a float64 softmax(q k^T) v of
the same (decoded fp16x2) operands, instead of through whole-model forwards whose synthetic weights give nearly flat
scores: peaked, ramped, descending and shifted scores make the online-softmax rescale (corr from 1 down to 0, in both
orders) decide the result, and one-hot key selection with integer v rows catches any mis-permuted key, head, image
or d row of the V^T LDS image and the 16x16x32 tail. The bound is the project's own for fp16x2 against fp32
arithmetic: 2 e32 + 2^-21 max|ref|, e32 the error of torch's float32 attention on the same operands (inputs and
margins are validated on the CPU by tests/test_attention_host.py). The err / e32 ratios go to the parity report.
"""
import ctypes

import pytest
import torch

from tests import attention_ref as ar

pytestmark = pytest.mark.gpu

PAD = 8   # untouched columns after heads * Dh in every `out` row


def _id(shape):
    return 'x'.join(map(str, shape))


def _attention(dev, shape, pq=None, pk=None, pv=None, qkv=None, alpha=1.0, b_scale=1.0, ev=ar.EV, o_ld=0,
               o_split_ea=6, form='out'):
    """dm_debug_attention on planes (CPU fp16 tensors in the kernel's layouts) or fp32 qkv rows [B L][3 heads Dh]
    (q | k | v column blocks). form 'out': fp32 rows of pitch heads Dh + PAD prefilled with NaN; 'o_split': the
    pre-split image of pitch o_ld prefilled with the sentinel. Returns (output on the CPU, range flag)."""
    from dmhip import _lib
    f = _lib.load().dm_debug_attention
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    f.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, cf, cf, ci, ci, ci, ci, vp, ci, vp, ci, ci, vp,
                  vp]
    B, H, L, Dh = shape
    C = H * Dh
    keep = [None if t is None else t.to(dev) for t in (pq, pk, pv, qkv)]
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    flag = torch.zeros((1, ), dtype=torch.int32, device=dev)
    out = img = None
    if form == 'out':
        out = torch.full((B, L, C + PAD), float('nan'), device=dev)
    else:
        img = torch.full((B * L * 2 * o_ld, ), SENTINEL, dtype=torch.int16, device=dev)
    _lib.check(f(p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), 3 * C if qkv is not None else 0, 0, C, 2 * C, Dh,
                 B, H, L, Dh, alpha, b_scale, ar.EA, ar.EB, ar.EP, ev, p(out), C + PAD, p(img), o_split_ea, o_ld,
                 flag.data_ptr(), torch.cuda.current_stream().cuda_stream), 'dm_debug_attention')
    res = out.cpu() if form == 'out' else img.cpu()
    return res, int(flag.item())


SENTINEL = 0x7e2a   # an fp16 NaN pattern no kernel writes


def _checked_out(o, shape):
    """The pad columns are still NaN, everything else finite -> [B, heads, L, Dh] float64."""
    B, H, L, Dh = shape
    assert torch.isnan(o[..., H * Dh:]).all(), 'the kernel wrote beyond heads * Dh'
    assert torch.isfinite(o[..., :H * Dh]).all()
    return ar.out_rows(o, H, Dh).double()


def _assert_close_f64(got, c, report, key):
    err = (got - c['ref']).abs().max().item()
    ratio = err / c['e32'] if c['e32'] > 0 else 0.0
    print(f'{key}: err {err:.3e} e32 {c["e32"]:.3e} ratio {ratio:.3f} bound {c["bound"]:.3e}')
    report(f'{key}_err_over_e32', ratio)
    assert err <= c['bound'], (key, err, c['e32'], c['scale'], ratio)


def _assert_selected(got, c, key):
    want = ar.selected_rows(c['v'], c['pi']).double()
    err = (got - want).abs().max().item()
    print(f'{key}: |out - v[pi]| {err:.3e}')
    assert err <= 2.0 ** -20 * c['v'].abs().max().item(), (key, err)


@pytest.mark.parametrize('dist', ar.FLASH_DISTS)
@pytest.mark.parametrize('shape', ar.FLASH_SHAPES, ids=_id)
def test_flash_vs_float64(cuda, report, shape, dist):
    """attn_flash_kernel against float64 on the decoded operands, every shape x distribution: pitched output with
    untouched pad columns, error <= 2 e32 + 2^-21 max|ref|."""
    c = ar.case(shape, dist)
    o, flag = _attention(cuda, shape, c['pq'], c['pk'], c['pv'])
    assert flag == 0
    _assert_close_f64(_checked_out(o, shape), c, report, f'attn_flash_{_id(shape)}_{dist}')


@pytest.mark.parametrize('shape', ar.FLASH_SHAPES, ids=_id)
def test_flash_key_selection(cuda, shape):
    """One-hot scores (the winner ahead by >= 128 nats), integer v rows: the output is v[pi(i)] to 2^-20 max|v| (a few
    fp32 roundings and the 2^-22 that P's split drops); rows differ by >= 1, so any mis-permuted key, head, image
    or d row fails."""
    c = ar.case(shape, 'select')
    o, _ = _attention(cuda, shape, c['pq'], c['pk'], c['pv'])
    _assert_selected(_checked_out(o, shape), c, f'attn_flash_{_id(shape)}_select')


@pytest.mark.parametrize('L,Dh', [(128, 72), (256, 32)])
def test_flash_batch_head_independence(cuda, L, Dh):
    """Replacing one (image, head)'s q, k, v leaves the other five slices' outputs bit-identical."""
    shape = (2, 3, L, Dh)
    q, k, v, _ = ar.generate(shape, 'peaked')
    base, _ = _attention(cuda, shape, *ar.pack_planes(q, k, v)[:3])
    q2, k2, v2, _ = ar.generate(shape, 'ramp40')
    b, h = 1, 1
    q, k, v = q.clone(), k.clone(), v.clone()
    q[b, h], k[b, h], v[b, h] = q2[b, h], k2[b, h], v2[b, h]
    other, _ = _attention(cuda, shape, *ar.pack_planes(q, k, v)[:3])
    x, y = _checked_out(base, shape), _checked_out(other, shape)
    for bb in range(2):
        for hh in range(3):
            if (bb, hh) == (b, h):
                assert not torch.equal(x[bb, hh], y[bb, hh])
            else:
                assert torch.equal(x[bb, hh], y[bb, hh]), (bb, hh)


@pytest.mark.parametrize('shape,o_ld', [((1, 3, 128, 72), 224), ((2, 2, 128, 64), 128)], ids=['dh72_ld224', 'dh64_ld128'])
@pytest.mark.parametrize('dist', ['peaked', 'select'])
def test_flash_o_split(cuda, shape, o_ld, dist):
    """The pre-split A image form (DiT's path) decodes to the `out` form of the same inputs within the fp16x2
    split's 2^-21 |out| + 2^-30 (fp16's subnormal spacing after the 2^-6 unscale); the columns in
    [heads Dh, o_ld) keep the sentinel; no range flag."""
    B, H, L, Dh = shape
    C = H * Dh
    q, k, v, _ = ar.generate(shape, dist)
    pq, pk, pv, _ = ar.pack_planes(q, k, v)
    o, _ = _attention(cuda, shape, pq, pk, pv)
    rows = _checked_out(o, shape).permute(0, 2, 1, 3).reshape(B * L, C)
    img, flag = _attention(cuda, shape, pq, pk, pv, o_ld=o_ld, form='o_split')
    assert flag == 0
    g = img.view(B * L, o_ld // 32, 2, 32)
    cols = torch.stack([g[:, :, 0].reshape(B * L, o_ld), g[:, :, 1].reshape(B * L, o_ld)])   # raw bits per column
    assert (cols[:, :, C:] == SENTINEL).all(), 'the kernel wrote beyond heads * Dh'
    assert (cols[:, :, :C] != SENTINEL).all()
    dec = ar.decode_o_split(img.view(torch.float16), B * L, o_ld, 6)[:, :C]
    assert torch.isfinite(dec).all()
    assert ((dec - rows).abs() <= 2.0 ** -21 * rows.abs() + 2.0 ** -30).all(), (dec - rows).abs().max().item()


def test_flash_o_split_range_flag(cuda):
    """ev = 0, a one-hot selection onto a v row of 1000s, then 1100s: with o_split_ea = 6 the image holds 64000
    (flag clear) and 70400 (beyond fp16: flag set); the `out` form never raises the flag."""
    shape = (1, 3, 128, 72)
    c = ar.case(shape, 'select')
    for val, want in ((1000.0, 0), (1100.0, 1)):
        v = c['v'].clone()
        v[0, 1, 17] = val
        pq, pk, pv, _ = ar.pack_planes(c['q'], c['k'], v, ev=0)
        _, flag = _attention(cuda, shape, pq, pk, pv, ev=0, o_ld=224, form='o_split')
        assert flag == want, (val, flag)
        o, flag = _attention(cuda, shape, pq, pk, pv, ev=0)
        assert flag == 0, val
        got = _checked_out(o, shape)
        assert (got - ar.selected_rows(v, c['pi']).double()).abs().max().item() <= 2.0 ** -20 * val


@pytest.mark.parametrize('dist', ar.L256_DISTS)
@pytest.mark.parametrize('kernel', ['presplit', 'fused'])
@pytest.mark.parametrize('shape', ar.L256_SHAPES, ids=_id)
def test_attention_l256_kernels_vs_float64(cuda, report, shape, kernel, dist):
    """attn_presplit_kernel<64> / <256> (planes) and attn_fused_kernel<64> / <256> (fp32 q | k | v rows, alpha =
    Dh^-1/2 applied and split in the kernel) through the same hook, against float64 and on key selection."""
    B, H, L, Dh = shape
    c = ar.case(shape, dist)
    if kernel == 'presplit':
        o, flag = _attention(cuda, shape, c['pq'], c['pk'], c['pv'])
    else:
        # alpha is a power of two for Dh = 64 / 256: q / alpha is exact and the kernel's fp32 (q / alpha) alpha split
        # at 2^ea gives the planes' operands exactly
        alpha = Dh ** -0.5
        assert alpha in (0.125, 0.0625)
        rows = [x.permute(0, 2, 1, 3).reshape(B * L, H * Dh) for x in (c['q'] / alpha, c['k'], c['v'])]
        o, flag = _attention(cuda, shape, qkv=torch.cat(rows, dim=1).contiguous(), alpha=alpha, b_scale=1.0)
    assert flag == 0
    got = _checked_out(o, shape)
    key = f'attn_{kernel}_{_id(shape)}_{dist}'
    if dist == 'select':
        _assert_selected(got, c, key)
    else:
        _assert_close_f64(got, c, report, key)
