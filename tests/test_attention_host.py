"""CPU checks of the attention tests' own inputs and margins (tests/attention_ref.py), so that the GPU tests
(tests/test_gpu_attention_ops.py) cannot hide a failure behind a bad input or an unreachable bound:

* for every (shape, distribution) the GPU tests run, the fp32 emulation of attn_flash_kernel's arithmetic meets
  the bound the kernel is held to (2 e32 + 2^-21 max|ref|), every scaled operand has an fp16 image, and the
  `select` softmax is one-hot in float64;
* the plane and output-image packers round-trip, and the fp16x2 split reproduces its operand to 2^-22.
"""
import pytest
import torch

from tests import attention_ref as ar

ALL_CASES = ([(s, d) for s in ar.FLASH_SHAPES for d in ar.FLASH_DISTS + ['select']]
             + [(s, d) for s in ar.L256_SHAPES for d in ar.L256_DISTS])


def _id(shape, dist):
    return 'x'.join(map(str, shape)) + '-' + dist


@pytest.mark.parametrize('shape,dist', ALL_CASES, ids=[_id(*c) for c in ALL_CASES])
def test_case_inputs_and_emulation_margin(shape, dist):
    c = ar.case(shape, dist)
    for x, e in ((c['q'], ar.EA), (c['k'], ar.EB), (c['v'], ar.EV)):
        assert x.abs().max().item() * 2.0 ** e <= ar.FP16_MAX
    for p in (c['pq'], c['pk'], c['pv']):
        assert torch.isfinite(p.float()).all()
    emu = ar.flash_emulation(c['pq'], c['pk'], c['pv'])
    assert torch.isfinite(emu).all()
    err = (emu.double() - c['ref']).abs().max().item()
    assert err <= c['bound'], (err, c['e32'], c['scale'], err / max(c['e32'], 1e-300))
    if dist == 'select':
        qd, kd, vd = c['dec']
        assert torch.equal(qd.float(), c['q']) and torch.equal(kd.float(), c['k']) and torch.equal(vd.float(), c['v'])
        s = qd @ kd.transpose(-1, -2)
        top2 = s.topk(2, dim=-1)
        assert torch.equal(top2.indices[..., 0], c['pi'])
        assert (top2.values[..., 0] - top2.values[..., 1]).min().item() >= 128.0
        p = torch.softmax(s, dim=-1)
        # one-hot: the winner exactly 1, every other key below fp32's smallest subnormal (exp(-128) = 2^-184.7)
        assert (p.gather(-1, c['pi'][..., None]) == 1.0).all()
        assert p.scatter(-1, c['pi'][..., None], 0.0).max().item() < 2.0 ** -149
        want = ar.selected_rows(c['v'], c['pi']).double()
        assert (c['ref'] - want).abs().max().item() < 2.0 ** -149 * 8 * shape[2]
        assert (emu.double() - want).abs().max().item() <= 2.0 ** -20 * c['v'].abs().max().item()


def test_split_planes_reproduces_operand():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((4096, ), generator=g) * torch.exp2(torch.randint(-6, 4, (4096, ), generator=g).float())
    for e in (0, 6):
        hi, lo = ar.split_planes(x, e)
        s = x.double() * 2.0 ** e
        got = hi.double() + lo.double()
        # two fp16 roundings of 11 bits each: 2^-22 relative, and fp16's subnormal spacing 2^-24 below 2^-14
        assert ((got - s).abs() <= 2.0 ** -22 * s.abs() + 2.0 ** -25).all()
        assert torch.equal(hi, s.float().half())
    # integers up to 2^11 and +-1 are exact with a zero low piece
    hi, lo = ar.split_planes(torch.tensor([1.0, -1.0, 64.0, -8.0, 1100.0]), 6)
    assert torch.equal(hi.float(), torch.tensor([64.0, -64.0, 4096.0, -512.0, 70400.0]).half().float())
    assert (lo[:4] == 0).all()


def test_pack_planes_layout_round_trip():
    B, H, L, Dh = 2, 3, 64, 72
    q, k, v, _ = ar.generate((B, H, L, Dh), 'peaked')
    pq, pk, pv, (qd, kd, vd) = ar.pack_planes(q, k, v)
    assert pq.shape == (B, H, 2, L, Dh) and pk.shape == (B, H, 2, L, Dh) and pv.shape == (B, H, 2, Dh, L)
    assert all(p.dtype == torch.float16 and p.is_contiguous() for p in (pq, pk, pv))
    # element (b, h, piece, i, d) of the flat buffers, as the kernel indexes them
    flat_q, flat_v = pq.view(-1), pv.view(-1)
    b, h, i, d = 1, 2, 37, 55
    hi, lo = ar.split_planes(q[b, h, i, d], ar.EA)
    assert flat_q[((b * H + h) * 2 + 0) * L * Dh + i * Dh + d] == hi
    assert flat_q[((b * H + h) * 2 + 1) * L * Dh + i * Dh + d] == lo
    hi, lo = ar.split_planes(v[b, h, i, d], ar.EV)
    assert flat_v[((b * H + h) * 2 + 0) * L * Dh + d * L + i] == hi
    assert flat_v[((b * H + h) * 2 + 1) * L * Dh + d * L + i] == lo
    for got, want, x in zip(ar.unpack_planes(pq, pk, pv), (qd, kd, vd), (q, k, v)):
        assert torch.equal(got, want)
        assert ((want - x.double()).abs() <= 2.0 ** -22 * x.double().abs() + 2.0 ** -31).all()
    # integer operands survive exactly
    q, k, v, _ = ar.generate((1, 1, 64, 32), 'select')
    _, _, _, (qd, kd, vd) = ar.pack_planes(q, k, v)
    assert torch.equal(qd, q.double()) and torch.equal(kd, k.double()) and torch.equal(vd, v.double())


@pytest.mark.parametrize('M,C,o_ld', [(5, 216, 224), (3, 128, 128)])
def test_o_split_image_round_trip(M, C, o_ld):
    g = torch.Generator().manual_seed(M)
    x = torch.randn((M, C), generator=g)
    img = ar.pack_o_split(x, o_ld, 6)
    assert img.dtype == torch.float16 and img.numel() == M * 2 * o_ld
    # column c of row m: hi at m 2 o_ld + (c >> 5) 64 + (c & 31), lo 32 further (the kernel's store expression)
    m, c = M - 1, C - 3
    hi, lo = ar.split_planes(x[m, c], 6)
    at = m * 2 * o_ld + (c >> 5) * 64 + ((c & 31) >> 3) * 8 + (c & 7)
    assert img[at] == hi and img[at + 32] == lo
    dec = ar.decode_o_split(img, M, o_ld, 6)
    assert dec.shape == (M, o_ld)
    assert ((dec[:, :C] - x.double()).abs() <= 2.0 ** -22 * x.double().abs() + 2.0 ** -31).all()
    assert (dec[:, C:] == 0).all()
    ints = torch.randint(-8, 9, (M, C), generator=g).float()
    assert torch.equal(ar.decode_o_split(ar.pack_o_split(ints, o_ld, 6), M, o_ld, 6)[:, :C], ints.double())


def test_out_rows_inverse_of_kernel_layout():
    B, H, L, Dh = 2, 3, 4, 8
    x = torch.arange(B * H * L * Dh, dtype=torch.float32).view(B, H, L, Dh)
    rows = torch.full((B, L, H * Dh + 8), float('nan'))
    for h in range(H):
        rows[:, :, h * Dh:(h + 1) * Dh] = x[:, h]
    assert torch.equal(ar.out_rows(rows, H, Dh), x)
