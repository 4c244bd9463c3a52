"""CPU checks of the token-path tests' own inputs, layouts, margins and logic (tests/token_ref.py,
tests/test_gpu_token_ops.py), so that the GPU tests cannot hide a failure behind a bad input or an unreachable bound:

* split_exact is exact, the image / plane packers and decoders round-trip and sit where the kernels' store
  expressions put them, the modulation buffers are NaN outside the addressed tables;
* every non-flag case keeps |operand 2^e| within half the fp16 range, every flag case sits on the intended side
  of 65504;
* the fp32 emulation of the fp16x2 GEMM meets the bound the kernels are held to in every GEMM case (worst
  err / e32 and worst (err - 2 e32) / max|ref| printed and asserted);
* the GPU tests' checking functions run against token_ref.EmuBackend: their own logic (sentinels, bit-identity of
  the three prologue arms, refusals, flags, decoders) is proven here.
"""
import pytest
import torch

from tests import attention_ref as ar
from tests import test_gpu_token_ops as tg
from tests import token_ref as tr

EMU = tr.EmuBackend()


def _noreport(*a):
    pass


# ------------------------------------------------------------------------------------- operands and layouts
def test_split_exact_is_exact():
    g = torch.Generator().manual_seed(11)
    x = torch.randn((8192, ), generator=g) * torch.exp2(torch.randint(-8, 8, (8192, ), generator=g).float())
    for e in (0, 6):
        y = tr.split_exact(x, e)
        hi, lo = ar.split_planes(y, e)
        assert torch.equal(hi.double() + lo.double(), y.double() * 2.0 ** e)
        assert ((y.double() - x.double()).abs() <= 2.0 ** -22 * x.double().abs() + 2.0 ** -(25 + e)).all()
        assert torch.equal(tr.split_exact(y, e), y)
    # exact at 2^0 stays exact at 2^6 while in range (the c_split flag case relies on it)
    y = tr.split_exact(torch.randn((4096, ), generator=g) * 4.0, 0)
    assert torch.equal(tr.split_exact(y, 6), y)
    edge = torch.tensor([tg.EDGE_OK, tg.EDGE_BAD])
    assert torch.equal(tr.split_exact(edge[:1], 6), edge[:1]) and torch.equal(tr.split_exact(edge[:1], 0), edge[:1])
    assert edge[0] * 64 == tr.FP16_MAX and edge[1] * 64 > tr.FP16_MAX


def test_presplit_image_layout_is_the_kernels():
    """Element (m, c) of the pre-split A image / c_split: piece 0 at m 2K + (c / 32) 64 + ((c % 32) / 8) 8 + c % 8,
    piece 1 32 further (presplit_a_kernel, row_stats_split_*_kernel and linear_k32's c_split store)."""
    M, K = 5, 192
    g = torch.Generator().manual_seed(2)
    x = torch.randn((M, K), generator=g)
    img = ar.pack_o_split(x, K, tr.EA)
    for m, c in ((0, 0), (4, 191), (2, 37), (3, 104)):
        hi, lo = ar.split_planes(x[m, c], tr.EA)
        at = m * 2 * K + (c // 32) * 64 + ((c % 32) // 8) * 8 + c % 8
        assert img[at] == hi and img[at + 32] == lo
    # linear_k32's c_split store: 4 columns ncol .. ncol + 3 at m 2N + (ncol >> 5) 64 + (ncol & 31)
    ncol = 44
    at = 3 * 2 * K + (ncol >> 5) * 64 + (ncol & 31)
    assert torch.equal(img[at:at + 4], ar.split_planes(x[3, ncol:ncol + 4], tr.EA)[0])


@pytest.mark.parametrize('shape,flags', tr.PLANE_CASES)
def test_plane_column_maps(shape, flags):
    """rows_to_heads (vectorized) equals the plain per-column definition for every column order, and covers every
    (part, head, d) exactly once."""
    c = tr.plane_case(shape, flags.get('legacy', 0), flags.get('vonly', 0), 0)
    ap, B = c['ap'], c['B']
    N = c['W'].shape[0]
    y = torch.arange(c['M'] * N, dtype=torch.float64).reshape(c['M'], N)
    a, b = tr.rows_to_heads(y, ap, B), tr.heads_from_rows(y, ap, B)
    for p in range(3):
        assert (a[p] is None) == (b[p] is None) == bool(flags.get('vonly') and p < 2)
        if a[p] is not None:
            assert torch.equal(a[p], b[p])
    part, h, d = tr.plane_columns(ap)
    keys = set(zip(part.tolist(), h.tolist(), d.tolist()))
    assert len(keys) == N
    if flags.get('legacy'):   # per head [q; k; v]
        Dh = ap['Dh']
        assert (int(part[Dh]), int(h[Dh]), int(d[Dh])) == (1, 0, 0) and int(h[3 * Dh]) == 1
    # K is heads Dh rounded up to 64 with zero weights beyond
    C = ap['heads'] * ap['Dh']
    assert c['W'].shape[1] % 64 == 0 and (c['W'][:, C:] == 0).all()


def test_modulation_buffers_are_nan_outside_the_tables():
    g = torch.Generator().manual_seed(4)
    buf, off = tr.mod_tables(3, 64, g)
    mask = torch.zeros_like(buf, dtype=torch.bool)
    for n in ('shift', 'scale', 'gate'):
        assert off[n] % 4 == 0 and buf.shape[1] % 4 == 0 and buf.shape[1] > off[n] + 64
        mask[:, off[n]:off[n] + 64] = True
        t = tr.table(buf, off, n, 64)
        assert torch.isfinite(t).all()
        # the images' tables differ by O(1) on average
        assert (t[1] - t[0]).mean().abs().item() > 0.2
    assert torch.isnan(buf[~mask]).all() and torch.isfinite(buf[mask]).all()
    assert len({off[n] for n in off}) == 3


def test_row_distributions():
    g = torch.Generator().manual_seed(9)
    x = tr.token_rows('offset', 64, 320, g)
    assert abs(x.mean().item() - 50.0) < 0.01 and abs(x.std().item() - 0.05) < 0.005
    x = tr.token_rows('spike', 64, 320, g)
    assert ((x == 1e3).sum(dim=1) == 1).all() and x.abs().median().item() < 0.05
    x = tr.token_rows('const', 5, 64, g)
    st = tr.row_stats_f32(x)
    assert torch.equal(st[:, 0], torch.full((5, ), 3.0))
    assert ((st[:, 1].double() - tr.LN_EPS ** -0.5).abs() <= 2.0 ** -22 * tr.LN_EPS ** -0.5).all()
    x = tr.token_rows('mixed', 256, 64, g)
    assert {0.0, 30.0, -30.0, 300.0} == set(x.mean(dim=1).div(10).round().mul(10).tolist())


# ------------------------------------------------------------------------------------------ ranges and margins
def _gemm_cases():
    """Every GEMM case the GPU tests run, as (key, spec, second spec of a chain | None)."""
    for B, T in tr.LN_BT + tr.LN_BT_SMALL:
        for K in tr.LN_K:
            for N in tr.LN_N:
                for dist in tr.LN_DISTS:
                    yield f'ln_{B}x{T}_k{K}_n{N}_{dist}', tr.ln_case(B, T, K, N, dist)
    for T, N in tr.GATE_CASES:
        yield f'gate_t{T}_n{N}', tr.gate_case(T, N, 'gate')
    for kind in ('res_mod', 'alpha'):
        yield kind, tr.gate_case(48, 64, kind)
    for shape in tr.ACT_SHAPES:
        yield 'gelu_' + tg._mnk(shape), tr.act_case(*shape, 2)
    yield 'silu', tr.act_case(*tr.ACT_SHAPES[0], 1)
    for shape, flags in tr.PLANE_CASES:
        for bs in (0, 1):
            yield 'planes_' + tg._mnk(shape), tr.plane_case(shape, flags.get('legacy', 0), flags.get('vonly', 0), bs)
    # the depths of the real models (DiT-XL/2: K = 1152; a wider one), LN-modulated rows of mean 50, std 0.05
    for K in (1152, 1536):
        yield f'ln_deep_k{K}', tr.ln_case(2, 128, K, 64, 'offset')


def test_every_non_flag_case_stays_within_half_the_fp16_range():
    worst = 0.0
    for key, c in _gemm_cases():
        stats = tr.row_stats_f32(c['A']) if c.get('ln') else None
        m = tr.max_scaled_operands(c, stats)
        e = tr.gemm_emulation(c, stats)
        assert e['flag'] == 0
        if c.get('ap'):
            for y, sc in zip(tr.rows_to_heads(e['y'], c['ap'], c['B']), tr.plane_scales(c['ap'])):
                if y is not None:
                    m = max(m, (y * sc).abs().max().item() * 64.0)
        if key.startswith('gelu'):
            m = max(m, e['y'].abs().max().item() * 64.0)     # the c_split image at 2^6
        assert m <= tr.HALF_RANGE, (key, m)
        worst = max(worst, m)
    for rows in tr.ROWK_ROWS:
        for D in tr.ROWK_D:
            for dist in tr.ROW_DISTS:
                c = tr.rows_case(rows, D, dist)
                y = tr.ln_modulate(c['x'], tr.row_stats_f32(c['x']), c['ln_scale'], c['ln_shift'], c['per'], tr.F32)
                m = y.abs().max().item() * 2.0 ** tr.EA
                assert m <= tr.HALF_RANGE, (rows, D, dist, m)
                worst = max(worst, m)
    print(f'largest scaled operand {worst:.1f} of {tr.HALF_RANGE}')


def test_gemm_emulation_meets_the_bound_in_every_case():
    """The fp16x2 arithmetic restated in fp32 against float64: within 2 e32 + 2^-21 max|ref| (x 1.13 + 4 ulp behind
    an activation) in every case, on linear_k32's row scales and gemm.hip's matrix-wide scale; the worst
    err / e32 and the worst (err - 2 e32) / max|ref| (the share of the 2^-21 term used) are printed."""
    worst_ratio, worst_share, at = 0.0, float('-inf'), None
    for key, c in _gemm_cases():
        stats = tr.row_stats_f32(c['A']) if c.get('ln') else None
        refs = tr.gemm_refs(c, stats)
        for path in (0, 1):
            y = tr.gemm_emulation(dict(c, path=path), stats)['y']
            err = (y.double() - refs['ref']).abs()
            assert (err <= refs['bound']).all(), (key, path, err.max().item(), refs['e32'], refs['scale'])
            ratio = err.max().item() / refs['e32']
            share = (err.max().item() - 2.0 * refs['e32']) / refs['scale']
            if ratio > worst_ratio:
                worst_ratio, at = ratio, (key, path)
            worst_share = max(worst_share, share)
    print(f'worst err / e32 {worst_ratio:.3f} at {at}; worst (err - 2 e32) / max|ref| {worst_share:.3e} '
          f'({worst_share / tr.REL:.3f} of 2^-21)')
    assert worst_share <= tr.REL
    assert worst_ratio <= 2.0   # the emulation stays below 2 e32 alone (the 2^-21 term is the kernels' margin)


def test_fp32_path_emulation_is_the_yardstick():
    c = tr.gate_case(16, 64, 'gate')
    refs = tr.gemm_refs(c)
    y = tr.gemm_emulation(dict(c, path=2))['y']
    assert (y.double() - refs['ref']).abs().max().item() <= refs['e32'] * 1.0000001


# ------------------------------------------------------------------------------------- dry runs of the checks
@pytest.mark.parametrize('a_form', [0, 1])
@pytest.mark.parametrize('path', [0, 1])
@pytest.mark.parametrize('shape', tr.PERM_SHAPES, ids=tg._mnk)
def test_dry_permutation(shape, path, a_form):
    tg.check_permutation(EMU, *shape, path, a_form)


@pytest.mark.parametrize('dist', tr.LN_DISTS)
@pytest.mark.parametrize('B,T,K,N', [(2, 128, 64, 32), (3, 144, 320, 192), (2, 192, 192, 32), (9, 16, 192, 192),
                                     (3, 64, 320, 32)])
def test_dry_ln(B, T, K, N, dist):
    tg.check_ln(EMU, _noreport, B, T, K, N, dist)


def test_dry_ln_catches_a_wrong_image_index():
    """The check fails when rows are modulated with the neighbouring image's tables, or with ln_rows off by one
    tile: the inputs make such faults O(1), not 1e-4."""
    class WrongImage(tr.EmuBackend):
        def gemm(self, s, stats32=None):
            if s.get('ln'):
                s = dict(s, ln_rows=s['ln_rows'] + 16)
            return super().gemm(s, stats32)
    with pytest.raises(AssertionError):
        tg.check_ln(WrongImage(), _noreport, 3, 144, 64, 32, 'std')


@pytest.mark.parametrize('path', [0, 2])
def test_dry_gate(path):
    for T, N in tr.GATE_CASES:
        tg.check_gate(EMU, _noreport, T, N, 'gate', path)
    for kind in ('res_mod', 'alpha'):
        tg.check_gate(EMU, _noreport, 48, 64, kind, path)


def test_dry_gate_catches_a_wrong_gate_row():
    class WrongGate(tr.EmuBackend):
        def gemm(self, s, stats32=None):
            return super().gemm(dict(s, gate_rows=s['gate_rows'] * 2) if s.get('gate') is not None else s, stats32)
    with pytest.raises(AssertionError):
        tg.check_gate(WrongGate(), _noreport, 16, 64, 'gate', 0)


@pytest.mark.parametrize('shape,a_form', list(zip(tr.ACT_SHAPES, (0, 1))))
def test_dry_act_chain(shape, a_form):
    tg.check_act_chain(EMU, _noreport, *shape, a_form)


def test_dry_silu():
    tg.check_silu(EMU, _noreport)


@pytest.mark.parametrize('bscale_on', [0, 1])
@pytest.mark.parametrize('shape,flags', tr.PLANE_CASES)
def test_dry_planes(shape, flags, bscale_on):
    tg.check_planes(EMU, _noreport, shape, flags, bscale_on, 1)


def test_dry_planes_catch_a_wrong_column_order():
    class WrongOrder(tr.EmuBackend):
        def gemm(self, s, stats32=None):
            return super().gemm(dict(s, ap=dict(s['ap'], legacy=1 - s['ap'].get('legacy', 0))), stats32)
    with pytest.raises(AssertionError):
        tg.check_planes(WrongOrder(), _noreport, (2, 4, 64, 32), {'legacy': 1}, 0, 1)


def test_dry_planes_feed_attention():
    tg.check_planes_feed_attention(EMU, _noreport)


def test_dry_range_flags():
    tg.check_range_flags(EMU)


@pytest.mark.parametrize('dist', tr.ROW_DISTS)
@pytest.mark.parametrize('rows,D', [(5, 64), (64, 320), (5, 1280), (5, 1344), (64, 2048)])
def test_dry_row_kernels(rows, D, dist):
    tg.check_row_kernels(EMU, _noreport, rows, D, dist)


def test_dry_patchify_embed_refusals():
    for p in (2, 4, 8):
        tg.check_patchify(EMU, p, 16, 4)
    tg.check_patchify(EMU, 2, 8, 8)
    tg.check_embed(EMU, _noreport, 64)
    tg.check_refusals(EMU)


def test_sentinel_layouts():
    """What the backends allocate: NaN pad columns and a NaN tile of rows for C, sentinel rows for the images, a
    sentinel tail for the planes -- and checked_c / checked_img reject a stray write or a missing one."""
    c = tr.perm_case(128, 128, 64)
    r = EMU.gemm(dict(c, path=0, a_form=1))
    assert r['C'].shape == (128 + tr.TILE, 128 + tr.PAD)
    assert r['as_img'].numel() == (128 + tr.TILE) * 2 * 64
    bad = dict(r, C=r['C'].clone())
    bad['C'][3, 130] = 0.0
    with pytest.raises(AssertionError):
        tg.checked_c(bad, 128, 128)
    bad = dict(r, C=r['C'].clone())
    bad['C'][128, 0] = 0.0
    with pytest.raises(AssertionError):
        tg.checked_c(bad, 128, 128)
    bad = dict(r, C=r['C'].clone())
    bad['C'][5, 5] = float('nan')
    with pytest.raises(AssertionError):
        tg.checked_c(bad, 128, 128)
    img = r['as_img'].clone()
    img[128 * 2 * 64 + 1] = 0
    with pytest.raises(AssertionError):
        tg.checked_img(img, 128, 64)
    img = r['as_img'].clone()
    img[77] = tr.SENT16
    with pytest.raises(AssertionError):
        tg.checked_img(img, 128, 64)
    assert torch.isnan(torch.tensor([tr.SENT16], dtype=torch.int16).view(torch.float16).float()).all()
