"""Operator-level tests of the half-precision token GEMM (DM_MATH_FP16: csrc/linear_h16.hip linear_h16_kernel,
h16_image_kernel<0..2>, its plane writers and c_split), through dm_debug_token_gemm path 3 on the test's own buffers.

The mode rounds each operand once to fp16, so its result is NOT close to the fp32 product; what the kernel owes is
stated piecewise, and each piece is checked against float64:
  1. integer operands (token_h16_ref.exact_case): the result is exact in any order -- bit for bit;
  2. the A image: every element within half an fp16 ulp of the float64 prologue, plus the fp32 prologue's own error;
  3. the GEMM on the device's OWN image against float64 a'_dev w'^T (w' computed on the host): the roundings are in
     the operands, so the bound is the existing token tests' |out - ref64| <= 2 e32 + 2^-21 max|ref64| (x 1.13 + 4 ulp
     behind an activation, + the fp16x2 image term for the q / k / v planes, + half an fp16 ulp for c_split);
  4. against linear_k32 on the same case: |C_fp16 - C_fp16x2| <= (2^-10 + 2^-20) sum_k |a_k w_k| (times the
     epilogue's slope) + the bound of 3, and the two differ (a mode that silently ran linear_k32 would be equal);
  5. the range flag at the image pass, at c_split and at the planes; 6. refusals launch nothing.
Buffers are NaN / sentinel prefilled with pad columns and a sentinel tile of rows, as in tests/test_gpu_token_ops.py,
whose DeviceBackend, descriptor binding and checking helpers are reused. The checks are functions of a backend:
tests/test_token_h16_host.py dry-runs them against token_h16_ref.H16Emu on the CPU.
"""
import ctypes

import pytest
import torch

from tests import test_gpu_token_ops as tg
from tests import token_h16_ref as hr
from tests import token_ref as tr

pytestmark = pytest.mark.gpu

UNSUPPORTED = tg.UNSUPPORTED
P3 = hr.PATH


class H16Device(tg.DeviceBackend):
    """tests/test_gpu_token_ops.py's backend with path 3: single-plane images, the GroupNorm-affine tables, and a
    deliberately misaligned caller image for the refusal test."""
    name = 'h16-device'

    def gemm(self, s, stats32=None):
        if s.get('path', 0) != P3:
            return super().gemm(s, stats32)
        M, (N, K) = s['M'], s['W'].shape
        a_form = s.get('a_form', 0)
        keep = []

        def up(t):
            d = self._up(t)
            keep.append(d)
            return d

        def ptr(t):
            return None if t is None else up(t).data_ptr()

        d = tg.GemmDesc()
        d.M, d.N, d.K, d.path, d.a_form, d.sk = M, N, K, P3, a_form, s.get('sk', 0)
        if s.get('A') is not None:
            d.A, d.lda = ptr(s['A']), K
        d.W, d.bias = ptr(s['W']), ptr(s.get('bias'))
        d.alpha, d.act, d.split_ea = s.get('alpha', 1.0), s.get('act', 0), s['ea']
        if s.get('res') is not None:
            d.res, d.ld_res, d.res_mod = ptr(s['res']), N, s.get('res_mod', 0)
        if s.get('gate') is not None:
            gb = up(s['gmod'])
            d.gate, d.gate_pitch, d.gate_rows = gb.data_ptr() + 4 * s['gmod_off']['gate'], gb.shape[1], s['gate_rows']
        if s.get('ln'):
            mb, st = up(s['mod']), up(stats32)
            d.ln_stats, d.ln_pitch, d.ln_rows = st.data_ptr(), mb.shape[1], s['ln_rows']
            d.ln_shift = mb.data_ptr() + 4 * s['mod_off']['shift']
            d.ln_scale = mb.data_ptr() + 4 * s['mod_off']['scale']
        if s.get('pro'):
            d.pro_scale, d.pro_shift, d.pro_rows = ptr(s['pro_scale']), ptr(s['pro_shift']), s['pro_rows']
        flag = torch.zeros((1, ), dtype=torch.int32, device=self.dev)
        d.range_flag = flag.data_ptr()
        C = as_img = c_img = planes = None
        if a_form == 1:
            as_img = self._sent((M + tr.TILE) * K)
            d.as_img = as_img.data_ptr()
        elif a_form == 2:
            d.as_img = ptr(s['as_img']) + (2 if s.get('as_misalign') else 0)
        if s.get('ap'):
            ap = s['ap']
            n = (M // ap['L']) * ap['heads'] * 2 * ap['L'] * ap['Dh']
            planes = [self._sent(n + tr.PLANE_TAIL) for _ in range(3)]
            tgt = [planes[2]] * 3 if ap.get('vonly') else planes
            d.ap_q, d.ap_k, d.ap_v = (t.data_ptr() for t in tgt)
            d.ap_vonly, d.ap_L, d.ap_heads, d.ap_Dh, d.ap_legacy = ap.get('vonly', 0), ap['L'], ap['heads'], ap['Dh'], ap.get('legacy', 0)
            d.ap_alpha, d.ap_bscale, d.ap_ea, d.ap_eb, d.ap_ev = ap['alpha'], ap.get('bscale', 0.0), ap['ea'], ap['eb'], ap['ev']
        elif s.get('c_split'):
            c_img = self._sent((M + tr.TILE) * N)
            d.c_split, d.c_split_ea = c_img.data_ptr(), s['c_split_ea']
        else:
            C = torch.full((M + tr.TILE, N + tr.PAD), float('nan'), device=self.dev)
            d.C, d.ldc = C.data_ptr(), N + tr.PAD
        rc = self.L.dm_debug_token_gemm(ctypes.byref(d), self._stream())
        if rc not in (0, UNSUPPORTED):
            self._lib.check(rc, 'dm_debug_token_gemm')
        cpu = lambda t: None if t is None else t.cpu()  # noqa: E731
        return dict(C=cpu(C), as_img=cpu(as_img), c_img=cpu(c_img), flag=int(flag.item()), rc=rc,
                    planes=None if planes is None else tuple(p.cpu() for p in planes))


@pytest.fixture(scope='module')
def be(cuda):
    return H16Device(cuda)


# ----------------------------------------------------------------------------------------------- the checks
def checked_plane(img, M, ld):
    """A single-plane image [M][ld] (int16 bits, sentinel prefill): rows past M keep the sentinel, nothing inside does,
    everything is finite -> the int16 bits of the M rows."""
    n = M * ld
    assert img.numel() == (M + tr.TILE) * ld
    assert (img[n:] == tr.SENT16).all(), 'the kernel wrote image rows past M'
    assert (img[:n] != tr.SENT16).all(), 'an image element was not written'
    assert torch.isfinite(img[:n].view(torch.float16).float()).all()
    return img[:n]


def check_exact(be, M, N, K, a_form):
    c = hr.exact_case(M, N, K)
    r = be.gemm(dict(c, path=P3, a_form=a_form))
    assert r['flag'] == 0
    got = tg.checked_c(r, M, N)
    want = c['A'].double() @ c['W'].double().T
    assert torch.equal(got.double(), want), (got.double() - want).abs().max().item()
    if a_form == 1:   # the image of integers times 2^6 is exact too
        bits = checked_plane(r['as_img'], M, K)
        assert torch.equal(hr.decode_image(bits, M, K, tr.EA), c['A'].double())


def check_image(be, report, c, key, stats=None):
    """Items 2 and 3 on one case with a prologue: the image against float64, then the GEMM's output against float64
    on that image. -> (the decoded image, the output)."""
    M, (N, K) = c['M'], c['W'].shape
    r = be.gemm(dict(c, path=P3, a_form=1), stats)
    assert r['rc'] == 0 and r['flag'] == 0
    a64 = hr.decode_image(checked_plane(r['as_img'], M, K), M, K, c['ea'])
    y, bound, e32, scale = hr.image_bound(c, stats)
    err = (a64 - y).abs()
    margin = (err / bound).max().item()
    print(f'{key}_image: err {err.max().item():.3e} prologue e32 {e32:.3e} max|y| {scale:.3e} margin {margin:.3f}')
    report(f'{key}_image_margin', margin)
    assert (err <= bound).all(), (key, err.max().item(), margin)
    got = tg.checked_c(r, M, N)
    tg.close(got, hr.image_refs(c, a64), report, key + '_gemm')
    # the temporary-image form (a_form 0) and the caller's-image form (a_form 2) are the same launches
    r0 = be.gemm(dict(c, path=P3, a_form=0), stats)
    assert r0['rc'] == 0 and r0['flag'] == 0
    assert torch.equal(tg.checked_c(r0, M, N), got), 'a_form 0 and a_form 1 differ'
    plain = {k: v for k, v in c.items() if k not in ('ln', 'pro', 'A')}
    r2 = be.gemm(dict(plain, path=P3, a_form=2, as_img=r['as_img'][:M * K]))
    assert r2['rc'] == 0 and r2['flag'] == 0
    assert torch.equal(tg.checked_c(r2, M, N), got), 'a_form 2 on the same image differs'
    return a64, got


def check_ln_image(be, report, B, T, K, dist):
    c = tr.ln_case(B, T, K, 32, dist)
    stats, _, _ = be.row_stats(c['A'])
    check_image(be, report, c, f'h16_ln_{B}x{T}_k{K}_{dist}', stats)


def check_gn_image(be, report, B, T, K):
    check_image(be, report, hr.gn_case(B, T, K), f'h16_gn_{B}x{T}_k{K}')


def check_vs_split(be, report, c, key, got, stats=None):
    """Item 4: the same case on linear_k32 (path 0, pre-split A). `got`: the half-precision output."""
    M, N = c['M'], c['W'].shape[0]
    rx = be.gemm(dict(c, path=0, a_form=1), stats)
    assert rx['rc'] == 0 and rx['flag'] == 0
    cx = tg.checked_c(rx, M, N)
    assert not torch.equal(cx, got), 'the half-precision path returned linear_k32\'s result'
    a16, _ = hr.a_image(c, stats)
    refs = hr.image_refs(c, torch.ldexp(a16.double(), torch.tensor(-c['ea'])))
    bound = hr.H16_REL * hr.sum_abs(c, stats) * hr.epilogue_slope(c) + refs['bound']
    dist = (got.double() - cx.double()).abs()
    margin = (dist / bound).max().item()
    print(f'{key}_vs_fp16x2: max distance {dist.max().item():.3e} margin {margin:.3f}')
    report(f'{key}_vs_fp16x2_margin', margin)
    assert (dist <= bound).all(), (key, dist.max().item(), margin)


def check_epilogue(be, report, c, key, stats=None):
    """Items 3 and 4 on a C-output case."""
    M, (N, K) = c['M'], c['W'].shape
    r = be.gemm(dict(c, path=P3, a_form=1), stats)
    assert r['rc'] == 0 and r['flag'] == 0
    a64 = hr.decode_image(checked_plane(r['as_img'], M, K), M, K, c['ea'])
    got = tg.checked_c(r, M, N)
    tg.close(got, hr.image_refs(c, a64), report, key)
    check_vs_split(be, report, c, key, got, stats)
    return got


def check_gate(be, report, T, N, kind):
    check_epilogue(be, report, tr.gate_case(T, N, kind), f'h16_{kind}_t{T}_n{N}')


def check_act_chain(be, report, M, N, K):
    """fc1's form (LN prologue, GELU-tanh at saturating biases) to C and as the c_split plane, then fc2 on it."""
    c = tr.act_case(M, N, K, 2)
    key = f'h16_fc1_{M}x{N}x{K}'
    stats, _, _ = be.row_stats(c['A'])
    got = check_epilogue(be, report, c, key + '_gelu', stats)
    pos, neg = c['sat_cols'][:8], c['sat_cols'][8:]
    assert (got[:, neg] == 0).all() and (got[:, pos] > 30).all()
    r = be.gemm(dict(c, path=P3, a_form=0, c_split=True, c_split_ea=6), stats)
    assert r['rc'] == 0 and r['flag'] == 0
    bits = checked_plane(r['c_img'], M, N)
    # the producer form is the image pass's expression on the fp32 output: bit-identical to rounding `got`
    assert torch.equal(bits, torch.ldexp(got, torch.tensor(6)).to(torch.float16).reshape(-1).view(torch.int16)), \
        'c_split differs from the image pass of the same output'
    dec = hr.decode_image(bits, M, N, 6)
    s2 = dict(c['fc2'], path=P3, a_form=2, as_img=r['c_img'][:M * N])
    r2 = be.gemm(s2)
    assert r2['rc'] == 0 and r2['flag'] == 0
    tg.close(tg.checked_c(r2, M, 64), hr.image_refs(s2, dec), report, key + '_fc2_chain')


def check_silu(be, report):
    M, N, K = tr.ACT_SHAPES[0]
    c = tr.act_case(M, N, K, 1)
    stats, _, _ = be.row_stats(c['A'])
    check_epilogue(be, report, c, f'h16_silu_{M}x{N}x{K}', stats)


def check_planes(be, report, shape, flags, bscale_on):
    """The q / k / v planes (hi + lo pieces of the fp32 accumulator) against float64 a'_dev w'^T + bias."""
    c = tr.plane_case(shape, flags.get('legacy', 0), flags.get('vonly', 0), bscale_on)
    ap, B, M = c['ap'], c['B'], c['M']
    K = c['W'].shape[1]
    key = 'h16_planes_' + 'x'.join(map(str, shape)) + ''.join('_' + k for k in flags) + f'_bs{bscale_on}'
    r = be.gemm(dict(c, path=P3, a_form=1))
    assert r['rc'] == 0 and r['flag'] == 0
    a64 = hr.decode_image(checked_plane(r['as_img'], M, K), M, K, c['ea'])
    dec = tg.decode_planes(r['planes'], c)
    w = hr.w_rounded(c['W'])
    y64 = a64 @ w.double().T + c['bias'].double()
    y32 = a64.float() @ w.T + c['bias']
    p64, p32 = tr.rows_to_heads(y64, ap, B), tr.rows_to_heads(y32, ap, B)
    for p, (name, sc, e) in enumerate(zip('qkv', tr.plane_scales(ap), (ap['ea'], ap['eb'], ap['ev']))):
        if dec[p] is None:
            continue
        f = torch.tensor(sc, dtype=tr.F32)
        ref = p64[p] * f.double()
        e32 = ((p32[p] * f).double() - ref).abs().max().item()
        scale = ref.abs().max().item()
        base = 2.0 * e32 + tr.REL * scale
        tg.close(dec[p], dict(ref=ref, e32=e32, scale=scale, base=base, bound=torch.full_like(ref, base)), report,
                 f'{key}_{name}', tr.image_term(ref, e))


EDGE_OK, EDGE_BAD = tg.EDGE_OK, tg.EDGE_BAD


def check_range_flags(be):
    """65504 2^-6 keeps the flag clear, 2^10 raises it: at the image pass (no prologue, and through the LN shift), at
    the c_split producer, at the planes. The backend zeroes the flag before each launch."""
    M, N, K = 128, 128, 64
    base = hr.exact_case(M, N, K)
    for val, want in ((EDGE_OK, 0), (EDGE_BAD, 1)):
        A = base['A'].clone()
        A[77, 21] = val
        c = dict(base, A=A)
        for a_form in (0, 1):
            r = be.gemm(dict(c, path=P3, a_form=a_form))
            assert r['rc'] == 0 and r['flag'] == want, ('image pass', a_form, val, r['flag'])
            if not want:   # 65504 = 2047 x 2^5: still exact
                assert torch.equal(tg.checked_c(r, M, N).double(), A.double() @ base['W'].double().T)
        # through the LayerNorm shift: constant rows normalise to exactly 0, so the image holds the shift
        rc = tr.rows_case(5, 64, 'const')
        buf = rc['mod']['buf'].clone()
        buf[1, rc['mod']['shift'] + 9] = val
        sh, sc = rc['mod']['shift'], rc['mod']['scale']
        s = dict(M=5, A=rc['x'], W=torch.zeros((32, 64)), ln=True, ln_rows=rc['per'], mod=buf, ea=tr.EA,
                 ln_shift=buf[:, sh:sh + 64], ln_scale=buf[:, sc:sc + 64], mod_off=dict(shift=sh, scale=sc),
                 path=P3, a_form=1)
        stats, _, _ = be.row_stats(rc['x'])
        r = be.gemm(s, stats)
        assert r['rc'] == 0 and r['flag'] == want, ('image pass, LN', val, r['flag'])
        # c_split at 2^6 of a GEMM whose image is taken at 2^0 (in range either way); selection weights
        perm = tr.perm_case(M, N, K)
        A = base['A'].clone()
        A[77, int(perm['perm'][5])] = val
        r = be.gemm(dict(M=M, A=A, W=perm['W'], ea=0, path=P3, a_form=0, c_split=True, c_split_ea=6))
        assert r['rc'] == 0 and r['flag'] == want, ('c_split', val, r['flag'])
        if not want:
            dec = hr.decode_image(checked_plane(r['c_img'], M, N), M, N, 6)
            assert torch.equal(dec, A[:, perm['perm']].double())
    # the planes: identity weights, N = K = 192 = 3 x (2 heads x 32): A column c lands in q (c < 64), k or v
    M, K = 128, 192
    g = torch.Generator().manual_seed(7)
    A0 = torch.randint(-8, 9, (M, K), generator=g).float()
    ap = dict(L=128, heads=2, Dh=32, legacy=0, vonly=0, alpha=1.0, bscale=0.0, ea=6, eb=6, ev=6)
    for part in range(3):
        for val, want in ((EDGE_OK, 0), (EDGE_BAD, 1)):
            A = A0.clone()
            A[33, 64 * part + 40] = val
            c = dict(M=M, B=1, A=A, W=torch.eye(K), ea=0, ap=ap)
            r = be.gemm(dict(c, path=P3, a_form=0))
            assert r['rc'] == 0 and r['flag'] == want, ('planes', part, val, r['flag'])
            if not want:
                dec = tg.decode_planes(r['planes'], c)
                rows = tr.rows_to_heads(A.double(), ap, 1)
                for p in range(3):
                    assert torch.equal(dec[p], rows[p])


REFUSED = [
    dict(K=96),                      # K % 64
    dict(N=30),                      # N % 4
    dict(c_split=True, N=32),        # c_split feeds a GEMM with K = N: N % 64
    dict(a_form=2, as_misalign=1),   # the image rows must be 16-byte aligned
    dict(sk=1),                      # no split-K tail in this arithmetic
]


def check_refusals(be):
    for kw in REFUSED:
        M, N, K = 128, kw.get('N', 64), kw.get('K', 64)
        g = torch.Generator().manual_seed(3)
        s = dict(M=M, A=torch.randn((M, K), generator=g), W=torch.randn((N, K), generator=g), ea=tr.EA, path=P3,
                 a_form=kw.get('a_form', 0), sk=kw.get('sk', 0), as_misalign=kw.get('as_misalign', 0))
        if kw.get('c_split'):
            s.update(c_split=True, c_split_ea=6)
        if s['a_form'] == 2:
            s['as_img'] = torch.zeros((M * K + 8, ), dtype=torch.int16)
        r = be.gemm(s)
        assert r['rc'] == UNSUPPORTED, (kw, r['rc'])
        assert r['flag'] == 0
        if r['C'] is not None:
            assert torch.isnan(r['C']).all()
        if r['c_img'] is not None:
            assert (r['c_img'] == tr.SENT16).all()


# ------------------------------------------------------------------------------------------------ the tests
_mnk = tg._mnk


@pytest.mark.parametrize('a_form', [0, 1])
@pytest.mark.parametrize('shape', hr.EXACT_SHAPES, ids=_mnk)
def test_exact_cases_bit_for_bit(be, shape, a_form):
    """1. Integer operands: one stage; a partial M tile with N no multiple of the block; N = 32 with an odd stage
    count; three column tiles."""
    check_exact(be, *shape, a_form)


@pytest.mark.parametrize('dist', tr.LN_DISTS)
@pytest.mark.parametrize('K', tr.LN_K)
@pytest.mark.parametrize('B,T', tr.LN_BT + tr.LN_BT_SMALL, ids=[_mnk(c) for c in tr.LN_BT + tr.LN_BT_SMALL])
def test_image_ln_modulate(be, report, B, T, K, dist):
    """2 + 3. The LayerNorm + modulate image (per-image tables O(1) apart inside a NaN-filled buffer, image boundaries
    mid-tile at T = 144 / 192, fewer than 128 rows per image at T = 16 / 64) and the GEMM on it."""
    check_ln_image(be, report, B, T, K, dist)


@pytest.mark.parametrize('K', hr.GN_K)
@pytest.mark.parametrize('B,T', hr.GN_BT, ids=[_mnk(c) for c in hr.GN_BT])
def test_image_groupnorm_affine(be, report, B, T, K):
    check_gn_image(be, report, B, T, K)


@pytest.mark.parametrize('T,N', tr.GATE_CASES, ids=[_mnk(c) for c in tr.GATE_CASES])
def test_gated_residual(be, report, T, N):
    check_gate(be, report, T, N, 'gate')


@pytest.mark.parametrize('kind', ['res_mod', 'alpha'])
def test_res_mod_and_alpha(be, report, kind):
    check_gate(be, report, 48, 64, kind)


@pytest.mark.parametrize('shape', tr.ACT_SHAPES, ids=_mnk)
def test_gelu_c_split_and_fc2_chain(be, report, shape):
    check_act_chain(be, report, *shape)


def test_silu_epilogue(be, report):
    check_silu(be, report)


@pytest.mark.parametrize('bscale_on', [0, 1])
@pytest.mark.parametrize('shape,flags', tr.PLANE_CASES, ids=[_mnk(s) + ''.join('_' + k for k in f) for s, f in tr.PLANE_CASES])
def test_attention_operand_planes(be, report, shape, flags, bscale_on):
    check_planes(be, report, shape, flags, bscale_on)


@pytest.mark.parametrize('shape', hr.WIDE_SHAPES, ids=_mnk)
def test_width_1280(be, report, shape):
    check_epilogue(be, report, hr.wide_case(*shape), 'h16_wide_' + _mnk(shape))


def test_range_flags(be):
    check_range_flags(be)


def test_hook_refuses_unsupported_descriptors(be):
    check_refusals(be)
