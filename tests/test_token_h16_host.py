"""CPU checks of the half-precision token GEMM tests' own inputs, bounds and logic (tests/token_h16_ref.py,
tests/test_gpu_token_h16.py), in the manner of tests/test_token_host.py:

* the exact cases are exact: a 2^6 and w 2^er are fp16 values, the fp32 emulation in the kernel's K order, in the
  reverse order and as one fp32 matmul all equal float64, and no two rows / columns of operands or result agree;
* w' is piece 0 of the fp16x2 weight split and a' piece 0 of the fp16x2 A image (the mode reads the images the
  fp16x2 path already has);
* every checking function of the GPU tests runs against token_h16_ref.H16Emu (operands rounded with .half(), fp32
  accumulation in the kernel's K order): sentinels, bit-identities, flags, refusals and decoders are proven here, and
  the emulation sits inside every bound. Worst ratios over all cases (printed by test_margins_over_all_cases): GEMM
  err / e32 0.99 (the bound starts at 2 e32), fp16-to-fp16x2 distance / bound 0.25; the image at 0.998 of its bound,
  which is tight by construction (round-to-nearest reaches half an ulp; its room is the prologue term);
* the model-level emulation: the host forwards reproduce the fp32 fixtures without the patch (DiT 4.8e-7, MDT
  6.8e-7 against the REFERENCE's own mdt_c outputs) and round exactly the covered GEMMs with it.
"""
import pytest
import torch

from tests import attention_ref as ar
from tests import test_gpu_token_h16 as th
from tests import token_h16_ref as hr
from tests import token_ref as tr

EMU = hr.H16Emu()


def _noreport(*a):
    pass


@pytest.mark.parametrize('shape', hr.EXACT_SHAPES, ids=th._mnk)
def test_exact_cases_are_exact(shape):
    M, N, K = shape
    c = hr.exact_case(M, N, K)
    A, W = c['A'], c['W']
    want = A.double() @ W.double().T
    assert want.abs().max().item() <= 64 * K < 2 ** 24
    a16, flag = hr.a_image(c)
    w16, e = hr.w_image(W)
    assert flag == 0
    assert torch.equal(torch.ldexp(a16.double(), torch.tensor(-tr.EA)), A.double())
    assert torch.equal(torch.ldexp(w16.double(), -e[:, None]), W.double())
    assert (W.abs().amax(dim=1) > 0).all()
    # any order: the kernel's, the reverse, one matmul
    scale = torch.ldexp(torch.ones(N), -e - tr.EA)[None, :]
    fwd = hr.acc_h16(a16, w16) * scale
    rev = hr.acc_h16(a16.flip(1), w16.flip(1)) * scale
    one = (a16.float() @ w16.float().T) * scale
    for got in (fwd, rev, one):
        assert torch.equal(got.double(), want)
    # a wrong row / column / K group shows: operands and results pairwise distinct
    assert len({tuple(r) for r in A.tolist()}) == M and len({tuple(r) for r in W.tolist()}) == N
    assert len({tuple(r) for r in want.tolist()}) == M and len({tuple(r) for r in want.T.tolist()}) == N
    assert len({tuple(r) for r in A.view(M, K // 8, 8).transpose(0, 1).reshape(K // 8, -1).tolist()}) == K // 8


def test_operands_are_piece_0_of_the_fp16x2_images():
    g = torch.Generator().manual_seed(5)
    W = tr._weights(192, 128, g)
    w16, e = hr.w_image(W)
    w0, _ = ar.split_planes(torch.ldexp(W, e[:, None]), 0)
    assert torch.equal(w16.view(torch.int16), w0.view(torch.int16))
    c = tr.ln_case(3, 144, 192, 32, 'mixed')
    st = tr.row_stats_f32(c['A'])
    a16, _ = hr.a_image(c, st)
    _, a0, _ = tr.a_pieces(c, st)
    assert torch.equal(a16.view(torch.int16), a0.view(torch.int16))
    x = torch.tensor([1.0, 1.0 + 2.0 ** -10, 3.0e-5, 65504.0, 1000.0])
    assert torch.equal(hr.ulp16(x.double()), torch.tensor([2.0 ** -10, 2.0 ** -10, 2.0 ** -24, 32.0, 0.5], dtype=tr.F64))
    assert th.EDGE_OK * 64 == tr.FP16_MAX and th.EDGE_BAD * 64 > tr.FP16_MAX
    assert float(torch.tensor(th.EDGE_OK).half()) == th.EDGE_OK   # exact at 2^0 too (the c_split flag case)


@pytest.mark.parametrize('a_form', [0, 1])
@pytest.mark.parametrize('shape', hr.EXACT_SHAPES, ids=th._mnk)
def test_check_exact(shape, a_form):
    th.check_exact(EMU, *shape, a_form)


@pytest.mark.parametrize('dist', tr.LN_DISTS)
@pytest.mark.parametrize('B,T', tr.LN_BT + tr.LN_BT_SMALL)
def test_check_ln_image(B, T, dist):
    for K in tr.LN_K:
        th.check_ln_image(EMU, _noreport, B, T, K, dist)


@pytest.mark.parametrize('B,T', hr.GN_BT)
def test_check_gn_image(B, T):
    for K in hr.GN_K:
        th.check_gn_image(EMU, _noreport, B, T, K)


def test_check_epilogues():
    for T, N in tr.GATE_CASES:
        th.check_gate(EMU, _noreport, T, N, 'gate')
    for kind in ('res_mod', 'alpha'):
        th.check_gate(EMU, _noreport, 48, 64, kind)
    for shape in tr.ACT_SHAPES:
        th.check_act_chain(EMU, _noreport, *shape)
    th.check_silu(EMU, _noreport)
    for shape in hr.WIDE_SHAPES:
        th.check_epilogue(EMU, _noreport, hr.wide_case(*shape), 'wide')


@pytest.mark.parametrize('shape,flags', tr.PLANE_CASES)
def test_check_planes(shape, flags):
    for bs in (0, 1):
        th.check_planes(EMU, _noreport, shape, flags, bs)


def test_check_flags_and_refusals():
    th.check_range_flags(EMU)
    th.check_refusals(EMU)


def test_a_wrong_image_index_or_a_split_result_fails_the_checks():
    """The checks can fail: an image taken from the neighbouring image's tables, and a 'half-precision' backend that
    answers with the fp16x2 result (equal to linear_k32's: refused; and outside the bound on the rounded operands)."""
    class WrongImage(hr.H16Emu):
        def gemm(self, s, stats32=None):
            if s.get('ln') and s.get('path') == hr.PATH:
                s = dict(s, ln_shift=s['ln_shift'].roll(1, 0))
            return super().gemm(s, stats32)

    with pytest.raises(AssertionError):
        th.check_ln_image(WrongImage(), _noreport, 3, 144, 64, 'std')

    c = tr.gate_case(144, 64, 'gate')
    split = EMU.gemm(dict(c, path=0, a_form=1))['C'][:c['M'], :64]
    with pytest.raises(AssertionError, match='linear_k32'):
        th.check_vs_split(EMU, _noreport, c, 'gate', split)
    with pytest.raises(AssertionError):   # ... and it is not within the GEMM bound of the rounded operands either
        a16, _ = hr.a_image(c)
        th.tg.close(split, hr.image_refs(c, torch.ldexp(a16.double(), torch.tensor(-tr.EA))), _noreport, 'gate')


def test_margins_over_all_cases(capsys):
    """The worst ratios the module docstring states."""
    worst = {}

    def rep(key, v):
        kind = 'image' if key.endswith('_image_margin') else 'vs' if key.endswith('_vs_fp16x2_margin') else 'gemm_ratio'
        worst[kind] = max(worst.get(kind, 0.0), v)

    for B, T in tr.LN_BT + tr.LN_BT_SMALL:
        for K in tr.LN_K:
            for dist in tr.LN_DISTS:
                th.check_ln_image(EMU, rep, B, T, K, dist)
    for B, T in hr.GN_BT:
        for K in hr.GN_K:
            th.check_gn_image(EMU, rep, B, T, K)
    for T, N in tr.GATE_CASES:
        th.check_gate(EMU, rep, T, N, 'gate')
    for shape in tr.ACT_SHAPES:
        th.check_act_chain(EMU, rep, *shape)
    for shape in hr.WIDE_SHAPES:
        th.check_epilogue(EMU, rep, hr.wide_case(*shape), 'wide')
    with capsys.disabled():
        print('\nh16 emulation, worst over all cases:', {k: round(v, 3) for k, v in worst.items()})
    # (the image bound is tight by construction: round-to-nearest reaches half an ulp; its room is the prologue term)
    assert worst['image'] <= 1.0 and worst['vs'] <= 0.5 and worst['gemm_ratio'] <= 2.0


# ------------------------------------------------------------------------------------- the model-level emulation
def _tiny(kind, golden):
    from utils.synthetic import init_synthetic_
    if kind == 'mdt':
        from models.mdt.model import MDTv2
        g, meta = golden('mdt')
        name, m = 'mdt_c', MDTv2(**meta['archs']['mdt_c']).eval()
    else:
        from models.dit.model import DiT
        g, meta = golden('dit')
        name, m = 'dit_tiny', DiT(**meta['archs']['dit_tiny']).eval()
    init_synthetic_(m)
    x, t, y = (torch.from_numpy(g[f'{name}_{k}']) for k in ('x', 't', 'labels'))
    return m, dict(meta['archs'][name]), x, t, y, torch.from_numpy(g[f'{name}_out_y']).double()


@pytest.mark.parametrize('kind', ['dit', 'mdt'])
def test_host_forward_reproduces_the_fixture_and_the_emulation_covers_the_plans_layers(golden, kind):
    """The host forwards (oracle/dit.py; token_h16_ref.mdt_forward against the REFERENCE's mdt_c fixture) reproduce the
    fp32 golden without the patch; with it exactly the covered GEMMs are rounded, and the result moves by the
    half-precision mode's error: 1e-4 .. 1e-2, far above the 1e-6 of the fp32-accurate arithmetics."""
    m, arch, x, t, y, want = _tiny(kind, golden)
    sd = m.state_dict()
    plain, n0 = hr.host_forward(kind, sd, arch, x, t, y)
    assert n0 == 0 and (plain - want).abs().max().item() <= 1e-5
    emu, n = hr.host_forward(kind, sd, arch, x, t, y, h16=True)
    assert n == hr.covered_gemms(kind, arch)
    emu16 = (emu - want).abs().max().item()
    print(f'{kind}: emu16 {emu16:.3e} (plain float64 host forward {(plain - want).abs().max().item():.3e})')
    assert 1e-4 < emu16 < 1e-1
    import torch.nn.functional as F
    assert F.linear.__module__ == 'torch._C._nn' or F.linear.__name__ == 'linear'   # the patch is gone


def test_set_math_validates_and_is_kept_for_future_handles():
    from models.dit.dit import DiT as LatentDiT
    from models.dit.model import DiT, TokenMath
    from models.mdt.mdt import MDT
    from models.mdt.model import MDTv2
    import dmhip
    assert issubclass(DiT, TokenMath) and issubclass(MDTv2, TokenMath) and issubclass(MDT, LatentDiT)
    m = DiT(input_size=8, patch_size=2, in_channels=4, hidden_size=64, depth=1, num_heads=4, num_classes=10)
    assert m.set_math('fp16') == 'fp16' and m._math == 'fp16' and m._native is None
    with pytest.raises(ValueError):
        m.set_math('bf16x3')
    assert hasattr(LatentDiT, 'set_math')
    assert dmhip.TOKEN_MATH == {'fp32': 0, 'fp16x2': 2, 'fp16': 1} and 'fp16' not in dmhip._lib.CONV_MATH
    assert dmhip.MATH_NAMES == dict(dmhip._lib.CONV_MATH, fp16=1)
