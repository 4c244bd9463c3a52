"""CPU checks of the GroupNorm-chain tests' own inputs, bounds and logic (tests/norm_ref.py,
tests/test_gpu_norm_ops.py), so that the GPU tests cannot hide a failure behind a bad input or an unreachable bound:

* the data families are what they claim (per-image offsets, NaN pad columns, a variance that cancels), the exact
  group moments agree with a two-pass float64 evaluation, the Python restatements of gn_concat_ok and of the first
  conv's geometry decide the listed cases as the launchers do;
* every checking function of the GPU file runs against norm_ref.EmuBackend (the kernels' expressions in fp32 / fp64,
  with and without contracted multiply-adds) and passes with its worst err / bound printed and <= 0.5;
* each mutant of the emulation -- a wrong image index in a finalize table, the last partial chunk dropped, a partial
  one chunk slot late, fp32 accumulation of the sums, no variance clamp, mod_pitch ignored, a pad column in the
  statistics, a concat group summed across the slice boundary wrongly -- fails at least one of those checks.
"""
import pytest
import torch

from tests import norm_ref as nr
from tests import test_gpu_norm_ops as tg

EMU = nr.EmuBackend()
EMU_FMA = nr.EmuBackend(fma=True)
F64 = torch.float64
MARGIN = 0.5


# ------------------------------------------------------------------------------------------ inputs and references
@pytest.mark.parametrize('fam', nr.FAMILIES)
def test_families(fam):
    B, HW, C, G = 3, 100, 32, 8
    x = nr.family(fam, B, HW, C, G, torch.Generator().manual_seed(1))
    assert x.dtype == torch.float32 and torch.isfinite(x).all()
    m = x.double().mean(dim=(1, 2))
    assert (m[1:] - m[:-1]).abs().min() > 9.0, 'the images must be far apart'
    if fam == 'const':
        assert all(len(x[b].unique()) == 1 for b in range(B))
    if fam == 'outlier':
        assert ((x.view(B, HW, G, C // G) > 2e4).sum(dim=(1, 3)) >= 1).all()
    if fam == 'offset':
        assert abs(float(x[0].double().mean()) - 1024.0) < 0.1 and abs(float(x[0].double().std()) - 1.0) < 0.05
    buf = nr.pitched(x, C + 8, 8)
    assert torch.isnan(buf[:, :, :8]).all() and torch.equal(buf[:, :, 8:], x)


def test_modulation_buffer_is_nan_outside_the_tables():
    buf, so, bo = nr.mod_tables(3, 64, torch.Generator().manual_seed(2))
    assert buf.shape[1] > 64 and buf.shape[1] % 4 == 0 and so % 4 == 0 and bo % 4 == 0
    mask = torch.zeros_like(buf, dtype=torch.bool)
    mask[:, so:so + 64] = True
    mask[:, bo:bo + 64] = True
    assert torch.isnan(buf[~mask]).all() and torch.isfinite(buf[mask]).all()
    assert (buf[1, so:so + 64] - buf[0, so:so + 64]).mean() > 0.1
    _, so, bo = nr.mod_tables(3, 64, torch.Generator().manual_seed(2), shift=False)
    assert so is not None and bo is None


def test_exact_moments_agree_with_a_two_pass_float64_evaluation():
    g = torch.Generator().manual_seed(3)
    x = nr.family('neg', 3, 100, 32, 8, g)
    part, _ = nr.partial_ref(x, 8)
    mean, var = nr.group_moments(part, 100 * 4)
    v = x.double().view(3, 100, 8, 4)
    m2 = v.mean(dim=(1, 3))
    v2 = ((v - m2[:, None, :, None]) ** 2).mean(dim=(1, 3))
    assert ((mean - m2).abs() <= 1e-12 * m2.abs()).all()
    # q / n - m^2 from partials rounded at 2^-53: m^2 2^-50 of slack on the variance
    assert ((var - v2).abs() <= 2.0 ** -48 * m2 * m2).all()
    # a sum of squares that came out low: the clamp
    c = nr.fin_case(4096, 32, 32, 'plain', 'clamp')
    _, var = nr.group_moments(c['part'], 4096)
    assert (var == 0).all()
    a, q = c['part'][..., 0].sum(dim=1), c['part'][..., 1].sum(dim=1)
    assert ((q / 4096 - (a / 4096) ** 2) < -nr.EPS).all(), 'the unclamped variance must fall below -eps'


def test_partial_bound_is_twice_the_fp64_summation_error():
    """A sequential fp64 sum in the worst order for it (largest magnitudes first, then alternating signs) stays
    within half the bound; an fp32 sum does not."""
    g = torch.Generator().manual_seed(4)
    x = nr.family('offset', 1, 64, 32, 8, g)
    ref, bound = nr.partial_ref(x, 8)
    v = x.double().view(64, 8, 4).permute(1, 0, 2).reshape(8, 256)
    for gi in range(8):
        s = 0.0
        for t in sorted(v[gi].tolist(), key=abs, reverse=True):
            s += t
        assert abs(s - float(ref[0, 0, gi, 0])) <= 0.5 * float(bound[0, 0, gi, 0])
    s32 = x.view(64, 8, 4).sum(dim=(0, 2)).double()
    assert ((s32 - ref[0, 0, :, 0]).abs() > bound[0, 0, :, 0]).any()


def test_concat_ok_restated():
    """gn_concat_ok's decisions on the cases the GPU test runs and refuses, and against its loop form."""
    for case in nr.CONCAT_CASES:
        assert nr.concat_ok(*case), case
    for case in nr.CONCAT_REFUSED:
        assert not nr.concat_ok(*case), case

    def loop_form(Ch, Gh, Cs, Gs, G):   # csrc/gn.hip gn_concat_ok, line for line
        C = Ch + Cs
        if G <= 0 or Gh <= 0 or Gs <= 0 or C % G or Ch % Gh or Cs % Gs:
            return False
        cpg, cph, cps = C // G, Ch // Gh, Cs // Gs
        for j in range(G):
            lo, hi = j * cpg, (j + 1) * cpg
            if lo < Ch and (lo % cph or min(hi, Ch) % cph):
                return False
            if hi > Ch and ((max(lo, Ch) - Ch) % cps or (hi - Ch) % cps):
                return False
        return True
    for Ch in (64, 96, 128, 256):
        for Cs in (64, 128, 192):
            for Gh in (8, 16, 32, 64):
                for Gs in (8, 24, 32):
                    for G in (0, 8, 32, 48):
                        assert nr.concat_ok(Ch, Gh, Cs, Gs, G) == loop_form(Ch, Gh, Cs, Gs, G), (Ch, Gh, Cs, Gs, G)


def test_first_conv_geometry_covers_every_path():
    cases = nr.small_in_cases()
    assert len(cases) == len(nr.SI_HW) * len(nr.SI_COUT)
    assert {c[0] for c in cases} == {1, 2, 3, 4}
    assert all(nr.small_in_fits(c[0], c[1], c[2], c[3], False) for c in cases)
    rows = {(H, W): nr.small_in_rows(H, W) for H, W in nr.SI_HW}
    assert rows == {(32, 32): 4, (28, 28): 1, (16, 16): 8, (8, 8): 8, (4, 4): 1, (2, 128): 1, (3, 192): 1}
    par = lambda Cout: 256 // min(Cout // 2, 256)  # noqa: E731
    # px_par >= R and px_par < R, threads left over (96, 192, 320: the pairs do not divide 256), a second cp pass
    assert par(128) >= rows[(32, 32)] and par(128) < rows[(16, 16)]
    assert 256 % (96 // 2) and 256 % (192 // 2) and 256 % (320 // 2) and 1024 // 2 > 256
    # statistics: the row segments of (3, 192) at Cout = 128 cross chunk boundaries (4 segments of 48 pixels)
    assert nr.small_in_can_emit(3, 192, 128, 8) and nr.small_in_can_emit(3, 192, 128, 32)
    emit = [(c, G) for c in cases for G in nr.SI_G if nr.small_in_can_emit(c[1], c[2], c[3], G)]
    assert {c[3] for c, _ in emit} == {128, 256, 512, 1024} and {G for _, G in emit} == {8, 16, 32}
    assert not nr.small_in_can_emit(28, 28, 128, 32) and not nr.small_in_can_emit(32, 32, 96, 8)


# ------------------------------------------------------------------------------- the checks on the emulation
@pytest.mark.parametrize('be', [EMU, EMU_FMA], ids=lambda b: b.name)
def test_groupnorm_checks_pass_on_the_emulation(be):
    worst = 0.0
    for shape, fam in tg.GN_FAMILY_CASES:
        worst = max(worst, *tg.check_groupnorm(be, shape, fam))
    for shape, variant in tg.GN_VARIANT_CASES:
        for fam in ('benign', 'offset'):
            worst = max(worst, *tg.check_groupnorm(be, shape, fam, variant))
    print(f'groupnorm: worst err / bound {worst:.3f} ({be.name})')
    assert worst <= MARGIN


@pytest.mark.parametrize('be', [EMU, EMU_FMA], ids=lambda b: b.name)
def test_finalize_checks_pass_on_the_emulation(be):
    worst = 0.0
    for HW, C, G, mode in tg.FIN_CASES:
        for flavour in nr.FIN_FLAVOURS:
            worst = max(worst, tg.check_finalize(be, HW, C, G, mode, flavour))
    worst = max(worst, tg.check_finalize_rechunk(be))
    for shape in tg.AFFINE_SHAPES:
        worst = max(worst, tg.check_affine_equals_hook(be, shape))
    print(f'finalize: worst err / bound {worst:.3f} ({be.name})')
    assert worst <= MARGIN


def test_concat_checks_pass_on_the_emulation():
    worst = max(tg.check_concat(EMU, case, HW) for case in nr.CONCAT_CASES for HW in nr.CONCAT_HW)
    for case in nr.CONCAT_REFUSED:
        tg.check_concat_refused(EMU, case)
    print(f'concat: worst err / bound {worst:.3f}')
    assert worst <= MARGIN


def test_conv_statistics_checks_pass_on_the_emulation():
    worst = max(tg.check_conv_gn(EMU, s, G) for s in nr.CONV_GN_CASES for G in s['G'])
    for s in nr.CONV_GN_REFUSED:
        tg.check_conv_gn_refused(EMU, s, s['G'][0])
    print(f'emitted statistics: worst err / bound {worst:.3f}')
    assert worst <= MARGIN
    worst = max(tg.check_gemm_gn(EMU, s) for s in nr.GEMM_GN_CASES)
    for s in nr.GEMM_GN_REFUSED:
        tg.check_gemm_gn_refused(EMU, s)
    print(f'GEMM statistics: worst err / bound {worst:.3f}')
    assert worst <= MARGIN
    for s in nr.CONV_GIN_CASES:
        for mod in (0, 1):
            for nosilu in (0, 1):
                tg.check_conv_gin(EMU, s, mod, nosilu)
    for s in nr.CONV_GIN_REFUSED:
        tg.check_conv_gin_refused(EMU, s)
    # every group width an emitter admits, a Cout that is no multiple of 128, both layouts
    assert {s['Cout'] // G for s in nr.CONV_GN_CASES for G in s['G']} >= {1, 2, 4, 8, 16, 32}
    assert any(s['Cout'] % 128 for s in nr.CONV_GN_CASES) and {s['layout'] for s in nr.CONV_GN_CASES} == {'slots', 'cover'}
    assert all((nr.conv_case(s)['Ho'] * nr.conv_case(s)['Wo']) % 64 == 0 or s.get('ksplit', 0) > 1 for s in nr.CONV_GN_CASES)


def test_conv_and_resample_checks_pass_on_the_emulation():
    worst = max(tg.check_small_in(EMU, case, G) for case in nr.small_in_cases() for G in [0] + nr.SI_G)
    print(f'first conv statistics: worst err / bound {worst:.3f}')
    assert worst <= MARGIN
    for case in tg.SO_CASES:
        tg.check_small_out_int(EMU, case)
    worst = max(tg.check_small_out_gn(EMU, case) for case in tg.SO_CASES[::2])
    print(f'last conv prologue: worst err / bound {worst:.3f}')
    assert worst <= MARGIN
    tg.check_small_out_refused(EMU)
    worst = max(tg.check_resample(EMU, *case) for case in tg.RS_CASES)
    print(f'resample2x prologue: worst err / bound {worst:.3f}')
    assert worst <= MARGIN
    tg.check_resample_refused(EMU)


# ---------------------------------------------------------------------------------------------------- mutants
S0 = (3, 64, 64, 32)
MUTANT_CHECKS = {
    'image_index': [lambda be: tg.check_groupnorm(be, S0, 'benign'),
                    lambda be: tg.check_finalize(be, 4096, 32, 32, 'plain', 'spread'),
                    lambda be: tg.check_small_out_gn(be, tg.SO_CASES[0])],
    'drop_last_chunk': [lambda be: tg.check_groupnorm(be, (3, 32, 100, 32), 'benign'),
                        lambda be: tg.check_finalize(be, 4097, 32, 32, 'plain', 'spread'),
                        lambda be: tg.check_finalize_rechunk(be)],
    'slot_late': [lambda be: tg.check_groupnorm(be, S0, 'benign'),
                  lambda be: tg.check_conv_gn(be, nr.CONV_GN_CASES[0], 32),
                  lambda be: tg.check_small_in(be, (3, 32, 32, 128), 32),
                  lambda be: tg.check_concat(be, nr.CONCAT_CASES[0], 100)],
    'fp32_sums': [lambda be: tg.check_groupnorm(be, S0, 'offset'),
                  lambda be: tg.check_groupnorm(be, S0, 'benign'),
                  lambda be: tg.check_concat(be, nr.CONCAT_CASES[0], 64)],
    'no_clamp': [lambda be: tg.check_finalize(be, 4096, 32, 32, 'plain', 'clamp'),
                 lambda be: tg.check_finalize(be, 16384, 256, 4, 'mod', 'clamp')],
    'mod_pitch': [lambda be: tg.check_groupnorm(be, S0, 'benign', 'mod'),
                  lambda be: tg.check_finalize(be, 4096, 32, 32, 'mod', 'spread')],
    'pad_in_stats': [lambda be: tg.check_groupnorm(be, S0, 'benign', 'pitched'),
                     lambda be: tg.check_concat(be, nr.CONCAT_CASES[1], 64)],
    'concat_boundary': [lambda be: tg.check_concat(be, nr.CONCAT_CASES[0], 64)],
}


@pytest.mark.parametrize('mutant', nr.MUTANTS)
def test_every_mutant_is_caught(mutant):
    """Every listed check fails on the mutant (and passes on the emulation proper)."""
    bad = nr.EmuBackend(mutant=mutant)
    for i, chk in enumerate(MUTANT_CHECKS[mutant]):
        chk(EMU)
        with pytest.raises(AssertionError):
            chk(bad)
            pytest.fail(f'{mutant}: check {i} did not notice', pytrace=False)


def test_mutant_list_is_complete():
    assert set(MUTANT_CHECKS) == set(nr.MUTANTS)
