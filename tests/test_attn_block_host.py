"""Host checks (no GPU) of tests/attn_block_ref.py, on which tests/test_gpu_attn_block_ops.py stands.

The emulation restates attn_block3_kernel / attn_block4_kernel in fp32: xn = (x sc + sh) 2^6 split to two fp16 pieces;
T = a1 b0 + a0 b1 + a0 b0 against At's row-scaled pieces, + w; T per query scaled to [2^13, 2^14) and split; eight
chunks of 32 keys with m_new = max(m_run, max S sl2), corr = exp2(m_run - m_new), P 2^14 split, l_run = l_run corr +
sum P, O rescaled from the second chunk on; O / (2^14 l) split; the Wg' product; x + (o + cb). The key image, T's
accumulators and Wg' carry the channel permutation pi explicitly.

It must meet the bounds the GPU test holds the kernels to -- 2 e32f + 2^-21 max|ref| against the folded float64
reference on the decoded operands, 2 e32 + 2^-21 max|ref| against the module in float64 -- on every family, so no
family needs a derived bound and the fold's own rounding needs no extra term; and each mutant of it must break the
first bound somewhere, which shows the families can see that mistake. The families' own claims (monotone chunk maxima,
the spread of the dropped bk term, exact zero T, one-hot scores, ...) are asserted from float64.
"""
import os
import re

import pytest
import torch

from tests import attn_block_ref as ab

F32, F64 = torch.float32, torch.float64
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'diffusion-models-pytorch_amd', 'csrc',
                   'attn_block.hip')


def _emu_err(fam, B, mutant=None):
    c = ab.case(fam, 256, B)
    fw = ab.fold_f32(c)
    kr = ab.kernel_refs(c, fw, True)
    e = ab.emulation(c, fw, mutant)
    y = e['y'].double()
    if not torch.isfinite(y).all():
        return float('inf'), kr, e
    return float((y - kr['ref']).abs().max()), kr, e


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('fam', ab.FAMILIES)
def test_emulation_meets_the_bounds(fam, B):
    err, kr, e = _emu_err(fam, B)
    assert err <= kr['bound'], (fam, err, kr['bound'], kr['e32f'])
    assert e['flag'] == 0
    c = ab.case(fam, 256, B)
    mr = ab.module_refs(c)
    assert torch.isfinite(mr['ref']).all() and mr['e32'] < float('inf')
    errm = float((e['y'].double() - mr['ref']).abs().max())
    assert errm <= mr['bound'], (fam, errm, mr['bound'], mr['e32'])


@pytest.mark.parametrize('mutant', ab.MUTANTS)
def test_every_mutant_fails_somewhere(mutant):
    caught = []
    for fam in ab.FAMILIES:
        err, kr, _ = _emu_err(fam, 3, mutant)
        if err > kr['bound']:
            caught.append(fam)
    assert caught, mutant
    # the mistakes only adversarial scores can show must not be visible on the whole-model regime alone
    if mutant in ('no_o_rescale', 'no_l_rescale', 'chunk_max', 'bk_back'):
        assert caught != ['flat']


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('fam', ['ramp8', 'ramp40', 'ramp200', 'desc8', 'desc40', 'desc200'])
def test_ramp_and_desc_move_the_running_maximum(fam, B):
    cm = ab.chunk_maxima(ab.case(fam, 256, B))                 # [B, L, 8]
    d = cm[..., 1:] - cm[..., :-1]
    mono = (d > 0).all(dim=-1) if fam.startswith('ramp') else (d < 0).all(dim=-1)
    assert float(mono.double().mean()) >= 0.9, (fam, float(mono.double().mean()))
    span = (cm.amax(dim=-1) - cm.amin(dim=-1)).median()
    assert float(span) >= 0.7 * float(fam[4:])


@pytest.mark.parametrize('L', [256, 16])
def test_bigbk_drops_a_large_term(L):
    c = ab.case('bigbk', L, 3)
    d = F64
    q = ab.xn_of(c, d) @ c['Wq'].to(d).T + c['bq'].to(d)
    t = c['scale'] * (q @ c['bk'].to(d))                       # s q_i . bk, [B, L]
    if L == 256:
        assert float((t.amax(dim=1) - t.amin(dim=1)).min()) >= 200.0
    assert abs(c['scale'] * float(c['bq'].to(d) @ c['bk'].to(d))) >= 50.0
    assert torch.isfinite(ab.unfolded(c, F32)).all()


def test_gnwide_and_its_twin():
    for L in (256, 16):
        c = ab.case('gnwide', L, 3)
        xs = ab.xn_of(c, F32).abs().amax() * 64.0
        assert 0.8 * ab.FP16_MAX < float(xs) < ab.FP16_MAX
        t = ab.gnwide_twin(c)
        assert float(ab.xn_of(t, F32).abs().amax() * 64.0) > ab.FP16_MAX
        assert int((c['x'] != t['x']).sum()) == 1
        assert float(c['gsc'][2].min() / c['gsc'][0].max()) > 4.0
    c = ab.case('gnwide', 256, 3)
    assert ab.emulation(c, ab.fold_f32(c))['flag'] == 0
    t = ab.gnwide_twin(c)
    assert ab.emulation(t, ab.fold_f32(t))['flag'] == 1


def test_zeroq_is_uniform():
    c = ab.case('zeroq', 256, 3)
    fw = ab.fold_f32(c)
    assert not fw['at'].any() and not fw['w'].any()
    xn = ab.xn_of(c, F64)
    y = c['x'].double() + (xn.mean(dim=1, keepdim=True) @ fw['wg'].double().T + fw['cb'].double())
    assert float((y - ab.kernel_refs(c, fw, False)['ref']).abs().max()) <= 1e-12
    assert float((y - ab.unfolded(c, F64)).abs().max()) <= 1e-6   # (the fold's fp32 rounding of wg, cb)


def test_tiny_scores_are_far_from_one_and_uniform():
    c = ab.case('tiny', 256, 3)
    fw = ab.fold_f32(c)
    t = ab.xn_of(c, F64) @ fw['at'].double().T + fw['w'].double()
    m = t.abs().amax(dim=-1)
    assert 2.0 ** -102 < float(m.min()) and float(m.max()) < 2.0 ** -98
    assert float(m.min()) > 2.0 ** -113                        # the kernel's scale ldexpf(1, 14 - E) stays finite
    kr = ab.kernel_refs(c, fw, True)
    xn = ab.xn_of(c, F64)
    y = c['x'].double() + (xn.mean(dim=1, keepdim=True) @ ab.split_decode(fw['wg']).double().T + fw['cb'].double())
    assert float((y - kr['ref']).abs().max()) <= kr['bound']


@pytest.mark.parametrize('L', [256, 16])
@pytest.mark.parametrize('B', [1, 3])
def test_select_is_exact(L, B):
    c = ab.case('select', L, B)
    s = ab.scores_f64(c)
    want = torch.zeros_like(s).scatter_(2, c['win'][..., None], 256.0)
    assert torch.equal(s, want)
    assert not (c['win'] == torch.arange(L)).any()             # no query selects itself
    g, y = ab.select_answer(c)
    assert torch.equal(g, g.round())
    for b in range(B):
        d = (g[b][:, None, :] - g[b][None, :, :]).abs().amax(dim=-1) + 1e9 * torch.eye(L, dtype=F64)
        assert float(d.min()) >= 1.0                           # pairwise distinct rows, by at least 1 somewhere
    assert float((y - ab.unfolded(c, F64)).abs().max()) <= 1e-12
    fw = ab.fold_f32(c)
    assert torch.equal(fw['at'].double(), c['Wq'].double()) and torch.equal(ab.split_decode(fw['at']), fw['at'])
    assert torch.equal(ab.split_decode(fw['wg']), fw['wg'])
    if B == 3 and L == 256:
        assert not torch.equal(c['x'][0], c['x'][1]) and not torch.equal(c['win'][0], c['win'][1])


@pytest.mark.parametrize('L', [256, 16])
@pytest.mark.parametrize('fam', ab.FAMILIES)
def test_fold_algebra(fam, L):
    """The folded form on the unrounded float64 fold equals the module to float64 accuracy, with the key-constant bk
    terms dropped or added back: they cancel."""
    c = ab.case(fam, L, 3)
    ref = ab.unfolded(c, F64)
    f64 = ab.fold_f64(c)[0]
    tol = 1e-10 * float(ref.abs().max())
    assert float((ab.folded(c, f64, F64) - ref).abs().max()) <= tol
    assert float((ab.folded(c, f64, F64, bk_terms=True) - ref).abs().max()) <= tol


def test_permutations_match_the_kernel_source():
    src = open(SRC).read()
    body = re.search(r'int pi32\(int m\) \{ return ([^;]+); \}', src).group(1)
    assert [eval(body, {'m': m}) for m in range(32)] == [ab.pi32(m) for m in range(32)]   # noqa: S307
    # the key image's comment: storage position 32 g + 8 q + e holds channel 32 g + 4 q + (e & 3) + 16 (e >> 2)
    assert 'storage position 32 g + 8 q + e holds\n// channel 32 g + 4 q + (e & 3) + 16 (e >> 2)' in src
    for g in range(8):
        for q in range(4):
            for e in range(8):
                assert int(ab.PI[32 * g + 8 * q + e]) == 32 * g + 4 * q + (e & 3) + 16 * (e >> 2)
    # the header's accumulator rule: k = 8 q + e <-> row 4 q + (e & 3) + 16 (e >> 2)
    assert 'k = 8q + e  <->  row 4q + (e & 3) + 16 (e >> 2)' in src
    expr = re.search(r'wgp\[id\] = wg\[\(size_t\)d \* C \+ ([^\]]+)\];', src).group(1)
    assert expr == '(k & ~31) + pi32(pi32(k & 31))'
    assert ab.PIPI.tolist() == [(k & ~31) + ab.pi32(ab.pi32(k & 31)) for k in range(256)]
    assert sorted(ab.PI.tolist()) == list(range(256)) and not torch.equal(ab.PIPI, torch.arange(256))
    assert not torch.equal(ab.PIPI, ab.PI)
