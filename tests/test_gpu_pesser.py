"""The pesser DDPM UNet (models/pesser/model.py, variant 3 of the UNet executor), the head-dim-512 instance of the
fused L = 256 attention core and SDEdit on the MI355X path.

tests/golden/pesser.npz holds outputs of the REFERENCE module and of the reference DDPM (make_golden_pesser.py).
Tolerance of a forward: fp32 max-abs <= 1e-4 (conftest.TOL). The fixture weights make every mechanism that differs
from models/unet.py worth >= 50 x that tolerance (tests/test_pesser_host.py).

  pesser_a  C = 256 at 16 x 16: the folded attention block at eps 1e-6 (down path, middle, up path)
  pesser_b  C = 512 at 16 x 16: attn_presplit_kernel<512> / attn_fused_kernel<512,32>; concat widths 1024 and 640
  pesser_c  two bottom/right-padded downsamples, L = 64 attention, level 0 without attention

The fused core runs every contraction in the k order of the split GEMMs it replaces and softmax_rows' softmax, so its
tests are torch.equal against the three-launch path: whole forwards in the four DM_ATTN oracle modes, and the
operator itself on adversarial scores.
"""
import os

import numpy as np
import pytest
import torch

from tests import attention_ref as ar
from tests.conftest import TOL, check_free_running
from tests.test_gpu_attention_ops import PAD, _assert_close_f64, _assert_selected, _attention, _checked_out

pytestmark = pytest.mark.gpu

NAMES = ['pesser_a', 'pesser_b', 'pesser_c']
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, 'diffusion-models-pytorch_amd', 'configs')
FUSED = ('attn_fused_kernel', 'attn_presplit_kernel')
FOLDED = ('attn_block4_kernel', 'attn_block3_kernel')


def _model(meta, name, dev):
    from models.pesser.model import Model
    from utils.synthetic import state_dict_sha256, synthetic_pesser_state_dict
    m = Model(**meta['archs'][name]).eval()
    sd = synthetic_pesser_state_dict(m.state_dict())
    assert state_dict_sha256(sd) == meta[f'{name}_weights_sha256']
    m.load_state_dict(sd)
    return m.to(dev)


def _labels(m, dev):
    import dmhip
    h = m.native_handle(torch.device(dev))
    dmhip.unet_profile_enable(h, 1)
    dmhip.unet_profile_enable(h, 0)
    return [op['label'] for op in dmhip.unet_profile_read(h)]


def _has(labels, prefixes):
    return any(lb.startswith(prefixes) for lb in labels)


@pytest.mark.parametrize('name', NAMES)
def test_forward_vs_reference(cuda, golden, report, name):
    """out and out_small (the input scaled down so that GroupNorm's eps shows) against the reference module's, in
    the default arithmetic."""
    g, meta = golden('pesser')
    model = _model(meta, name, cuda)
    t = torch.from_numpy(g[f'{name}_t']).to(cuda)
    for key in ('', '_small'):
        out = model(torch.from_numpy(g[f'{name}_x{key}']).to(cuda), t).cpu()
        err = (out - torch.from_numpy(g[f'{name}_out{key}'])).abs().max().item()
        print(f'pesser_forward_{name}{key}: {err:.3e}')
        report(f'pesser_forward_{name}{key}', err)
        assert err <= TOL, (name, key, err)


def test_batch_invariance(cuda, golden):
    """Rows of a B = 5 forward of pesser_b are bit-equal to their B = 1 forwards."""
    g, meta = golden('pesser')
    model = _model(meta, 'pesser_b', cuda)
    gen = torch.Generator().manual_seed(11)
    x = torch.randn((5, 3, 32, 32), generator=gen).to(cuda)
    t = torch.tensor([999, 700, 400, 12, 0], device=cuda)
    full = model(x, t).cpu()
    for i in range(5):
        assert torch.equal(model(x[i:i + 1], t[i:i + 1]).cpu()[0], full[i]), i


def test_dispatch(cuda, golden, monkeypatch):
    """The default plans: pesser_b's C = 512 blocks on the fused L = 256 core, pesser_a's C = 256 blocks on the folded
    block; under DM_ATTN=unfused neither has a fused attention label."""
    g, meta = golden('pesser')
    x = torch.from_numpy(g['pesser_a_x']).to(cuda)
    t = torch.from_numpy(g['pesser_a_t']).to(cuda)
    for name, want in (('pesser_b', FUSED), ('pesser_a', FOLDED)):
        model = _model(meta, name, cuda)
        model(x, t)
        labels = _labels(model, cuda)
        assert _has(labels, want), (name, labels)
        if name == 'pesser_b':
            assert any(lb in ('attn_presplit_kernel<512>', 'attn_fused_kernel<512>') for lb in labels), labels
            assert not _has(labels, FOLDED), labels
    monkeypatch.setenv('DM_ATTN', 'unfused')
    for name in ('pesser_b', 'pesser_a'):
        model = _model(meta, name, cuda)
        model(x, t)
        labels = _labels(model, cuda)
        assert not _has(labels, FUSED + FOLDED + ('attn_flash_kernel', 'attn_small_kernel')), (name, labels)
        assert 'softmax_rows' in labels


def _unet_512(dev):
    from models.unet import UNet
    from utils.synthetic import init_synthetic_
    m = UNet(dim=128, dim_mults=[1, 4], use_attn=[False, True], num_res_blocks=1).eval()
    init_synthetic_(m)
    return m.to(dev)


@pytest.mark.parametrize('arch', ['pesser_b', 'unet_512'])
def test_fused_attention_512_bit_identical(cuda, golden, arch, monkeypatch):
    """One head of 512 channels on a 16 x 16 map, B = 8 forwards in the four DM_ATTN oracle modes: the fused kernel
    label appears exactly in the modes that select it (never with the output projection fused: that form is built for
    head dim 256 only), and the outputs equal the three-launch path's bit for bit. pesser_b, and models.unet.UNet
    with a 512-channel stage at 16 x 16 (the shape configs/ddpm_celebahq.yaml has)."""
    g, meta = golden('pesser')
    kernel = {'unfused': None, 'fused': 'attn_fused_kernel', 'presplit': 'attn_presplit_kernel',
              'noproj': 'attn_presplit_kernel'}
    gen = torch.Generator().manual_seed(4)
    x = torch.randn((8, 3, 32, 32), generator=gen).to(cuda)
    t = torch.tensor([999, 800, 600, 400, 200, 100, 10, 0], device=cuda)
    outs = {}
    for mode in ('unfused', 'fused', 'noproj', 'presplit'):
        monkeypatch.setenv('DM_ATTN', mode)
        m = _model(meta, 'pesser_b', cuda) if arch == 'pesser_b' else _unet_512(cuda)
        outs[mode] = m(x, t).cpu()
        labels = _labels(m, cuda)
        for name in FUSED:
            assert _has(labels, (name, )) == (kernel[mode] == name), (mode, labels)
            assert all(lb == f'{name}<512>' for lb in labels if lb.startswith(name)), (mode, labels)
        assert ('softmax_rows' in labels) == (mode == 'unfused'), (mode, labels)
    assert torch.isfinite(outs['unfused']).all()
    for mode in ('fused', 'noproj', 'presplit'):
        assert torch.equal(outs[mode], outs['unfused']), mode


# ---------------------------------------------------------------------------------------------------- operator level
SHAPE512 = (2, 1, 256, 512)
ALPHA512 = 512 ** -0.5   # not a power of two: q * alpha rounds, identically in all three paths


def _near_fp16(shape):
    """flat scores with a few operand elements at +-1000 (x 2^6 = 64000, just inside fp16's 65504) in q, k and v."""
    q, k, v, _ = ar.generate(shape, 'flat')
    q, k, v = q.clone(), k.clone(), v.clone()
    gen = torch.Generator().manual_seed(23)
    for x in (q, k, v):
        idx = torch.randint(0, x.numel(), (64, ), generator=gen)
        x.view(-1)[idx] = 1000.0 * (torch.randint(0, 2, (64, ), generator=gen) * 2 - 1).float()
    return q, k, v, None


def _equal_rows(shape):
    """Every key the same vector: each query's 256 scores are equal, P is exactly 1 / 256, the output the mean of v."""
    q, k, v, _ = ar.generate(shape, 'peaked')
    return q, k[:, :, :1].expand_as(k).contiguous(), v, None


def _case512(dist):
    """(fp32 q | k | v rows [B L][3 C] the unfused and fused operators read, the planes of the same operands, the
    float64 reference of the decoded operands with the bound of tests/attention_ref.py, pi for 'select')."""
    B, H, L, Dh = SHAPE512
    if dist == 'near_fp16':
        q, k, v, pi = _near_fp16(SHAPE512)
    elif dist == 'equal':
        q, k, v, pi = _equal_rows(SHAPE512)
    else:
        q, k, v, pi = ar.generate(SHAPE512, dist)
    q_rows = (q / ALPHA512).float()             # what the qkv projection would hold: the kernels apply alpha
    q_eff = q_rows * torch.tensor(ALPHA512)     # fp32 product, as `v * a.alpha` on the device
    pq, pk, pv, (qd, kd, vd) = ar.pack_planes(q_eff, k, v)
    ref = ar.attention_f64(qd, kd, vd)
    e32 = (ar.attention_f32(qd, kd, vd).double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    rows = torch.cat([x.permute(0, 2, 1, 3).reshape(B * L, H * Dh) for x in (q_rows, k, v)], dim=1).contiguous()
    return dict(rows=rows, pq=pq, pk=pk, pv=pv, v=v, pi=pi, ref=ref, e32=e32, scale=scale,
                bound=2.0 * e32 + 2.0 ** -21 * scale)


def _unfused(dev, rows):
    """The three launches the fused core replaces, as the plans issue them (unet_exec.hip): the split S GEMM
    (alpha on q, exponents 6 / 6), softmax_rows, the split PV GEMM (exponents 14 / 6, v read [k][n])."""
    import dmhip
    B, H, L, Dh = SHAPE512
    C = H * Dh
    qkv = rows.to(dev)
    S = torch.empty((B, H, L, L), device=dev)
    O = torch.full((B, L, C + PAD), float('nan'), device=dev)
    flag = torch.zeros((1, ), dtype=torch.int32, device=dev)
    d = dmhip.GemmDesc()
    d.M, d.N, d.K, d.Z1, d.Z2 = L, L, Dh, B, H
    d.A, d.a_s1, d.a_s2, d.lda = qkv.data_ptr(), L * 3 * C, Dh, 3 * C
    d.B, d.b_s1, d.b_s2, d.ldb, d.b_kn = qkv.data_ptr() + 4 * C, L * 3 * C, Dh, 3 * C, 0
    d.C, d.c_s1, d.c_s2, d.ldc = S.data_ptr(), H * L * L, L * L, L
    d.alpha, d.b_scale = ALPHA512, 0.0
    d.split, d.split_ea, d.split_eb, d.range_flag = 2, ar.EA, ar.EB, flag.data_ptr()
    dmhip.gemm(d, dev)
    dmhip.softmax_rows(S, B * H * L, L, L)
    d = dmhip.GemmDesc()
    d.M, d.N, d.K, d.Z1, d.Z2 = L, Dh, L, B, H
    d.A, d.a_s1, d.a_s2, d.lda = S.data_ptr(), H * L * L, L * L, L
    d.B, d.b_s1, d.b_s2, d.ldb, d.b_kn = qkv.data_ptr() + 8 * C, L * 3 * C, Dh, 3 * C, 1
    d.C, d.c_s1, d.c_s2, d.ldc = O.data_ptr(), L * (C + PAD), Dh, C + PAD
    d.alpha, d.b_scale = 1.0, 0.0
    d.split, d.split_ea, d.split_eb, d.range_flag = 2, ar.EP, ar.EV, flag.data_ptr()
    dmhip.gemm(d, dev)
    torch.cuda.synchronize()
    return O.cpu(), int(flag.item())


@pytest.mark.parametrize('dist', ['select', 'equal', 'near_fp16', 'flat', 'ramp40'])
def test_attention_512_operator(cuda, report, dist):
    """dm_debug_attention at L = 256, Dh = 512 -- attn_presplit_kernel<512> on the operand planes and
    attn_fused_kernel<512, 32> on fp32 q | k | v rows -- on one dominant key per row (select), all-equal rows, operands
    next to the fp16 range, flat and ramped scores: both equal the unfused operator (split S GEMM, softmax_rows, split
    PV GEMM) bit for bit, leave the pad columns alone and raise no range flag, and are within the attention operator
    tests' bound (2 e32 + 2^-21 max|ref|) of float64 on the decoded operands."""
    c = _case512(dist)
    want, flag_u = _unfused(cuda, c['rows'])
    o_f, flag_f = _attention(cuda, SHAPE512, qkv=c['rows'], alpha=ALPHA512, b_scale=1.0)
    o_p, flag_p = _attention(cuda, SHAPE512, c['pq'], c['pk'], c['pv'])
    assert (flag_u, flag_f, flag_p) == (0, 0, 0)
    C = SHAPE512[1] * SHAPE512[3]
    assert torch.isnan(want[..., C:]).all()
    for kernel, o in (('fused', o_f), ('presplit', o_p)):
        got = _checked_out(o, SHAPE512)
        assert torch.equal(o[..., :C], want[..., :C]), (kernel, dist, (o[..., :C] - want[..., :C]).abs().max().item())
        key = f'attn_{kernel}_2x1x256x512_{dist}'
        if dist == 'select':
            _assert_selected(got, c, key)
        else:
            _assert_close_f64(got, c, report, key)
        if dist == 'equal':
            mean = c['v'].double().mean(dim=2, keepdim=True).expand_as(got)
            assert (got - mean).abs().max().item() <= c['bound']


# ------------------------------------------------------------------------------------------------------------ SDEdit
def test_sdedit_fold_vs_reference(cuda, golden, report):
    """sdedit_fold on pesser_c with the fixture's noises (the diffuse draw first, then one per step) against the
    reference DDPM's float32 and float64 trajectories, step by step."""
    from diffusions.ddpm import DDPM
    from scripts.sample_sdedit import sdedit_fold
    g, meta = golden('pesser')
    p = meta['sdedit']
    model = _model(meta, 'pesser_c', cuda)
    d = DDPM(var_type=p['var_type'], respace_type=p['respace_type'], respace_steps=p['respace_steps'], device=cuda)
    draws = [g['sdedit_diffuse_noise']] + list(g['sdedit_step_noise'])
    steps = []
    it = iter(draws)
    d.noise_fn = lambda x: torch.from_numpy(next(it)).to(x.device)
    denoise = d.denoise

    def recording(*a, **k):
        out = denoise(*a, **k)
        steps.append(out['sample'].cpu().numpy())
        return out
    d.denoise = recording
    x0 = torch.from_numpy(g['sdedit_x0']).to(cuda)
    noised, edited = sdedit_fold(d, model, x0, p['edit_steps'], dict(disable=True))
    assert next(it, None) is None and len(steps) == p['edit_steps']
    assert np.abs(noised.cpu().numpy() - g['sdedit_noised']).max() <= 1e-6
    worst = 0.0
    for i, s in enumerate(steps):
        e32, e64 = check_free_running(s, g[f'sdedit_step{i}_sample'], g[f'sdedit_step{i}_sample64'],
                                      g['sdedit_drift_sample'], i)
        worst = max(worst, e32)
    report('pesser_sdedit_worst_e32', worst)
    assert np.abs(edited.cpu().numpy() - g['sdedit_edited']).max() <= max(TOL, 2.5 * g['sdedit_drift_sample'].max())
    assert edited.min() >= -1 and edited.max() <= 1


def _write_inputs(folder, n, size):
    from PIL import Image
    os.makedirs(folder)
    rng = np.random.default_rng(9)
    imgs = []
    for i in range(n):
        a = rng.integers(0, 256, (size, size, 3), dtype=np.uint8)
        Image.fromarray(a).save(os.path.join(folder, f'{i:02d}.png'))
        imgs.append(a)
    return imgs


def test_sample_sdedit_script(cuda, golden, tmp_path):
    """scripts/sample_sdedit.py on three 32 x 32 PNGs with weights saved from the synthetic recipe (pesser_c through
    dotlist overrides of the LSUN config): three PNGs of [input | noised | edited] tiles (3 x 32 + 4 x 2 = 104 by
    36 pixels), the left tile the input within one grey level, the same bytes from a second run with the same seed,
    and --edit_steps 0 refused with the ValueError."""
    from scripts import sample_sdedit
    from utils.png import read_png_rgb
    g, meta = golden('pesser')
    arch = meta['archs']['pesser_c']
    wpath = str(tmp_path / 'pesser_c.pt')
    torch.save(_model(meta, 'pesser_c', 'cpu').state_dict(), wpath)
    src = str(tmp_path / 'in')
    imgs = _write_inputs(src, 3, 32)
    over = ['--model.params.ch', str(arch['ch']), '--model.params.ch_mult', str(list(arch['ch_mult'])),
            '--model.params.attn_resolutions', str(list(arch['attn_resolutions'])), '--model.params.resolution', '32',
            '--data.params.img_size', '32']
    common = ['-c', os.path.join(CONFIGS, 'pesser_lsun_church_256.yaml'), '--weights', wpath, '--input_dir', src,
              '--respace_steps', '10', '--batch_size', '2']
    runs = []
    for tag in ('a', 'b'):
        out = tmp_path / tag
        sample_sdedit.main(common + ['--edit_steps', '4', '--save_dir', str(out)] + over)
        assert sorted(os.listdir(out)) == ['0.png', '1.png', '2.png']
        runs.append([open(out / f'{i}.png', 'rb').read() for i in range(3)])
    assert runs[0] == runs[1]
    for i in range(3):
        img = read_png_rgb(str(tmp_path / 'a' / f'{i}.png'))
        assert img.shape == (36, 104, 3)
        left = img[2:34, 2:34].astype(np.int16)
        assert np.abs(left - imgs[i].astype(np.int16)).max() <= 1
        tiles = [img[2:34, 2 + 34 * k:34 + 34 * k] for k in range(3)]
        assert not np.array_equal(tiles[1], tiles[0]) and not np.array_equal(tiles[2], tiles[1])
    with pytest.raises(ValueError, match='edit_steps'):
        sample_sdedit.main(common + ['--edit_steps', '0', '--save_dir', str(tmp_path / 'c')] + over)
