"""The half-precision arithmetic DM_MATH_FP16 ('fp16') of DiT and MDTv2 at the model level, on dit_tiny and mdt_c
(tests/golden/dit.json, mdt.json; B <= 3): the setter contract, plan routing, accuracy against a host emulation of the
same roundings, batch invariance, the range fallback (tests/test_gpu_exec_abi.py's hot label) and the Python surface
(set_math, DDIMCFG, scripts/sample_cfg.py --math).

The mode has no fp32 parity to assert. What is asserted instead: the engine's error against the fp32 golden (err16) is
at most twice the error of a HOST forward that makes the same roundings at the same points (emu16: oracle/dit.py, or
token_h16_ref.mdt_forward for MDT, in float64 with torch.nn.functional.linear replaced from here on the covered
layers) -- engine and emulation are two realisations of the same rounding noise over a few thousand outputs, differing
in accumulation order and rare rounding flips -- and err16 exceeds the fp16x2 error, so the mode is the cheaper one.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import dmhip
from dmhip._lib import DM_ERR_ARG, DM_OK, load, stream_handle
from tests import test_gpu_exec_abi as ea
from tests import token_h16_ref as hr

pytestmark = pytest.mark.gpu

KINDS = ['dit', 'mdt']
ABI = {'dit': 'dm_dit', 'mdt': 'dm_mdt'}
CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'diffusion-models-pytorch_amd',
                       'configs')


def _model(kind, cuda, golden):
    """-> (model on the device, arch, golden arrays, fixture name)"""
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
    return m.to(cuda), dict(meta['archs'][name]), g, name


def _inputs(g, name, cuda):
    return tuple(torch.from_numpy(g[f'{name}_{k}']).to(cuda) for k in ('x', 't', 'labels'))


def _labels(h, abi):
    return [op['label'] for op in dmhip.unet_profile_read(h, abi)]


@pytest.mark.parametrize('kind', KINDS)
def test_setter_contract(cuda, golden, kind):
    abi = ABI[kind]
    model, arch, g, name = _model(kind, cuda, golden)
    h = model.native_handle(torch.device(cuda))
    x, t, y = _inputs(g, name, cuda)
    assert dmhip.dit_math(h, abi=abi) == 'fp16x2'
    model(x, t, y)
    assert dmhip.plan_stats(h, abi) == (1, 1)
    assert dmhip.dit_math(h, 'fp16', abi=abi) == 'fp16'          # DM_ERR_ARG without the mode
    assert dmhip.plan_stats(h, abi) == (1, 0)                    # the switch drops the cached plans
    assert dmhip.range_stats(h, abi) == (0, 'fp16')
    out = model(x, t, y)
    assert torch.isfinite(out).all()
    assert dmhip.plan_stats(h, abi) == (2, 1)                    # ... and the next forward builds one
    assert dmhip.dit_math(h, 'fp16', abi=abi) == 'fp16' and dmhip.plan_stats(h, abi) == (2, 1)
    k = ctypes.c_int()
    assert getattr(load(), abi + '_get_math')(h, ctypes.byref(k)) == DM_OK and k.value == dmhip.MATH_FP16 == 1
    for bad in (3, 7, -1):
        assert getattr(load(), abi + '_set_math')(h, bad) == DM_ERR_ARG
    assert dmhip.dit_math(h, abi=abi) == 'fp16'
    with pytest.raises(ValueError):
        dmhip.dit_math(h, 'bf16x3', abi=abi)


def test_conv_nets_reject_the_mode(cuda, golden):
    L = load()
    c = ea._unet(cuda, golden)
    assert L.dm_unet_set_conv_math(c.handle(), 1) == DM_ERR_ARG
    assert 'DM_MATH_FP16 is for the token models' in L.dm_last_error().decode()   # the error names the kind
    assert dmhip.unet_conv_math(c.handle()) == 'fp16x2'
    with pytest.raises(ValueError):
        dmhip.unet_conv_math(c.handle(), 'fp16')
    for enc in (False, True):
        v = ea._vae(cuda, enc)
        assert getattr(L, v.abi + '_set_math')(v.handle(), 1) == DM_ERR_ARG
        assert dmhip.vae_math(v.handle(), abi=v.abi) == 'fp16x2'


@pytest.mark.parametrize('kind', KINDS)
def test_routing_accuracy_and_batch_invariance(cuda, golden, report, kind):
    abi = ABI[kind]
    model, arch, g, name = _model(kind, cuda, golden)
    h = model.native_handle(torch.device(cuda))
    x, t, y = _inputs(g, name, cuda)
    want = torch.from_numpy(g[f'{name}_out_y']).double()
    out_x2 = model(x, t, y).cpu().double()
    assert model.set_math('fp16') == 'fp16' and dmhip.dit_math(h, abi=abi) == 'fp16'
    out16 = model(x, t, y).cpu().double()

    # --- routing: every covered GEMM on the new kernel, behind its image pass or a producer; linear_k32 keeps the
    # adaLN GEMM only
    labels = _labels(h, abi)
    n_cov = hr.covered_gemms(kind, arch)
    blocks = (n_cov - 1) // 4 if kind == 'dit' else 2 * ((arch['depth'] - arch['decode_layer']) // 2) + arch['decode_layer']
    skips = n_cov - 1 - 4 * blocks
    assert labels.count('linear_h16_kernel') == n_cov, labels
    assert labels.count('linear_h16_image') == 3 * blocks + 1, labels      # qkv, proj, fc1 (fc2: fc1's c_split), final
    assert labels.count('linear_h16_image_cat') == skips, labels
    assert len([s for s in labels if s.startswith('linear_k32')]) == 1, labels
    assert not [s for s in labels if s.startswith('linear_presplit') or s == 'row_stats_split'], labels

    # --- accuracy against the emulation of the same roundings
    emu, n = hr.host_forward(kind, model.state_dict(), arch, x, t, y, h16=True)
    assert n == n_cov
    err16 = (out16 - want).abs().max().item()
    emu16 = (emu - want).abs().max().item()
    direct = (out16 - emu).abs().max().item()
    err_x2 = (out_x2 - want).abs().max().item()
    print(f'{name} fp16: err16 {err16:.3e} emu16 {emu16:.3e} engine-to-emulation {direct:.3e} fp16x2 {err_x2:.3e}')
    report(f'{name}_fp16_err16_maxabs_vs_golden', err16)
    report(f'{name}_fp16_emu16_maxabs_vs_golden', emu16)
    report(f'{name}_fp16_engine_to_emulation_maxabs', direct)
    report(f'{name}_fp16x2_maxabs_vs_golden', err_x2)
    assert err16 <= 2.0 * emu16, (err16, emu16)
    assert err16 > err_x2, (err16, err_x2)

    # --- batch invariance: row 0 of a B = 3 forward is the B = 1 forward, bit for bit (no split-K tail)
    gen = torch.Generator().manual_seed(12)
    x3 = torch.randn((3, *x.shape[1:]), generator=gen).to(cuda)
    t3 = torch.tensor([500, 20, 777], device=cuda)
    y3 = torch.tensor([1, 2, 5], device=cuda)
    o3 = model(x3, t3, y3).cpu()
    o1 = model(x3[:1], t3[:1], y3[:1]).cpu()
    assert torch.equal(o3[:1], o1)
    assert not torch.equal(o3[1:2], o1)


@pytest.mark.parametrize('kind', KINDS)
def test_range_fallback(cuda, golden, kind):
    """tests/test_gpu_exec_abi.py's sequence with 'fp16' as the caller's arithmetic: label 3's table row (x 1e5) sends
    the adaLN GEMM's operand beyond fp16."""
    abi = ABI[kind]
    L = load()
    c = ea._token_model(cuda, golden, kind == 'mdt')
    h = c.handle()
    fn = lambda name: getattr(L, abi + name)   # noqa: E731

    def run(inp):
        out = c.run(inp)
        torch.cuda.synchronize()
        return out.cpu()

    stats = lambda: dmhip.range_stats(h, abi)   # noqa: E731
    assert dmhip.dit_math(h, 'fp32', abi=abi) == 'fp32'
    want = run(c.hot)
    assert torch.isfinite(want).all() and stats() == (0, 'fp32')
    assert dmhip.dit_math(h, 'fp16', abi=abi) == 'fp16'
    first = run(c.cold)
    assert torch.isfinite(first).all() and stats() == (0, 'fp16')
    got = run(c.hot)
    assert torch.equal(got, want)                    # the flagged forward is the fp32 arithmetic's own
    assert stats() == (1, 'fp16') and dmhip.dit_math(h, abi=abi) == 'fp16'   # counted once, not sticky
    assert torch.equal(run(c.cold), first)
    assert stats() == (1, 'fp16')

    # deferred mode: no second pass; the poll reports the flag and switches to the fallback until told otherwise
    flagged = ctypes.c_int(-1)
    st = stream_handle(cuda)
    assert fn('_set_range_deferred')(h, 1) == DM_OK
    assert fn('_range_poll')(h, st, ctypes.byref(flagged)) == DM_OK and flagged.value == 0
    raw = run(c.hot)
    assert stats() == (1, 'fp16')
    assert not torch.equal(raw, want)
    assert fn('_range_poll')(h, st, ctypes.byref(flagged)) == DM_OK and flagged.value == 1
    assert stats() == (2, 'fp32') and dmhip.dit_math(h, abi=abi) == 'fp16'
    assert torch.equal(run(c.hot), want)
    assert fn('_range_poll')(h, st, ctypes.byref(flagged)) == DM_OK and flagged.value == 0
    assert fn('_range_fallback')(h, 0) == DM_OK
    assert stats() == (2, 'fp16')
    assert fn('_set_range_deferred')(h, 0) == DM_OK
    assert torch.equal(run(c.cold), first)
    assert stats() == (2, 'fp16')


def test_set_math_reaches_future_handles_and_the_sampler_runs(cuda, golden, report):
    """model.set_math before the handle exists, three DDIMCFG steps on dit_tiny: finite, and not the fp16x2
    trajectory. The distance is reported, not asserted (free-running trajectories are chaotic)."""
    from diffusions import DDIMCFG
    from models.dit.model import DiT
    from utils.synthetic import init_synthetic_
    g, meta = golden('dit')
    cfg = meta['cfg5']
    labels = torch.from_numpy(g['cfg5_labels']).to(cuda)
    init = torch.from_numpy(g['cfg5_init']).to(cuda)
    last = {}
    for math in ('fp16x2', 'fp16'):
        model = DiT(**meta['archs']['dit_tiny']).eval()
        init_synthetic_(model)
        assert model.set_math(math) == math          # no handle yet
        model = model.to(cuda)
        # ('uniform' keeps arange(0, 1000, 333): four steps; linspace gives exactly three)
        d = DDIMCFG(guidance_scale=cfg['guidance_scale'], respace_type='uniform-linspace', respace_steps=3,
                    eta=cfg['eta'], device=cuda)
        steps = list(d.sample_loop(model, init, model_kwargs=dict(y=labels)))
        assert len(steps) == 3
        last[math] = steps[-1]['sample'].cpu()
        assert dmhip.dit_math(model.native_handle(torch.device(cuda))) == math
        assert dmhip.range_stats(model.native_handle(torch.device(cuda)), 'dm_dit') == (0, math)
    assert torch.isfinite(last['fp16']).all()
    assert not torch.equal(last['fp16'], last['fp16x2'])
    dist = (last['fp16'] - last['fp16x2']).abs().max().item()
    print(f'dit_tiny DDIMCFG-3: fp16 to fp16x2 {dist:.3e}')
    report('dit_tiny_ddimcfg3_fp16_to_fp16x2_maxabs', dist)


def test_latent_wrapper_forwards_set_math(cuda):
    from models.dit.dit import DiT as LatentDiT
    from utils.synthetic import init_synthetic_
    arch = dict(input_size=8, patch_size=2, hidden_size=64, depth=2, num_heads=4, num_classes=10)
    model = LatentDiT(vae_config=dict(target='models.dit.autoencoder.AutoEncoderKL', params=dict(from_pretrained='none')),
                      vit_config=dict(target='models.dit.model.DiT', params=arch))
    init_synthetic_(model.vit)
    model = model.to(cuda).eval()
    gen = torch.Generator().manual_seed(2)
    x = torch.randn((2, 4, 8, 8), generator=gen).to(cuda)
    t, y = torch.tensor([500, 20], device=cuda), torch.tensor([1, 2], device=cuda)
    a = model(x, t, y).cpu()
    assert model.set_math('fp16') == 'fp16'
    assert dmhip.dit_math(model.vit.native_handle(torch.device(cuda))) == 'fp16'
    b = model(x, t, y).cpu()
    assert torch.isfinite(b).all() and not torch.equal(a, b) and (a - b).abs().max().item() < 0.1
    assert model.vae is None                          # the VAE is not touched


def test_sample_cfg_math_option(cuda, tmp_path):
    """scripts/sample_cfg.py --math fp16 on the reduced DiT config writes its latents; they differ from the default
    arithmetic's; a model without a token path refuses the option."""
    from scripts import sample_cfg
    from tests.test_gpu_scripts import TINY_ADAGN, TINY_DIT
    cfg = os.path.join(CONFIGS, 'dit_xl2_256.yaml')
    common = ['-c', cfg, '--weights', 'synthetic', '--guidance_scale', '4', '--class_ids', '7', '--n_samples_each_class',
              '2', '--batch_size', '2', '--sampler', 'ddim', '--respace_steps', '3'] + TINY_DIT
    sample_cfg.main(common + ['--save_dir', str(tmp_path / 'h'), '--math', 'fp16'])
    sample_cfg.main(common + ['--save_dir', str(tmp_path / 'x')])
    assert sorted(os.listdir(tmp_path / 'h' / 'class7')) == ['0.npy', '1.npy']
    h = np.stack([np.load(tmp_path / 'h' / 'class7' / f'{i}.npy') for i in range(2)])
    x = np.stack([np.load(tmp_path / 'x' / 'class7' / f'{i}.npy') for i in range(2)])
    assert h.shape == (2, 4, 8, 8) and np.isfinite(h).all()
    assert not np.array_equal(h, x) and np.abs(h - x).max() < 0.5
    with pytest.raises(SystemExit, match='no token path'):
        sample_cfg.main(['-c', os.path.join(CONFIGS, 'ddpm_cfg_cifar10.yaml'), '--weights', 'synthetic',
                         '--guidance_scale', '3', '--class_ids', '1', '--n_samples_each_class', '1', '--batch_size', '1',
                         '--save_dir', str(tmp_path / 'u'), '--sampler', 'ddim', '--respace_steps', '2', '--math', 'fp16']
                        + TINY_ADAGN)
