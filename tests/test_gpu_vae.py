"""The native VAE latent decoder (dm_vae_decoder, csrc/vae_exec.hip) on the GPU against tests/vae_ref.py, which
tests/golden/vae.npz pins to the reference module (tests/test_vae_host.py).

Configurations (tests/vae_ref.py CONFIGS): T1 narrow maps with a nin_shortcut at every level (2 x 4 x 8 x 8 -> 32^2,
attention L = 64, Dh = 128); T2 wide maps (1 x 4 x 32 x 32 -> 128^2, attention at the production L = 1024); T3 the
real architecture at a cropped size (ch 128, (1, 2, 4, 4), 1 x 4 x 8 x 8 -> 64^2, Dh = 512).

Bound: the project's parity criterion, max-abs error <= 1e-4 max(1, max|ref|) against the float32 reference. Where
the reference's own float32-vs-float64 error exceeds half of that, |out - ref64| <= 2 e32 + 2^-21 max|ref64| instead
(tests/test_gpu_token_ops.py's rule); measured on the CPU the ratio e32 / bound is 0.008 (T1), 0.010 (T2), 0.010 (T3)
and 0.007 for the range-fallback weights, so the first form applies to every case here. References are computed
once per case and shared.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import vae_ref
from utils.png import read_png_rgb

pytestmark = pytest.mark.gpu

SCALE_FACTOR = 0.18215  # not a power of two; applied as the reference does: 1. / scale_factor * z
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, 'diffusion-models-pytorch_amd', 'configs')


def _scale32() -> float:
    return float(torch.tensor(1. / SCALE_FACTOR, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def _weights(name, variant=''):
    sd = vae_ref.weights(name)
    if variant == 'range':
        # mid.block_2's output conv scaled 10^6-fold: the block's output (~5e5) feeds the level's raw-input consumers
        # (the upsample conv) beyond the fp16 range; every GroupNorm downstream renormalises it, so the float32
        # reference stays finite and O(1) at the output (checked on the CPU: finite, e32 1.3e-6, max|out| 1.84)
        for k in ('decoder.mid.block_2.conv2.weight', 'decoder.mid.block_2.conv2.bias'):
            sd[k] = sd[k] * 1e6
    return sd


@functools.lru_cache(maxsize=None)
def _case(name, shape=None, variant='', seed=7):
    """(z, ref32, ref64-derived figures) of a case, computed once."""
    sd = _weights(name, variant)
    shape = shape or vae_ref.CONFIGS[name]['z_shape']
    z = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    with torch.no_grad():
        r32 = vae_ref.decode(sd, z, SCALE_FACTOR)
        r64 = vae_ref.decode(sd, z, SCALE_FACTOR, torch.float64)
    assert torch.isfinite(r32).all()
    return z, r32, r64


@functools.lru_cache(maxsize=None)
def _model(name, variant='', decode_batch=8):
    from models.dit.autoencoder import AutoEncoderKL
    return AutoEncoderKL.from_state_dict(vae_ref.diffusers_config(name), _weights(name, variant),
                                         decode_batch=decode_batch)


def _check(key, got, r32, r64, report=None):
    got = got.detach().cpu()
    assert got.shape == r32.shape, (key, got.shape, r32.shape)
    assert torch.isfinite(got).all(), key
    m = r64.abs().max().item()
    e32 = (r32.double() - r64).abs().max().item()
    base = 1e-4 * max(1.0, m)
    if e32 <= base / 2:
        err, bound = (got - r32).abs().max().item(), 1e-4 * max(1.0, r32.abs().max().item())
    else:
        err, bound = (got.double() - r64).abs().max().item(), 2 * e32 + 2.0 ** -21 * m
    print(f'{key}: err {err:.3e} bound {bound:.3e} err/bound {err / bound:.4f} (e32 {e32:.3e}, max|ref| {m:.3f})')
    if report is not None:
        report(f'vae_{key}_err_over_bound', err / bound)
    assert err <= bound, (key, err, bound)


def _decode(m, z, cuda):
    out = m.decode(z.to(cuda), scale=_scale32()).sample
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('name', ['T1', 'T2', 'T3'])
def test_decode_matches_reference(cuda, report, name):
    z, r32, r64 = _case(name)
    m = _model(name)
    _check(name, _decode(m, z, cuda), r32, r64, report)
    w, s = m.memory(cuda)
    print(f'{name}: weights {w / 2 ** 20:.1f} MiB, workspace {s / 2 ** 20:.1f} MiB')
    assert w > 0 and s > 0


@pytest.mark.parametrize('shape', [(1, 4, 8, 16), (1, 4, 16, 8), (1, 4, 6, 6)])
def test_non_square_and_odd_latents(cuda, report, shape):
    """Rows, columns and the upsample parities must not be mixed up; 6 x 6 -> 24^2 is no multiple of any tile."""
    z, r32, r64 = _case('T1', shape, seed=11)
    _check('T1_%dx%d' % shape[2:], _decode(_model('T1'), z, cuda), r32, r64, report)


def test_batch_invariance_and_micro_batches(cuda):
    """Image i of a B = 3 decode is bit-identical to its own B = 1 decode (fixed tile heuristics), and to the
    micro-batched decode (decode_batch = 2: a batch of 2 and a batch of 1)."""
    z = torch.randn((3, 4, 8, 8), generator=torch.Generator().manual_seed(5)).to(cuda)
    m = _model('T1')
    whole = _decode(m, z, cuda)
    for i in range(3):
        assert torch.equal(_decode(m, z[i:i + 1], cuda)[0], whole[i]), i
    micro = _decode(_model('T1', decode_batch=2), z, cuda)
    assert torch.equal(micro, whole)


def test_output_layout_and_guard_region(cuda):
    """The ABI writes exactly [B, 3, 4 H, 4 W] floats at `out`: a NaN-filled buffer around it stays NaN."""
    from dmhip._lib import check, load, stream_handle
    z, r32, r64 = _case('T1')
    m = _model('T1')
    zd = z.to(cuda).contiguous()
    n, guard = r32.numel(), 4096
    buf = torch.full((n + 2 * guard, ), float('nan'), device=cuda)
    out = buf[guard:guard + n]
    check(load().dm_vae_decoder_forward(m.native_handle(cuda), zd.data_ptr(), zd.shape[0], 8, 8, _scale32(),
                                        out.data_ptr(), stream_handle(cuda)), 'dm_vae_decoder_forward')
    torch.cuda.synchronize()
    assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + n:]).all()
    _check('T1_layout', out.reshape(r32.shape), r32, r64)


def test_scale_is_applied_as_the_reference_does(cuda):
    """decode(z, scale) == decode(scale * z) with the host's float32 product (1. / scale_factor * z), bit for bit,
    and differs from the unscaled decode."""
    z, r32, r64 = _case('T1')
    m = _model('T1')
    zd = z.to(cuda)
    a = _decode(m, z, cuda)
    b = m.decode(1. / SCALE_FACTOR * zd).sample
    c = m.decode(zd).sample
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert (a - c).abs().max().item() > 1e-2
    _check('T1_scale', a, r32, r64)


def test_range_fallback(cuda, report):
    """An activation beyond the fp16 range: that forward is re-run in bf16x3 (one fallback reported), stays within
    the bound, and the next forward starts in fp16x2 again."""
    from dmhip._lib import range_stats
    z, r32, r64 = _case('T1', variant='range')
    m = _model('T1', 'range')
    h = m.native_handle(cuda)
    assert range_stats(h, 'dm_vae_decoder') == (0, 'fp16x2')
    out = _decode(m, z, cuda)
    _check('T1_range', out, r32, r64, report)
    assert range_stats(h, 'dm_vae_decoder') == (1, 'fp16x2')
    out2 = _decode(m, z, cuda)
    assert range_stats(h, 'dm_vae_decoder') == (2, 'fp16x2')
    assert torch.equal(out, out2)
    # the ordinary weights never trip the flag
    _decode(_model('T1'), _case('T1')[0], cuda)
    assert range_stats(_model('T1').native_handle(cuda), 'dm_vae_decoder')[0] == 0


@pytest.mark.parametrize('math', ['fp32', 'bf16x3'])
def test_arithmetic_arms(cuda, report, math):
    from dmhip._lib import vae_math
    z, r32, r64 = _case('T1')
    m = _model('T1')
    h = m.native_handle(cuda)
    try:
        assert vae_math(h, math) == math
        _check(f'T1_{math}', _decode(m, z, cuda), r32, r64, report)
    finally:
        assert vae_math(h, 'fp16x2') == 'fp16x2'
    with pytest.raises(ValueError):
        from dmhip._lib import check, load
        check(load().dm_vae_decoder_set_math(h, 7), 'dm_vae_decoder_set_math')


def test_plan_cache_profile_and_memory(cuda):
    from dmhip._lib import plan_stats, unet_profile_enable, unet_profile_read
    z, r32, r64 = _case('T1')
    m = _model('T1')
    h = m.native_handle(cuda)
    _decode(m, z, cuda)
    b0, _ = plan_stats(h, 'dm_vae_decoder')
    _decode(m, z, cuda)
    assert plan_stats(h, 'dm_vae_decoder')[0] == b0  # same shape: the cached plan
    unet_profile_enable(h, 1, 'dm_vae_decoder')
    out = _decode(m, z, cuda)
    ops = unet_profile_read(h, 'dm_vae_decoder')
    unet_profile_enable(h, 0, 'dm_vae_decoder')
    _check('T1_profiled', out, r32, r64)
    labels = [o['label'] for o in ops]
    assert labels[0] == 'vae_latent_in_kernel' and labels[-1] == 'conv3x3_small_out' and 'softmax_rows' in labels
    assert all(o['launches'] == 1 for o in ops) and sum(o['ms_total'] for o in ops) > 0


def test_error_codes_launch_nothing(cuda):
    """Channels not a multiple of 32, a parameter count off by one, a parameter of the wrong size and a latent the
    attention GEMMs do not take: each returns its error code with a message, and the output stays untouched."""
    from dmhip._lib import DM_ERR_ARG, DM_ERR_UNSUPPORTED, VaeArch, load, stream_handle, vp
    L = load()
    m = _model('T1')
    a = m._arch_struct()
    dev = [p.to(cuda) for p in m.params]
    ptrs = (vp * len(dev))(*[p.data_ptr() for p in dev])
    nums = (ctypes.c_int64 * len(dev))(*[p.numel() for p in dev])
    h = vp()
    assert L.dm_vae_decoder_create(ctypes.byref(a), ptrs, nums, len(dev) - 1, stream_handle(cuda),
                                   ctypes.byref(h)) == DM_ERR_ARG and not h.value
    assert b'parameter tensors' in L.dm_last_error()
    bad = m._arch_struct()
    bad.ch = 48
    assert L.dm_vae_decoder_create(ctypes.byref(bad), ptrs, nums, len(dev), stream_handle(cuda),
                                   ctypes.byref(h)) == DM_ERR_ARG and not h.value
    assert b'multiple of 32' in L.dm_last_error()
    nums2 = (ctypes.c_int64 * len(dev))(*[p.numel() for p in dev])
    nums2[3] += 1
    assert L.dm_vae_decoder_create(ctypes.byref(a), ptrs, nums2, len(dev), stream_handle(cuda),
                                   ctypes.byref(h)) == DM_ERR_ARG and not h.value
    assert b'parameter 3' in L.dm_last_error()
    z = torch.zeros((1, 4, 5, 5), device=cuda)
    out = torch.full((1, 3, 20, 20), float('nan'), device=cuda)
    hd = m.native_handle(cuda)
    assert L.dm_vae_decoder_forward(hd, z.data_ptr(), 1, 5, 5, 1.0, out.data_ptr(),
                                    stream_handle(cuda)) == DM_ERR_UNSUPPORTED
    assert b'multiple of 4' in L.dm_last_error()
    assert L.dm_vae_decoder_forward(hd, z.data_ptr(), 0, 8, 8, 1.0, out.data_ptr(), stream_handle(cuda)) == DM_ERR_ARG
    assert L.dm_vae_decoder_forward(hd, z.data_ptr(), 1, 8, 8, 1.0, z.data_ptr(), stream_handle(cuda)) == DM_ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    with pytest.raises(ValueError, match='latents'):
        m.decode(torch.zeros((1, 3, 8, 8), device=cuda))


# a reduced DiT on the DiT-XL/2 config (latent 4 x 8 x 8 from img_size 64, 2 blocks of width 64)
TINY_DIT = ['--data.params.img_size', '64', '--data.num_classes', '10',
            '--model.params.vit_config.params.input_size', '8', '--model.params.vit_config.params.hidden_size', '64',
            '--model.params.vit_config.params.depth', '2', '--model.params.vit_config.params.num_heads', '4',
            '--model.params.vit_config.params.num_classes', '10']


def test_end_to_end_checkpoint_dir_decode_latent_and_script(cuda, tmp_path):
    """A diffusers-layout directory on disk -> AutoEncoderKL(dir).decode, DiT.decode_latent, and scripts/sample_cfg.py
    with the from_pretrained override: PNGs (latent size x 4 for this three-level VAE) whose pixels are the
    reference decode of the latents the same run writes without the override, within one 8-bit level."""
    from models.dit.autoencoder import AutoEncoderKL
    from models.dit.dit import DiT
    from scripts import sample_cfg
    from utils.misc import load_config
    vdir = str(tmp_path / 'vae')
    vae_ref.write_checkpoint_dir(vdir, 'T1')
    z, r32, r64 = _case('T1')
    m = AutoEncoderKL(vdir)
    _check('T1_dir', m.decode(z.to(cuda), scale=_scale32()).sample, r32, r64)

    cfg = os.path.join(CONFIGS, 'dit_xl2_256.yaml')
    override = ['--model.params.vae_config.params.from_pretrained', vdir]
    dot = [a[2:] if a.startswith('--') else a for a in TINY_DIT + override]
    conf = load_config(cfg, [f'{k}={v}' for k, v in zip(dot[::2], dot[1::2])])
    dit = DiT(**conf.model.params)
    assert dit.vae is None
    _check('T1_decode_latent', dit.decode_latent(z.to(cuda)), r32, r64)
    assert isinstance(dit.vae, AutoEncoderKL)

    common = ['-c', cfg, '--weights', 'synthetic', '--guidance_scale', '4', '--class_ids', '7',
              '--n_samples_each_class', '3', '--batch_size', '2', '--sampler', 'ddim', '--respace_steps', '5']
    sample_cfg.main(common + ['--save_dir', str(tmp_path / 'lat')] + TINY_DIT)
    sample_cfg.main(common + ['--save_dir', str(tmp_path / 'img')] + TINY_DIT + override)
    assert sorted(os.listdir(tmp_path / 'lat' / 'class7')) == ['0.npy', '1.npy', '2.npy']
    assert sorted(os.listdir(tmp_path / 'img' / 'class7')) == ['0.png', '1.png', '2.png']
    lat = torch.from_numpy(np.stack([np.load(tmp_path / 'lat' / 'class7' / f'{i}.npy') for i in range(3)]))
    with torch.no_grad():
        want = vae_ref.decode(_weights('T1'), lat, SCALE_FACTOR).clamp(-1, 1)
    want = ((want + 1) / 2).mul(255).add_(0.5).clamp_(0, 255).permute(0, 2, 3, 1).to(torch.uint8).numpy()
    for i in range(3):
        got = read_png_rgb(str(tmp_path / 'img' / 'class7' / f'{i}.png'))
        assert got.shape == (32, 32, 3), got.shape
        diff = np.abs(got.astype(np.int16) - want[i].astype(np.int16))
        assert diff.max() <= 1, (i, int(diff.max()))
        assert (diff > 0).mean() < 0.01, (i, float((diff > 0).mean()))
