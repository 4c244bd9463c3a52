"""The native VAE image encoder (dm_vae_encoder, csrc/vae_enc_exec.hip) on the GPU against tests/vae_enc_ref.py, which
tests/golden/vae_enc.npz pins to the reference module (tests/test_vae_enc_host.py).

Configurations (tests/vae_enc_ref.py CONFIGS): E1 narrow maps (2 x 3 x 32 x 32 -> 8 x 8 latents); E2 wide maps
(1 x 3 x 32 x 256: downsamples at Wout = 128 on the stride-2 row-segment tile and at Wout = 64 on whole rows, the
middle attention at L = 512); E3 the real architecture at a cropped size (ch 128, (1, 2, 4, 4), 1 x 3 x 64 x 64).
Inputs are uniform in [-1, 1].

Bound: tests/test_gpu_vae.py::_check, unchanged: max-abs error <= 1e-4 max(1, max|ref|) against the float32 reference,
the ref64 form where the reference's own float32 error exceeds half of that. Measured on the CPU with the reference
module (tests/golden/make_golden_vae_enc.py) e32 / bound is 0.005 (E1), 0.009 (E2), 0.007 (E3), max|moments| 0.64 /
0.69 / 0.54 and every unclamped logvar within +-0.7: the first form applies. References are computed once per case.
"""
import functools
import os

import pytest
import torch

from tests import vae_enc_ref, vae_ref
from tests.test_gpu_vae import _check

pytestmark = pytest.mark.gpu

SCALE_FACTOR = 0.18215
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, 'diffusion-models-pytorch_amd', 'configs')
ZC = vae_ref.Z_CHANNELS


def _scale32() -> float:
    return float(torch.tensor(SCALE_FACTOR, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def _weights(name, variant=''):
    sd = vae_enc_ref.weights(name)
    if variant == 'range':
        for k in ('encoder.down.0.block.0.conv2.weight', 'encoder.down.0.block.0.conv2.bias'):
            sd[k] = sd[k] * 1e6
    if variant == 'clamp':
        sd['quant_conv.bias'] = sd['quant_conv.bias'].clone()
        sd['quant_conv.bias'][ZC:] = torch.tensor([25.0, -35.0, 0.0, 0.0])
    return sd


@functools.lru_cache(maxsize=None)
def _case(name, shape=None, variant='', seed=11):
    """(x, float32 moments, float64 moments) of a case, computed once."""
    sd = _weights(name, variant)
    x = vae_enc_ref.images(name, seed, shape)
    with torch.no_grad():
        r32 = vae_enc_ref.moments(sd, x)
        r64 = vae_enc_ref.moments(sd, x, torch.float64)
    assert torch.isfinite(r32).all()
    return x, r32, r64


@functools.lru_cache(maxsize=None)
def _model(name, variant='', encode_batch=8):
    from models.dit.autoencoder import AutoEncoderKL
    sd = dict(_weights(name, variant))
    sd.update(vae_ref.recipe_state_dict(vae_ref.decoder_shapes(vae_enc_ref.CONFIGS[name])))
    return AutoEncoderKL.from_state_dict(vae_enc_ref.diffusers_config(name), sd, encode_batch=encode_batch)


def _clamped(mom):
    """mean | clamp(logvar): what dm_vae_encoder_forward's moments_out holds."""
    mean, logvar, _ = vae_enc_ref.posterior(mom)
    return torch.cat([mean, logvar], dim=1)


def _moments(m, x, cuda):
    out = m.encode(x.to(cuda)).latent_dist
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('name', ['E1', 'E2', 'E3'])
def test_moments_and_mode_match_reference(cuda, report, name):
    x, r32, r64 = _case(name)
    m = _model(name)
    dist = _moments(m, x, cuda)
    _check(name, dist.parameters, _clamped(r32), _clamped(r64), report)
    z = m.encode_to_latent(x.to(cuda))
    torch.cuda.synchronize()
    _check(name + '_mode', z, r32[:, :ZC], r64[:, :ZC], report)
    assert torch.equal(z, dist.mode())
    if name == 'E2':  # both downsamples on the K = 32 stride-2 kernel: Wout = 128 row segments, Wout = 64 whole rows
        from dmhip._lib import unet_profile_enable, unet_profile_read
        h = m.encoder_handle(cuda)
        unet_profile_enable(h, 1, 'dm_vae_encoder')
        m.encode_to_latent(x.to(cuda))
        labels = [o['label'] for o in unet_profile_read(h, 'dm_vae_encoder')]
        unet_profile_enable(h, 0, 'dm_vae_encoder')
        assert sum('conv_k32_kernel<64,128,32,32' in lb for lb in labels) == 2, labels
        assert not any(lb.startswith('conv_igemm_kernel') for lb in labels), labels
        assert labels[0] == 'conv3x3_small_in' and labels[-1] == 'conv3x3_small_out' and 'softmax_rows' in labels


def test_sample_and_scale(cuda, report):
    """sample with a given noise tensor is mean + std * noise; scale multiplies the result on the device, bit for bit
    the host's float32 product applied to the unscaled latents."""
    x, r32, r64 = _case('E1')
    m = _model('E1')
    noise = torch.randn((2, ZC, 8, 8), generator=torch.Generator().manual_seed(3))
    mean32, _, std32 = vae_enc_ref.posterior(r32)
    mean64, _, std64 = vae_enc_ref.posterior(r64)
    z1 = m.encode_to_latent(x.to(cuda), noise=noise.to(cuda))
    zs = m.encode_to_latent(x.to(cuda), scale=_scale32(), noise=noise.to(cuda))
    torch.cuda.synchronize()
    _check('E1_sample', z1, mean32 + std32 * noise, mean64 + std64 * noise.double(), report)
    assert torch.equal(zs, torch.tensor(SCALE_FACTOR, device=cuda) * z1)
    assert (zs - z1).abs().max().item() > 1e-2


@pytest.mark.parametrize('shape', [(1, 3, 24, 40), (1, 3, 40, 24), (1, 3, 20, 32)])
def test_awkward_shapes(cuda, report, shape):
    """Not multiples of any tile, rows and columns not interchangeable; 20 x 32 gives an odd 5 x 8 latent map."""
    x, r32, r64 = _case('E1', shape)
    _check('E1_%dx%d' % shape[2:], _moments(_model('E1'), x, cuda).parameters, _clamped(r32), _clamped(r64), report)


def test_size_not_a_multiple_raises(cuda):
    """H or W not a multiple of 2^(L-1) = 4: ValueError from the Python surface, DM_ERR_ARG with a message from the
    ABI, and nothing is written."""
    from dmhip._lib import DM_ERR_ARG, load, stream_handle
    m = _model('E1')
    with pytest.raises(ValueError, match='multiples of 4'):
        m.encode(torch.zeros((1, 3, 22, 32), device=cuda))
    x = torch.zeros((1, 3, 22, 32), device=cuda)
    z = torch.full((1, ZC, 5, 8), float('nan'), device=cuda)
    L = load()
    assert L.dm_vae_encoder_forward(m.encoder_handle(cuda), x.data_ptr(), 1, 22, 32, None, 1.0, z.data_ptr(), None,
                                    stream_handle(cuda)) == DM_ERR_ARG
    assert b'multiples of 4' in L.dm_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(z).all()


def test_batch_invariance_and_micro_batches(cuda):
    """Image i of a B = 3 encode is bit-identical to its own B = 1 encode and to the encode_batch = 2 micro-batched
    encode (a batch of 2 and a batch of 1)."""
    x = vae_enc_ref.images('E1', 5, (3, 3, 32, 32)).to(cuda)
    m = _model('E1')
    whole = m.encode(x).latent_dist.parameters
    for i in range(3):
        assert torch.equal(m.encode(x[i:i + 1]).latent_dist.parameters[0], whole[i]), i
    micro = _model('E1', encode_batch=2).encode(x).latent_dist.parameters
    assert torch.equal(micro, whole)


def test_output_layout_and_guard_region(cuda):
    """The ABI writes exactly [B, zc, h, w] floats at z_out and [B, 2 zc, h, w] at moments_out: NaN-filled buffers
    around them stay NaN."""
    from dmhip._lib import check, load, stream_handle
    x, r32, r64 = _case('E1')
    m = _model('E1')
    xd = x.to(cuda).contiguous()
    nz, nm, guard = 2 * ZC * 64, 2 * 2 * ZC * 64, 4096
    bz = torch.full((nz + 2 * guard, ), float('nan'), device=cuda)
    bm = torch.full((nm + 2 * guard, ), float('nan'), device=cuda)
    z, mo = bz[guard:guard + nz], bm[guard:guard + nm]
    check(load().dm_vae_encoder_forward(m.encoder_handle(cuda), xd.data_ptr(), 2, 32, 32, None, 1.0, z.data_ptr(),
                                        mo.data_ptr(), stream_handle(cuda)), 'dm_vae_encoder_forward')
    torch.cuda.synchronize()
    for b, n in ((bz, nz), (bm, nm)):
        assert torch.isnan(b[:guard]).all() and torch.isnan(b[guard + n:]).all()
    _check('E1_layout', mo.reshape(r32.shape), _clamped(r32), _clamped(r64))
    assert torch.equal(z.reshape(2, ZC, 8, 8), mo.reshape(r32.shape)[:, :ZC])


def test_logvar_clamp(cuda):
    """quant_conv.bias[zc:] = (+25, -35, 0, 0): the unclamped logvar stays within +-1.1 of it, so channels 0 and 1
    clamp at every pixel: the returned logvar is exactly 20 and -30, and z is within 2^-21 (|mean| + |std noise|) of
    float32 mean + exp(0.5 logvar) noise computed by torch from the device's own moments (one ulp each for the two
    exp implementations and the final rounding)."""
    x, r32, r64 = _case('E1', variant='clamp')
    lv = r32[:, ZC:]
    assert (lv[:, 0] > 20).all() and (lv[:, 1] < -30).all() and lv[:, 2:].abs().max() < 1.1
    m = _model('E1', 'clamp')
    noise = torch.randn((2, ZC, 8, 8), generator=torch.Generator().manual_seed(4)).to(cuda)
    dist = m.encode(x.to(cuda)).latent_dist
    z = m.encode_to_latent(x.to(cuda), noise=noise)
    torch.cuda.synchronize()
    mom = dist.parameters
    assert (mom[:, ZC] == 20.0).all() and (mom[:, ZC + 1] == -30.0).all()
    mean, logvar = mom[:, :ZC], mom[:, ZC:]
    sn = torch.exp(0.5 * logvar) * noise
    budget = 2.0 ** -21 * (mean.abs() + sn.abs())
    assert ((z - (mean + sn)).abs() <= budget).all(), ((z - (mean + sn)).abs() / budget).max().item()


def test_range_fallback(cuda, report):
    """An activation beyond the fp16 range: that forward is re-run in bf16x3 (one fallback reported), stays within
    the bound, and the next forward starts in fp16x2 again. The weights: down.0.block.0's output conv scaled
    10^6-fold, so the block's output reaches the level's raw-input consumer, the downsample conv, beyond the fp16
    range; every GroupNorm downstream renormalises it (checked on the CPU: the float32 reference is finite, e32
    5.0e-7, 0.005 of the bound). The decoder test's tensor, mid.block_2.conv2, does not serve here: in the encoder
    that block's output is read only by norm_out, in fp32, and the flag stays clear (measured on the GPU: no
    fallback; its CPU e32 is 7.9e-7)."""
    from dmhip._lib import range_stats
    x, r32, r64 = _case('E1', variant='range')
    m = _model('E1', 'range')
    h = m.encoder_handle(cuda)
    assert range_stats(h, 'dm_vae_encoder') == (0, 'fp16x2')
    out = _moments(m, x, cuda).parameters
    _check('E1_range', out, _clamped(r32), _clamped(r64), report)
    assert range_stats(h, 'dm_vae_encoder') == (1, 'fp16x2')
    out2 = _moments(m, x, cuda).parameters
    assert range_stats(h, 'dm_vae_encoder') == (2, 'fp16x2')
    assert torch.equal(out, out2)
    _moments(_model('E1'), _case('E1')[0], cuda)
    assert range_stats(_model('E1').encoder_handle(cuda), 'dm_vae_encoder')[0] == 0


@pytest.mark.parametrize('math', ['fp32', 'bf16x3', 'fp16x2'])
def test_arithmetic_arms(cuda, report, math):
    from dmhip._lib import vae_math
    x, r32, r64 = _case('E2')
    m = _model('E2')
    h = m.encoder_handle(cuda)
    try:
        assert vae_math(h, math, 'dm_vae_encoder') == math
        _check(f'E2_{math}', _moments(m, x, cuda).parameters, _clamped(r32), _clamped(r64), report)
    finally:
        assert vae_math(h, 'fp16x2', 'dm_vae_encoder') == 'fp16x2'


def test_round_trip_encode_latent_decode_latent(cuda, tmp_path):
    """DiT.encode_latent -> decode_latent through an E1 / T1 checkpoint directory (a full state dict written with
    vae_ref.write_safetensors) against the composed references."""
    from models.dit.autoencoder import AutoEncoderKL
    from models.dit.dit import DiT
    from tests.test_gpu_vae import TINY_DIT
    from utils.misc import load_config
    vdir = str(tmp_path / 'vae')
    vae_enc_ref.write_checkpoint_dir(vdir, 'E1')
    x, r32, r64 = _case('E1')
    cfg = os.path.join(CONFIGS, 'dit_xl2_256.yaml')
    dot = [a[2:] if a.startswith('--') else a
           for a in TINY_DIT + ['--model.params.vae_config.params.from_pretrained', vdir]]
    conf = load_config(cfg, [f'{k}={v}' for k, v in zip(dot[::2], dot[1::2])])
    dit = DiT(**conf.model.params).to(cuda)
    assert dit.vae is None
    z = dit.encode_latent(x.to(cuda), sample_posterior=False)
    assert isinstance(dit.vae, AutoEncoderKL)
    s32 = torch.tensor(SCALE_FACTOR, dtype=torch.float32)
    _check('E1_encode_latent', z, s32 * r32[:, :ZC], s32.double() * r64[:, :ZC])
    g = torch.Generator().manual_seed(9)
    zs = dit.encode_latent(x.to(cuda), generator=g)
    noise = torch.randn((2, ZC, 8, 8), generator=torch.Generator().manual_seed(9))
    mean32, _, std32 = vae_enc_ref.posterior(r32)
    mean64, _, std64 = vae_enc_ref.posterior(r64)
    _check('E1_encode_latent_sample', zs, s32 * (mean32 + std32 * noise), s32.double() * (mean64 + std64 * noise))
    img = dit.decode_latent(z)
    torch.cuda.synchronize()
    dsd = vae_ref.weights('T1')
    with torch.no_grad():
        d32 = vae_ref.decode(dsd, s32 * r32[:, :ZC], SCALE_FACTOR)
        d64 = vae_ref.decode(dsd, s32.double() * r64[:, :ZC], SCALE_FACTOR, torch.float64)
    _check('E1_round_trip', img, d32, d64)
