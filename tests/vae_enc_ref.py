"""Reference of the KL-autoencoder image encoder for the tests: a functional torch restatement (float32 / float64) of
the reference's models.stablediffusion.autoencoder (Encoder :280-373, Downsample :47-66, AutoEncoderKL.encode
:516-520, DiagonalGaussianDistribution) evaluated from a CompVis-layout state dict, the synthetic weight recipe
(tests/vae_ref.py recipe_state_dict over the encoder.* / quant_conv.* shapes), the three test configurations and
converters to the diffusers key layouts. tests/golden/vae_enc.npz pins it to the reference module itself
(tests/golden/make_golden_vae_enc.py)."""
import torch
import torch.nn.functional as F

from tests import vae_ref
from tests.vae_ref import EPS, GROUPS, Z_CHANNELS, _attn, _conv, _gn_silu, _res

IN_CHANNELS = 3
CONFIGS = {
    # narrow maps, a nin_shortcut at levels 1 and 2: 8 x 8 latents
    'E1': dict(ch=32, ch_mult=(1, 2, 4), num_res_blocks=1, x_shape=(2, 3, 32, 32)),
    # wide maps: downsamples at Wo = 128 (row-segment tile) and Wo = 64 (whole rows), attention at L = 512
    'E2': dict(ch=32, ch_mult=(1, 1, 2), num_res_blocks=1, x_shape=(1, 3, 32, 256)),
    # the real architecture (sd-vae-ft) at a cropped image size
    'E3': dict(ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, x_shape=(1, 3, 64, 64)),
}


def diffusers_config(name_or_cfg):
    """The diffusers AutoencoderKL config.json of a test configuration (the decoder's, same architecture)."""
    return vae_ref.diffusers_config(CONFIGS[name_or_cfg] if isinstance(name_or_cfg, str) else name_or_cfg)


def encoder_shapes(c):
    """CompVis name -> shape of encoder.* and quant_conv.*, in the reference's state_dict() order."""
    ch, mult, nrb = c['ch'], c['ch_mult'], c['num_res_blocks']
    L = len(mult)
    out = {}

    def conv(n, co, ci, k):
        out[n + '.weight'] = (co, ci, k, k)
        out[n + '.bias'] = (co, )

    def norm(n, ch_):
        out[n + '.weight'] = (ch_, )
        out[n + '.bias'] = (ch_, )

    def res(n, ci, co):
        norm(n + '.norm1', ci)
        conv(n + '.conv1', co, ci, 3)
        norm(n + '.norm2', co)
        conv(n + '.conv2', co, co, 3)
        if ci != co:
            conv(n + '.nin_shortcut', co, ci, 1)

    conv('encoder.conv_in', ch, IN_CHANNELS, 3)
    ci = ch
    for i in range(L):
        co = ch * mult[i]
        for j in range(nrb):
            res(f'encoder.down.{i}.block.{j}', ci, co)
            ci = co
        if i != L - 1:
            conv(f'encoder.down.{i}.downsample.conv', ci, ci, 3)
    res('encoder.mid.block_1', ci, ci)
    norm('encoder.mid.attn_1.norm', ci)
    for p in ('q', 'k', 'v', 'proj_out'):
        conv(f'encoder.mid.attn_1.{p}', ci, ci, 1)
    res('encoder.mid.block_2', ci, ci)
    norm('encoder.norm_out', ci)
    conv('encoder.conv_out', 2 * Z_CHANNELS, ci, 3)
    conv('quant_conv', 2 * Z_CHANNELS, 2 * Z_CHANNELS, 1)
    return out


def weights(name, seed=0):
    """The CompVis-layout encoder state dict of a test configuration."""
    return vae_ref.recipe_state_dict(encoder_shapes(CONFIGS[name]), seed)


def full_weights(name, seed=0):
    """Encoder and decoder tensors of the same architecture in one CompVis-layout state dict."""
    c = CONFIGS[name]
    sd = dict(weights(name, seed))
    sd.update(vae_ref.recipe_state_dict(vae_ref.decoder_shapes(c), seed))
    return sd


def images(name, seed=11, shape=None):
    """Inputs uniform in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape or CONFIGS[name]['x_shape'], generator=g) * 2 - 1


# ----------------------------------------------------------------------------- the encoder
def moments(sd, x, dtype=torch.float32):
    """AutoEncoderKL.encode(x).parameters of the CompVis state dict `sd`: [B, 2 zc, h, w] = mean | unclamped logvar.
    dtype float64 evaluates the same graph in double."""
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith('encoder.') or k.startswith('quant_conv.')}
    h = _conv(x.to(dtype), sd, 'encoder.conv_in', 1)
    n_levels = 1 + max(int(k.split('.')[2]) for k in sd if k.startswith('encoder.down.'))
    for i in range(n_levels):
        j = 0
        while f'encoder.down.{i}.block.{j}.conv1.weight' in sd:
            h = _res(h, sd, f'encoder.down.{i}.block.{j}')
            j += 1
        if i != n_levels - 1:
            n = f'encoder.down.{i}.downsample.conv'
            h = F.conv2d(F.pad(h, (0, 1, 0, 1), mode='constant', value=0), sd[n + '.weight'], sd[n + '.bias'], stride=2)
    h = _res(h, sd, 'encoder.mid.block_1')
    h = _attn(h, sd, 'encoder.mid.attn_1')
    h = _res(h, sd, 'encoder.mid.block_2')
    h = _conv(_gn_silu(h, sd, 'encoder.norm_out'), sd, 'encoder.conv_out', 1)
    if 'quant_conv.weight' in sd:
        h = _conv(h, sd, 'quant_conv', 0)
    return h


def posterior(mom):
    """(mean, clamped logvar, std) of the moments, as DiagonalGaussianDistribution."""
    mean, logvar = torch.chunk(mom, 2, dim=1)
    logvar = torch.clamp(logvar, -30.0, 20.0)
    return mean, logvar, torch.exp(0.5 * logvar)


# ----------------------------------------------------------------------------- key layouts
def to_diffusers(sd, legacy_attention=False):
    """The CompVis state dict (encoder.* / quant_conv.*; decoder tensors go through vae_ref.to_diffusers) under
    diffusers' names; with legacy_attention the pre-0.18 attention names."""
    attn = (dict(norm='group_norm', q='query', k='key', v='value', proj_out='proj_attn') if legacy_attention else
            {'norm': 'group_norm', 'q': 'to_q', 'k': 'to_k', 'v': 'to_v', 'proj_out': 'to_out.0'})
    dec = {k: v for k, v in sd.items() if k.startswith('decoder.') or k.startswith('post_quant_conv.')}
    out = {}
    if dec:
        out = {k: v for k, v in vae_ref.to_diffusers(dec, legacy_attention).items()
               if k.startswith('decoder.') or k.startswith('post_quant_conv.')}
    for k, v in sd.items():
        if k in dec:
            continue
        p = k.split('.')
        if k.startswith('encoder.mid.attn_1.'):
            nk = f'encoder.mid_block.attentions.0.{attn[p[3]]}.{p[4]}'
            if v.ndim == 4:
                v = v.reshape(v.shape[0], v.shape[1])
        elif k.startswith('encoder.mid.block_'):
            nk = f'encoder.mid_block.resnets.{int(p[2][-1]) - 1}.' + '.'.join(p[3:])
        elif k.startswith('encoder.down.') and p[3] == 'block':
            nk = f'encoder.down_blocks.{p[2]}.resnets.{p[4]}.' + '.'.join(p[5:])
        elif k.startswith('encoder.down.') and p[3] == 'downsample':
            nk = f'encoder.down_blocks.{p[2]}.downsamplers.0.' + '.'.join(p[4:])
        elif k.startswith('encoder.norm_out.'):
            nk = 'encoder.conv_norm_out.' + p[2]
        else:
            nk = k
        out[nk.replace('nin_shortcut', 'conv_shortcut')] = v
    return out


def write_checkpoint_dir(path, name, sd=None, legacy_attention=False):
    """A diffusers-layout checkpoint directory (config.json + diffusion_pytorch_model.safetensors) with encoder and
    decoder."""
    import json
    import os
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(diffusers_config(name), f)
    vae_ref.write_safetensors(os.path.join(path, 'diffusion_pytorch_model.safetensors'),
                              to_diffusers(full_weights(name) if sd is None else sd, legacy_attention))
