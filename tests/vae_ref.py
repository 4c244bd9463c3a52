"""Reference of the KL-autoencoder latent decoder for the tests: a functional torch restatement (float32 / float64)
of the reference's models.stablediffusion.autoencoder (Decoder :376-483, ResnetBlock :69-128, AttnBlock :131-182,
AutoEncoderKL.decode :522-525) evaluated from a CompVis-layout state dict, the synthetic weight recipe, the three
test configurations and converters to the diffusers key layouts. tests/golden/vae.npz pins it to the reference
module itself (tests/golden/make_golden_vae.py)."""
import numpy as np
import torch
import torch.nn.functional as F

from utils.synthetic import state_dict_sha256, synthetic_state_dict

CONFIGS = {
    # narrow maps, a nin_shortcut at every level, one channel per GroupNorm group at the top
    'T1': dict(ch=32, ch_mult=(1, 2, 4), num_res_blocks=1, z_shape=(2, 4, 8, 8)),
    # wide maps: the middle attention at L = 1024, 64^2 / 128^2 conv tiles
    'T2': dict(ch=32, ch_mult=(1, 1, 2), num_res_blocks=1, z_shape=(1, 4, 32, 32)),
    # the real architecture (sd-vae-ft) at a cropped latent size
    'T3': dict(ch=128, ch_mult=(1, 2, 4, 4), num_res_blocks=2, z_shape=(1, 4, 8, 8)),
}
Z_CHANNELS, OUT_CHANNELS, EPS, GROUPS = 4, 3, 1e-6, 32


def diffusers_config(name_or_cfg):
    """The diffusers AutoencoderKL config.json of a test configuration."""
    c = CONFIGS[name_or_cfg] if isinstance(name_or_cfg, str) else name_or_cfg
    boc = [c['ch'] * m for m in c['ch_mult']]
    return dict(_class_name='AutoencoderKL', act_fn='silu', block_out_channels=boc, in_channels=3,
                out_channels=OUT_CHANNELS, latent_channels=Z_CHANNELS, layers_per_block=c['num_res_blocks'],
                norm_num_groups=GROUPS, up_block_types=['UpDecoderBlock2D'] * len(boc),
                down_block_types=['DownEncoderBlock2D'] * len(boc), sample_size=256)


def decoder_shapes(c):
    """CompVis name -> shape of decoder.* and post_quant_conv.*, in the reference's state_dict() order."""
    ch, mult, nrb = c['ch'], c['ch_mult'], c['num_res_blocks']
    L, top = len(mult), c['ch'] * c['ch_mult'][-1]
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

    conv('decoder.conv_in', top, Z_CHANNELS, 3)
    res('decoder.mid.block_1', top, top)
    norm('decoder.mid.attn_1.norm', top)
    for p in ('q', 'k', 'v', 'proj_out'):
        conv(f'decoder.mid.attn_1.{p}', top, top, 1)
    res('decoder.mid.block_2', top, top)
    for i in range(L):
        co = ch * mult[i]
        ci = top if i == L - 1 else ch * mult[i + 1]
        for j in range(nrb + 1):
            res(f'decoder.up.{i}.block.{j}', ci, co)
            ci = co
        if i != 0:
            conv(f'decoder.up.{i}.upsample.conv', co, co, 3)
    norm('decoder.norm_out', ch * mult[0])
    conv('decoder.conv_out', OUT_CHANNELS, ch * mult[0], 3)
    conv('post_quant_conv', Z_CHANNELS, Z_CHANNELS, 1)
    return out


def recipe_state_dict(like, seed=0):
    """The weight recipe: utils.synthetic.synthetic_state_dict over `like` (name -> tensor or shape), then -- from a
    second PCG64 stream (seed + 1), in key order -- every GroupNorm weight ~ U(0.5, 1.5), every GroupNorm bias ~
    U(-0.5, 0.5) and every conv bias ~ U(-0.1, 0.1): with gamma = 1 and beta ~ 0 a wrong channel or group index in a
    fused GroupNorm prologue would stay invisible."""
    like = {k: (torch.empty(v) if not isinstance(v, torch.Tensor) else v) for k, v in like.items()}
    sd = synthetic_state_dict(like, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    for k, v in sd.items():
        if v.ndim != 1:
            continue
        u = torch.from_numpy(rng.random(v.numel(), dtype=np.float32))
        is_norm = '.norm' in k or 'norm_out' in k
        if is_norm and k.endswith('weight'):
            sd[k] = 0.5 + u
        elif is_norm:
            sd[k] = u - 0.5
        else:
            sd[k] = (u * 2 - 1) * 0.1
    return sd


def weights(name, seed=0):
    """The CompVis-layout decoder state dict of a test configuration."""
    return recipe_state_dict(decoder_shapes(CONFIGS[name]), seed)


def latents(name, seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(CONFIGS[name]['z_shape'], generator=g)


def sha256(sd):
    return state_dict_sha256(sd)


# ----------------------------------------------------------------------------- the decoder
def _gn_silu(x, sd, n):
    h = F.group_norm(x, GROUPS, sd[n + '.weight'], sd[n + '.bias'], EPS)
    return h * torch.sigmoid(h)


def _conv(x, sd, n, pad):
    return F.conv2d(x, sd[n + '.weight'], sd[n + '.bias'], padding=pad)


def _res(x, sd, n):
    h = _conv(_gn_silu(x, sd, n + '.norm1'), sd, n + '.conv1', 1)
    h = _conv(_gn_silu(h, sd, n + '.norm2'), sd, n + '.conv2', 1)
    if n + '.nin_shortcut.weight' in sd:
        x = _conv(x, sd, n + '.nin_shortcut', 0)
    return x + h


def _attn(x, sd, n):
    h = F.group_norm(x, GROUPS, sd[n + '.norm.weight'], sd[n + '.norm.bias'], EPS)
    q, k, v = (_conv(h, sd, f'{n}.{p}', 0) for p in ('q', 'k', 'v'))
    b, c, hh, ww = q.shape
    q = q.reshape(b, c, hh * ww).permute(0, 2, 1)
    k = k.reshape(b, c, hh * ww)
    w = torch.bmm(q, k) * (int(c) ** (-0.5))
    w = F.softmax(w, dim=2)
    v = v.reshape(b, c, hh * ww)
    h = torch.bmm(v, w.permute(0, 2, 1)).reshape(b, c, hh, ww)
    return x + _conv(h, sd, n + '.proj_out', 0)


def decode(sd, z, scale_factor=None, dtype=torch.float32):
    """AutoEncoderKL.decode(z) of the CompVis state dict `sd`; with scale_factor, of `1. / scale_factor * z`
    (models/dit/dit.py decode_latent). dtype float64 evaluates the same graph in double."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    z = z.to(dtype)
    if scale_factor is not None:
        z = 1. / scale_factor * z
    n_levels = 1 + max(int(k.split('.')[2]) for k in sd if k.startswith('decoder.up.'))
    h = _conv(z, sd, 'post_quant_conv', 0)
    h = _conv(h, sd, 'decoder.conv_in', 1)
    h = _res(h, sd, 'decoder.mid.block_1')
    h = _attn(h, sd, 'decoder.mid.attn_1')
    h = _res(h, sd, 'decoder.mid.block_2')
    for i in reversed(range(n_levels)):
        j = 0
        while f'decoder.up.{i}.block.{j}.conv1.weight' in sd:
            h = _res(h, sd, f'decoder.up.{i}.block.{j}')
            j += 1
        if i != 0:
            h = F.interpolate(h, scale_factor=2.0, mode='nearest')
            h = _conv(h, sd, f'decoder.up.{i}.upsample.conv', 1)
    return _conv(_gn_silu(h, sd, 'decoder.norm_out'), sd, 'decoder.conv_out', 1)


# ----------------------------------------------------------------------------- key layouts
def to_diffusers(sd, legacy_attention=False):
    """The CompVis state dict under diffusers' names (attention projections as Linear [C, C] weights); with
    legacy_attention the pre-0.18 attention names. Adds encoder / quant_conv tensors a loader must ignore."""
    n_levels = 1 + max(int(k.split('.')[2]) for k in sd if k.startswith('decoder.up.'))
    attn = (dict(norm='group_norm', q='query', k='key', v='value', proj_out='proj_attn') if legacy_attention else
            {'norm': 'group_norm', 'q': 'to_q', 'k': 'to_k', 'v': 'to_v', 'proj_out': 'to_out.0'})
    out = {'encoder.conv_in.weight': torch.zeros(8, 3, 3, 3), 'quant_conv.weight': torch.zeros(8, 8, 1, 1),
           'quant_conv.bias': torch.zeros(8)}
    for k, v in sd.items():
        p = k.split('.')
        if k.startswith('decoder.mid.attn_1.'):
            nk = f'decoder.mid_block.attentions.0.{attn[p[3]]}.{p[4]}'
            if v.ndim == 4:
                v = v.reshape(v.shape[0], v.shape[1])
        elif k.startswith('decoder.mid.block_'):
            nk = f'decoder.mid_block.resnets.{int(p[2][-1]) - 1}.' + '.'.join(p[3:])
        elif k.startswith('decoder.up.') and p[3] == 'block':
            nk = f'decoder.up_blocks.{n_levels - 1 - int(p[2])}.resnets.{p[4]}.' + '.'.join(p[5:])
        elif k.startswith('decoder.up.') and p[3] == 'upsample':
            nk = f'decoder.up_blocks.{n_levels - 1 - int(p[2])}.upsamplers.0.' + '.'.join(p[4:])
        elif k.startswith('decoder.norm_out.'):
            nk = 'decoder.conv_norm_out.' + p[2]
        else:
            nk = k
        out[nk.replace('nin_shortcut', 'conv_shortcut')] = v
    return out


def write_safetensors(path, sd):
    """A minimal safetensors writer (float32 tensors): 8-byte little-endian header length, JSON header, raw data."""
    import json
    import struct
    header, blobs, off = {}, [], 0
    for k, v in sd.items():
        b = v.detach().to(torch.float32).contiguous().numpy().astype('<f4').tobytes()
        header[k] = dict(dtype='F32', shape=list(v.shape), data_offsets=[off, off + len(b)])
        blobs.append(b)
        off += len(b)
    hj = json.dumps(header, separators=(',', ':')).encode()
    hj += b' ' * (-len(hj) % 8)
    with open(path, 'wb') as f:
        f.write(struct.pack('<Q', len(hj)))
        f.write(hj)
        for b in blobs:
            f.write(b)


def write_checkpoint_dir(path, name, sd=None, legacy_attention=False):
    """A diffusers-layout checkpoint directory (config.json + diffusion_pytorch_model.safetensors)."""
    import json
    import os
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, 'config.json'), 'w') as f:
        json.dump(diffusers_config(name), f)
    write_safetensors(os.path.join(path, 'diffusion_pytorch_model.safetensors'),
                      to_diffusers(weights(name) if sd is None else sd, legacy_attention))
