"""models/dit/autoencoder.py: the KL autoencoder (latent decoder and image encoder) the reference's DiT wraps.

The reference builds diffusers' ``AutoencoderKL.from_pretrained('stabilityai/sd-vae-ft-ema')``: a network fetch.
Here ``AutoEncoderKL(from_pretrained)`` takes a checkpoint directory that is already on disk, in the diffusers
layout (``config.json`` plus ``diffusion_pytorch_model.safetensors`` or ``.bin``), and decodes on the native engine
(dm_vae_decoder, csrc/vae_exec.hip). Anything else -- a hub id -- raises NotImplementedError before any file or
network access, and the sampling scripts then keep their latents (``.npy``).

``encode(x).latent_dist`` is the posterior (``DiagonalGaussianDistribution``: ``sample()`` / ``mode()``, the diffusers
call shape) from the native encoder (dm_vae_encoder, csrc/vae_enc_exec.hip); ``encode_to_latent`` is the fused form.
The encoder is built on the first ``encode``: a decoder-only state dict constructs and decodes as before, and only
``encode`` reports its missing ``encoder.*`` / ``quant_conv.*`` tensors.

State dicts are accepted in three key layouts and mapped to the C ABI's parameter order (the reference
``models.stablediffusion.autoencoder.AutoEncoderKL.state_dict()`` order of ``decoder.*``, then ``post_quant_conv.*``):
current diffusers names (``mid_block.attentions.0.to_q`` ...), diffusers' legacy attention names (``query``, ``key``,
``value``, ``proj_attn``) and the CompVis names of the reference module (``mid.attn_1.q`` ..., 1x1 conv weights,
``up.0`` the highest resolution).
"""
import ctypes
import json
import os
from typing import Dict, List, Mapping, Tuple

import torch
from torch import Tensor

SUPPORTED_UP_BLOCK = 'UpDecoderBlock2D'
SUPPORTED_DOWN_BLOCK = 'DownEncoderBlock2D'
WEIGHT_FILES = ('diffusion_pytorch_model.safetensors', 'diffusion_pytorch_model.bin')


class DecoderOutput:
    """What ``decode`` returns: ``.sample`` holds the decoded images (diffusers' DecoderOutput)."""

    def __init__(self, sample: Tensor):
        self.sample = sample


class DiagonalGaussianDistribution:
    """The posterior N(mean, std^2) of ``encode`` (reference models/stablediffusion/autoencoder.py, diffusers'
    class of the same name): ``parameters`` [B, 2 C, H, W] = mean | logvar, logvar clamped to [-30, 20]."""

    def __init__(self, parameters: Tensor):
        self.parameters = parameters
        self.mean, logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def sample(self, generator=None) -> Tensor:
        """mean + std * noise; the noise is torch.randn on the distribution's device (RNG stays with torch)."""
        noise = torch.randn(self.mean.shape, generator=generator, device=self.mean.device, dtype=self.mean.dtype)
        return self.mean + self.std * noise

    def mode(self) -> Tensor:
        return self.mean


class EncoderOutput:
    """What ``encode`` returns: ``.latent_dist`` is the posterior (diffusers' AutoencoderKLOutput)."""

    def __init__(self, latent_dist: DiagonalGaussianDistribution):
        self.latent_dist = latent_dist


def enc_arch_from_config(config: Mapping, arch: Mapping) -> dict:
    """The encoder's hyper-parameters from a diffusers config the decoder checks (arch_from_config) have passed.
    Raises ValueError naming every offending entry."""
    bad = []
    boc = list(config.get('block_out_channels', ()))
    dbt = list(config.get('down_block_types', [SUPPORTED_DOWN_BLOCK] * len(boc)))
    if any(t != SUPPORTED_DOWN_BLOCK for t in dbt) or len(dbt) != len(boc):
        bad.append(f'down_block_types={dbt!r} ({SUPPORTED_DOWN_BLOCK} per level: attention in the middle block only)')
    ic = config.get('in_channels', 3)
    if not isinstance(ic, int) or not 1 <= ic <= 4:
        bad.append(f'in_channels={ic!r} (1..4)')
    if config.get('double_z', True) is False:
        bad.append('double_z=False (the encoder returns mean and logvar)')
    if arch['num_res_blocks'] < 1:
        bad.append(f'layers_per_block={arch["num_res_blocks"]!r} (the encoder needs >= 1)')
    if bad:
        raise ValueError('unsupported VAE config: ' + '; '.join(bad))
    return dict(ch=arch['ch'], ch_mult=arch['ch_mult'], num_res_blocks=arch['num_res_blocks'],
                z_channels=arch['z_channels'], in_channels=ic, norm_groups=32, norm_eps=1e-6,
                quant=bool(config.get('use_quant_conv', True)))


def arch_from_config(config: Mapping) -> dict:
    """Validate a diffusers AutoencoderKL ``config.json`` against what the engine decodes; returns the decoder
    hyper-parameters (ch, ch_mult, num_res_blocks, z_channels, out_channels, norm_groups, post_quant).
    Raises ValueError naming every offending entry."""
    bad = []
    boc = list(config.get('block_out_channels', ()))
    if not boc or any((not isinstance(c, int)) or c <= 0 for c in boc):
        bad.append(f'block_out_channels={boc!r} (a non-empty list of positive ints)')
    elif any(c % boc[0] or c % 32 or c > 1024 for c in boc) or len(boc) > 8:
        bad.append(f'block_out_channels={boc!r} (at most 8 levels, each a multiple of the first and of 32, <= 1024)')
    lpb = config.get('layers_per_block', 1)
    if not isinstance(lpb, int) or lpb < 0:
        bad.append(f'layers_per_block={lpb!r}')
    zc = config.get('latent_channels', 4)
    if not isinstance(zc, int) or not 1 <= zc <= 4:
        bad.append(f'latent_channels={zc!r} (1..4)')
    oc = config.get('out_channels', 3)
    if not isinstance(oc, int) or not 1 <= oc <= 8:
        bad.append(f'out_channels={oc!r} (1..8)')
    if config.get('norm_num_groups', 32) != 32:
        bad.append(f'norm_num_groups={config.get("norm_num_groups")!r} (32)')
    if config.get('act_fn', 'silu') not in ('silu', 'swish'):
        bad.append(f'act_fn={config.get("act_fn")!r} (silu)')
    ubt = list(config.get('up_block_types', [SUPPORTED_UP_BLOCK] * len(boc)))
    if any(t != SUPPORTED_UP_BLOCK for t in ubt) or (boc and len(ubt) != len(boc)):
        bad.append(f'up_block_types={ubt!r} ({SUPPORTED_UP_BLOCK} per level: attention in the middle block only)')
    if not config.get('mid_block_add_attention', True):
        bad.append('mid_block_add_attention=False (the middle block has one single-head attention)')
    # the middle attention is one head of block_out_channels[-1] channels (diffusers passes attention_head_dim =
    # block_out_channels[-1]); a config that states otherwise is another network
    ahd = config.get('attention_head_dim', None)
    if ahd is not None and boc and ahd != boc[-1]:
        bad.append(f'attention_head_dim={ahd!r} (single-head middle attention: {boc[-1]})')
    if bad:
        raise ValueError('unsupported VAE config: ' + '; '.join(bad))
    return dict(ch=boc[0], ch_mult=tuple(c // boc[0] for c in boc), num_res_blocks=lpb, z_channels=zc,
                out_channels=oc, norm_groups=32, norm_eps=1e-6,
                post_quant=bool(config.get('use_post_quant_conv', True)))


def _res_names(prefix: str, shortcut: bool) -> List[str]:
    parts = ['norm1', 'conv1', 'norm2', 'conv2'] + (['nin_shortcut'] if shortcut else [])
    return [f'{prefix}.{p}.{s}' for p in parts for s in ('weight', 'bias')]


def abi_param_names(arch: Mapping) -> List[Tuple[str, Tuple[int, ...]]]:
    """(CompVis name, shape) of every decoder parameter in the C ABI's order."""
    ch, mult, nrb, zc = arch['ch'], arch['ch_mult'], arch['num_res_blocks'], arch['z_channels']
    L = len(mult)
    top = ch * mult[-1]
    shapes = {}
    names = []

    def conv(name, cout, cin, k):
        names.extend([f'{name}.weight', f'{name}.bias'])
        shapes[f'{name}.weight'] = (cout, cin, k, k)
        shapes[f'{name}.bias'] = (cout, )

    def norm(name, c):
        names.extend([f'{name}.weight', f'{name}.bias'])
        shapes[f'{name}.weight'] = shapes[f'{name}.bias'] = (c, )

    def res(prefix, cin, cout):
        norm(f'{prefix}.norm1', cin)
        conv(f'{prefix}.conv1', cout, cin, 3)
        norm(f'{prefix}.norm2', cout)
        conv(f'{prefix}.conv2', cout, cout, 3)
        if cin != cout:
            conv(f'{prefix}.nin_shortcut', cout, cin, 1)

    conv('decoder.conv_in', top, zc, 3)
    res('decoder.mid.block_1', top, top)
    norm('decoder.mid.attn_1.norm', top)
    for p in ('q', 'k', 'v', 'proj_out'):
        conv(f'decoder.mid.attn_1.{p}', top, top, 1)
    res('decoder.mid.block_2', top, top)
    for i in range(L):
        cout = ch * mult[i]
        cin = top if i == L - 1 else ch * mult[i + 1]
        for j in range(nrb + 1):
            res(f'decoder.up.{i}.block.{j}', cin, cout)
            cin = cout
        if i != 0:
            conv(f'decoder.up.{i}.upsample.conv', cout, cout, 3)
    norm('decoder.norm_out', ch * mult[0])
    conv('decoder.conv_out', arch['out_channels'], ch * mult[0], 3)
    if arch['post_quant']:
        conv('post_quant_conv', zc, zc, 1)
    return [(n, shapes[n]) for n in names]


def enc_abi_param_names(arch: Mapping) -> List[Tuple[str, Tuple[int, ...]]]:
    """(CompVis name, shape) of every encoder parameter in the C ABI's order (``encoder.*``, then ``quant_conv.*``)."""
    ch, mult, nrb, zc = arch['ch'], arch['ch_mult'], arch['num_res_blocks'], arch['z_channels']
    L = len(mult)
    names = []

    def conv(name, cout, cin, k):
        names.append((f'{name}.weight', (cout, cin, k, k)))
        names.append((f'{name}.bias', (cout, )))

    def norm(name, c):
        names.append((f'{name}.weight', (c, )))
        names.append((f'{name}.bias', (c, )))

    def res(prefix, cin, cout):
        norm(f'{prefix}.norm1', cin)
        conv(f'{prefix}.conv1', cout, cin, 3)
        norm(f'{prefix}.norm2', cout)
        conv(f'{prefix}.conv2', cout, cout, 3)
        if cin != cout:
            conv(f'{prefix}.nin_shortcut', cout, cin, 1)

    conv('encoder.conv_in', ch, arch['in_channels'], 3)
    cin = ch
    for i in range(L):
        cout = ch * mult[i]
        for j in range(nrb):
            res(f'encoder.down.{i}.block.{j}', cin, cout)
            cin = cout
        if i != L - 1:
            conv(f'encoder.down.{i}.downsample.conv', cin, cin, 3)
    res('encoder.mid.block_1', cin, cin)
    norm('encoder.mid.attn_1.norm', cin)
    for p in ('q', 'k', 'v', 'proj_out'):
        conv(f'encoder.mid.attn_1.{p}', cin, cin, 1)
    res('encoder.mid.block_2', cin, cin)
    norm('encoder.norm_out', cin)
    conv('encoder.conv_out', 2 * zc, cin, 3)
    if arch['quant']:
        conv('quant_conv', 2 * zc, 2 * zc, 1)
    return names


_ATTN_CURRENT = {'group_norm': 'norm', 'to_q': 'q', 'to_k': 'k', 'to_v': 'v', 'to_out.0': 'proj_out'}
_ATTN_LEGACY = {'group_norm': 'norm', 'query': 'q', 'key': 'k', 'value': 'v', 'proj_attn': 'proj_out'}


def _to_compvis(key: str, n_levels: int) -> str:
    """A diffusers decoder key -> its CompVis name (keys of other layouts come back unchanged)."""
    if not key.startswith('decoder.'):
        return key
    rest = key[len('decoder.'):]
    stem, _, leaf = rest.rpartition('.')
    if rest.startswith('mid_block.attentions.0.'):
        sub = stem[len('mid_block.attentions.0.'):]
        for table in (_ATTN_CURRENT, _ATTN_LEGACY):
            if sub in table:
                return f'decoder.mid.attn_1.{table[sub]}.{leaf}'
        return key
    if rest.startswith('mid_block.resnets.'):
        parts = rest.split('.')
        if parts[2] in ('0', '1'):
            tail = '.'.join(parts[3:]).replace('conv_shortcut', 'nin_shortcut')
            return f'decoder.mid.block_{int(parts[2]) + 1}.{tail}'
        return key
    if rest.startswith('up_blocks.'):
        parts = rest.split('.')
        if not parts[1].isdigit():
            return key
        lvl = n_levels - 1 - int(parts[1])
        if parts[2] == 'resnets':
            tail = '.'.join(parts[4:]).replace('conv_shortcut', 'nin_shortcut')
            return f'decoder.up.{lvl}.block.{parts[3]}.{tail}'
        if parts[2] == 'upsamplers' and parts[3] == '0':
            return f'decoder.up.{lvl}.upsample.' + '.'.join(parts[4:])
        return key
    if rest.startswith('conv_norm_out.'):
        return 'decoder.norm_out.' + leaf
    return key


def _enc_to_compvis(key: str) -> str:
    """A diffusers encoder key -> its CompVis name (keys of other layouts come back unchanged); down_blocks.{i} is
    down.{i}: no index reversal, unlike the decoder's up."""
    if not key.startswith('encoder.'):
        return key
    rest = key[len('encoder.'):]
    stem, _, leaf = rest.rpartition('.')
    if rest.startswith('mid_block.attentions.0.'):
        sub = stem[len('mid_block.attentions.0.'):]
        for table in (_ATTN_CURRENT, _ATTN_LEGACY):
            if sub in table:
                return f'encoder.mid.attn_1.{table[sub]}.{leaf}'
        return key
    if rest.startswith('mid_block.resnets.'):
        parts = rest.split('.')
        if parts[2] in ('0', '1'):
            tail = '.'.join(parts[3:]).replace('conv_shortcut', 'nin_shortcut')
            return f'encoder.mid.block_{int(parts[2]) + 1}.{tail}'
        return key
    if rest.startswith('down_blocks.'):
        parts = rest.split('.')
        if not parts[1].isdigit():
            return key
        if parts[2] == 'resnets':
            tail = '.'.join(parts[4:]).replace('conv_shortcut', 'nin_shortcut')
            return f'encoder.down.{parts[1]}.block.{parts[3]}.{tail}'
        if parts[2] == 'downsamplers' and parts[3] == '0':
            return f'encoder.down.{parts[1]}.downsample.' + '.'.join(parts[4:])
        return key
    if rest.startswith('conv_norm_out.'):
        return 'encoder.norm_out.' + leaf
    return key


def enc_abi_params(arch: Mapping, state_dict: Mapping[str, Tensor]) -> List[Tensor]:
    """The encoder's parameters in the C ABI's order (float32 CPU tensors, attention and quant_conv weights as [C][C]
    matrices) from a state dict in any of the three layouts. Missing or unexpected ``encoder.*`` / ``quant_conv.*``
    keys, and tensors of the wrong size, raise ValueError listing them."""
    have = {}
    for k, v in state_dict.items():
        if k.startswith('encoder.') or k.startswith('quant_conv.'):
            have[_enc_to_compvis(k)] = (k, v)
    want = enc_abi_param_names(arch)
    wanted = {n for n, _ in want}
    missing = [n for n, _ in want if n not in have]
    extra = sorted(orig for name, (orig, _) in have.items() if name not in wanted)
    if missing or extra:
        raise ValueError('VAE encoder state dict does not match its config: '
                         + (f'missing keys {missing}' if missing else '')
                         + ('; ' if missing and extra else '')
                         + (f'unexpected keys {extra}' if extra else ''))
    out, wrong = [], []
    for name, shape in want:
        orig, t = have[name]
        n = 1
        for s in shape:
            n *= s
        if t.numel() != n:
            wrong.append(f'{orig}: {tuple(t.shape)}, expected {shape}')
            continue
        t = t.detach().to('cpu', torch.float32)
        if name.startswith('encoder.mid.attn_1.') and name.endswith('.weight') and '.norm.' not in name \
                or name == 'quant_conv.weight':
            t = t.reshape(shape[0], shape[1])
        else:
            t = t.reshape(shape)
        out.append(t.contiguous())
    if wrong:
        raise ValueError('VAE encoder state dict has tensors of the wrong size: ' + '; '.join(wrong))
    return out


def abi_params(arch: Mapping, state_dict: Mapping[str, Tensor]) -> List[Tensor]:
    """The decoder's parameters in the C ABI's order (float32 CPU tensors, attention and post_quant weights as
    [C][C] matrices) from a state dict in any of the three layouts. Encoder and quant_conv tensors are ignored;
    missing or unexpected decoder keys, and tensors of the wrong size, raise ValueError listing them."""
    L = len(arch['ch_mult'])
    have = {}
    for k, v in state_dict.items():
        if k.startswith('decoder.') or k.startswith('post_quant_conv.'):
            have[_to_compvis(k, L)] = (k, v)
    want = abi_param_names(arch)
    missing = [n for n, _ in want if n not in have]
    extra = sorted(orig for name, (orig, _) in have.items() if name not in {n for n, _ in want})
    if missing or extra:
        raise ValueError('VAE decoder state dict does not match its config: '
                         + (f'missing keys {missing}' if missing else '')
                         + ('; ' if missing and extra else '')
                         + (f'unexpected keys {extra}' if extra else ''))
    out, wrong = [], []
    for name, shape in want:
        orig, t = have[name]
        n = 1
        for s in shape:
            n *= s
        if t.numel() != n:
            wrong.append(f'{orig}: {tuple(t.shape)}, expected {shape}')
            continue
        t = t.detach().to('cpu', torch.float32)
        if name.startswith('decoder.mid.attn_1.') and name.endswith('.weight') and '.norm.' not in name \
                or name == 'post_quant_conv.weight':
            t = t.reshape(shape[0], shape[1])
        else:
            t = t.reshape(shape)
        out.append(t.contiguous())
    if wrong:
        raise ValueError('VAE decoder state dict has tensors of the wrong size: ' + '; '.join(wrong))
    return out


class AutoEncoderKL:
    """The KL autoencoder on the native engine: ``decode`` (built with the object) and ``encode`` (built on first use).

    ``AutoEncoderKL(from_pretrained)``: an existing local checkpoint directory in the diffusers layout.
    ``AutoEncoderKL.from_state_dict(config, state_dict)``: a diffusers config dict and the weights.
    ``decode(z).sample``: images for latents ``z`` [B, latent_channels, H, W] on a ROCm device, decoded
    ``decode_batch`` images at a time (the workspace is that of one micro-batch).
    ``encode(x).latent_dist`` / ``encode_to_latent(x)``: the posterior / latents of images ``x`` [B, in_channels,
    H, W], encoded ``encode_batch`` images at a time."""

    def __init__(self, from_pretrained: str = None, decode_batch: int = 8, encode_batch: int = 8, **kwargs):
        if not isinstance(from_pretrained, (str, os.PathLike)) or not os.path.isdir(from_pretrained):
            raise NotImplementedError(
                f'AutoEncoderKL: {from_pretrained!r} is not a local checkpoint directory; the engine never fetches '
                'weights. Pass model.params.vae_config.params.from_pretrained=/path/to/dir (config.json + '
                'diffusion_pytorch_model.safetensors or .bin)')
        path = os.fspath(from_pretrained)
        cfg_path = os.path.join(path, 'config.json')
        if not os.path.isfile(cfg_path):
            raise FileNotFoundError(f'{cfg_path} not found')
        with open(cfg_path) as f:
            config = json.load(f)
        for name in WEIGHT_FILES:
            wpath = os.path.join(path, name)
            if os.path.isfile(wpath):
                break
        else:
            raise FileNotFoundError(f'no weights in {path}: expected one of {WEIGHT_FILES}')
        if wpath.endswith('.safetensors'):
            from utils.safetensors_io import load_safetensors
            sd = load_safetensors(wpath)
        else:
            sd = torch.load(wpath, map_location='cpu', weights_only=True)
        self._init(config, sd, decode_batch, encode_batch)

    @classmethod
    def from_state_dict(cls, config: Mapping, state_dict: Mapping[str, Tensor], decode_batch: int = 8,
                        encode_batch: int = 8):
        self = cls.__new__(cls)
        self._init(config, state_dict, decode_batch, encode_batch)
        return self

    def _init(self, config, state_dict, decode_batch, encode_batch=8):
        if int(decode_batch) < 1:
            raise ValueError('decode_batch must be >= 1')
        if int(encode_batch) < 1:
            raise ValueError('encode_batch must be >= 1')
        self.encode_batch = int(encode_batch)
        # the encoder is built on the first encode: its tensors are kept as given (no copy) until then
        self._enc_source = {k: v for k, v in state_dict.items()
                            if k.startswith('encoder.') or k.startswith('quant_conv.')}
        self.enc_arch = None
        self.enc_params = None
        self._enc_handles: Dict[torch.device, ctypes.c_void_p] = {}
        self.config = dict(config)
        self.arch = arch_from_config(config)
        self.params = abi_params(self.arch, state_dict)
        self.decode_batch = int(decode_batch)
        self.upscale = 2 ** (len(self.arch['ch_mult']) - 1)
        self._handles: Dict[torch.device, ctypes.c_void_p] = {}

    # ----------------------------------------------------------- native side
    def _arch_struct(self):
        from dmhip._lib import VaeArch
        a = VaeArch()
        a.z_channels, a.out_channels, a.ch = self.arch['z_channels'], self.arch['out_channels'], self.arch['ch']
        a.n_levels = len(self.arch['ch_mult'])
        for i, m in enumerate(self.arch['ch_mult']):
            a.ch_mult[i] = m
        a.num_res_blocks = self.arch['num_res_blocks']
        a.norm_groups, a.norm_eps = self.arch['norm_groups'], self.arch['norm_eps']
        a.post_quant = int(self.arch['post_quant'])
        return a

    def native_handle(self, device) -> ctypes.c_void_p:
        """The dm_vae_decoder on `device` (created on first use; the weights are packed into library memory)."""
        from dmhip._lib import check, load, stream_handle, vp
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError(f'dm_hip: the VAE decoder runs only on ROCm devices, got {device} (no CPU fallback)')
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._handles:
            with torch.cuda.device(device):
                dev = [p.to(device) for p in self.params]
                ptrs = (vp * len(dev))(*[p.data_ptr() for p in dev])
                nums = (ctypes.c_int64 * len(dev))(*[p.numel() for p in dev])
                h = vp()
                check(load().dm_vae_decoder_create(ctypes.byref(self._arch_struct()), ptrs, nums, len(dev),
                                                   stream_handle(device), ctypes.byref(h)), 'dm_vae_decoder_create')
                torch.cuda.synchronize(device)  # the packing reads `dev`
            self._handles[device] = h
        return self._handles[device]

    def decode(self, z: Tensor, scale: float = 1.0) -> DecoderOutput:
        """Images [B, out_channels, H * upscale, W * upscale] (float32, unclamped) of the latents ``scale * z``;
        ``scale`` is rounded to float32 and multiplied on the device (DiT.decode_latent scales before calling)."""
        from dmhip._lib import check, load, require_device_tensor, stream_handle
        if z.ndim != 4 or z.shape[1] != self.arch['z_channels']:
            raise ValueError(f'expected latents [B, {self.arch["z_channels"]}, H, W], got {tuple(z.shape)}')
        z = z.to(torch.float32).contiguous()
        require_device_tensor(z, 'z')
        B, _, H, W = z.shape
        out = torch.empty((B, self.arch['out_channels'], H * self.upscale, W * self.upscale), device=z.device)
        h = self.native_handle(z.device)
        with torch.cuda.device(z.device):
            for b0 in range(0, B, self.decode_batch):
                zb, ob = z[b0:b0 + self.decode_batch], out[b0:b0 + self.decode_batch]
                check(load().dm_vae_decoder_forward(h, zb.data_ptr(), zb.shape[0], H, W, float(scale), ob.data_ptr(),
                                                    stream_handle(z.device)), 'dm_vae_decoder_forward')
        return DecoderOutput(out)

    # ----------------------------------------------------------- encoder
    def _enc_prepare(self):
        if self.enc_params is None:
            arch = enc_arch_from_config(self.config, self.arch)
            self.enc_params = enc_abi_params(arch, self._enc_source)
            self.enc_arch = arch

    def _enc_arch_struct(self):
        from dmhip._lib import VaeEncArch
        a = VaeEncArch()
        e = self.enc_arch
        a.in_channels, a.z_channels, a.ch = e['in_channels'], e['z_channels'], e['ch']
        a.n_levels = len(e['ch_mult'])
        for i, m in enumerate(e['ch_mult']):
            a.ch_mult[i] = m
        a.num_res_blocks = e['num_res_blocks']
        a.norm_groups, a.norm_eps = e['norm_groups'], e['norm_eps']
        a.quant = int(e['quant'])
        return a

    def encoder_handle(self, device) -> ctypes.c_void_p:
        """The dm_vae_encoder on `device` (created on first use; raises ValueError listing what the state dict
        lacks for an encoder)."""
        from dmhip._lib import check, load, stream_handle, vp
        self._enc_prepare()
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError(f'dm_hip: the VAE encoder runs only on ROCm devices, got {device} (no CPU fallback)')
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._enc_handles:
            with torch.cuda.device(device):
                dev = [p.to(device) for p in self.enc_params]
                ptrs = (vp * len(dev))(*[p.data_ptr() for p in dev])
                nums = (ctypes.c_int64 * len(dev))(*[p.numel() for p in dev])
                h = vp()
                check(load().dm_vae_encoder_create(ctypes.byref(self._enc_arch_struct()), ptrs, nums, len(dev),
                                                   stream_handle(device), ctypes.byref(h)), 'dm_vae_encoder_create')
                torch.cuda.synchronize(device)  # the packing reads `dev`
            self._enc_handles[device] = h
        return self._enc_handles[device]

    def _encode(self, x: Tensor, noise, scale: float, want_moments: bool):
        from dmhip._lib import check, load, require_device_tensor, stream_handle
        self._enc_prepare()
        e = self.enc_arch
        if x.ndim != 4 or x.shape[1] != e['in_channels']:
            raise ValueError(f'expected images [B, {e["in_channels"]}, H, W], got {tuple(x.shape)}')
        B, _, H, W = x.shape
        f = self.upscale
        if H % f or W % f:
            raise ValueError(f'image H and W must be multiples of {f}, got {H} x {W}')
        x = x.to(torch.float32).contiguous()
        require_device_tensor(x, 'x')
        zc = e['z_channels']
        if noise is not None:
            if tuple(noise.shape) != (B, zc, H // f, W // f):
                raise ValueError(f'expected noise {(B, zc, H // f, W // f)}, got {tuple(noise.shape)}')
            noise = noise.to(torch.float32).contiguous()
            require_device_tensor(noise, 'noise')
        z = torch.empty((B, zc, H // f, W // f), device=x.device)
        mom = torch.empty((B, 2 * zc, H // f, W // f), device=x.device) if want_moments else None
        h = self.encoder_handle(x.device)
        with torch.cuda.device(x.device):
            for b0 in range(0, B, self.encode_batch):
                sl = slice(b0, b0 + self.encode_batch)
                xb = x[sl]
                check(load().dm_vae_encoder_forward(
                    h, xb.data_ptr(), xb.shape[0], H, W, noise[sl].data_ptr() if noise is not None else None,
                    float(scale), z[sl].data_ptr(), mom[sl].data_ptr() if want_moments else None,
                    stream_handle(x.device)), 'dm_vae_encoder_forward')
        return z, mom

    def encode(self, x: Tensor) -> EncoderOutput:
        """``.latent_dist``: the posterior of images ``x`` [B, in_channels, H, W] on a ROCm device (diffusers' call
        shape: ``vae.encode(x).latent_dist.sample()``)."""
        _, mom = self._encode(x, None, 1.0, True)
        return EncoderOutput(DiagonalGaussianDistribution(mom))

    def encode_to_latent(self, x: Tensor, scale: float = 1.0, noise: Tensor = None) -> Tensor:
        """``scale * z`` in one native call per micro-batch: z = mean + std * noise for a noise tensor [B,
        latent_channels, H / f, W / f] (torch.randn on the device), the posterior's mode without one; ``scale`` is
        rounded to float32 and multiplied on the device."""
        return self._encode(x, noise, scale, False)[0]

    def memory(self, device) -> Tuple[int, int]:
        """(weight bytes, workspace bytes) the decoder holds on `device` (dm_vae_decoder_memory)."""
        from dmhip._lib import check, load
        w, s = ctypes.c_int64(), ctypes.c_int64()
        check(load().dm_vae_decoder_memory(self.native_handle(device), ctypes.byref(w), ctypes.byref(s)),
              'dm_vae_decoder_memory')
        return w.value, s.value

    def close(self):
        handles, self._handles = getattr(self, '_handles', {}), {}
        if handles:
            from dmhip import _lib
            if _lib._lib is not None:
                for h in handles.values():
                    _lib._lib.dm_vae_decoder_destroy(h)
        handles, self._enc_handles = getattr(self, '_enc_handles', {}), {}
        if handles:
            from dmhip import _lib
            if _lib._lib is not None:
                for h in handles.values():
                    _lib._lib.dm_vae_encoder_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
