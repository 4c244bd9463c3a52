"""MDTv2 (Masked Diffusion Transformer v2) on the MI355X engine.

Drop-in for the reference models/mdt/model.py:246-606 at inference: the same constructor (input_size, patch_size,
in_channels, hidden_size, depth, num_heads, mlp_ratio, class_dropout_prob, num_classes, learn_sigma, mask_ratio,
decode_layer), the MDTv2_* factories and the same state_dict names and shapes, buffers included
(``*.attn.rel_pos_bias.relative_position_index``), so MDT checkpoints load unchanged. ``forward(x, t, y,
enable_mask=False)``: y None (or, inside the CFG samplers' ``dmhip.null_label_scope()``, y[b] = -1) selects the
null class ``num_classes``; ``forward_with_cfg`` applies the reference's power-cosine guidance scale.

The modules are parameter containers; the forward pass is one dm_mdt_forward call (csrc/dit_exec.hip): DiT's token
path with the learned relative-position bias inside the flash attention kernel, the U-ViT long skips as one
K = 2 D GEMM each (the concat done by the operand pre-split pass), and the en_inblocks -> en_outblocks ->
+ decoder_pos_embed -> de_blocks topology. The side block and mask_token are loaded but never executed: they
serve the training-time masking only (``enable_mask=True`` raises NotImplementedError).

The kernels form the relative-position index arithmetically, (qy - ky + W - 1)(2W - 1) + (qx - kx + W - 1);
``load_state_dict`` compares a checkpoint's ``relative_position_index`` buffers with that formula and raises on a
mismatch.
"""
import ctypes
import math

import torch
import torch.nn as nn
from torch import Tensor

from dmhip._lib import MDTArch, check, load, stream_handle
from ..unet import NativeDenoiser
from ..dit.model import (FinalLayer, LabelEmbedder, Mlp, PatchEmbed, TimestepEmbedder, TokenMath,
                         get_2d_sincos_pos_embed)


def relative_position_index(W: int) -> Tensor:
    """The BEiT relative-position index of a W x W window (mdt/model.py:71-86) in closed form: entry [i, j] =
    (iy - jy + W - 1)(2W - 1) + (ix - jx + W - 1), int64 [W^2, W^2]."""
    p = torch.arange(W * W)
    py, px = p // W, p % W
    return (py[:, None] - py[None, :] + W - 1) * (2 * W - 1) + (px[:, None] - px[None, :] + W - 1)


def power_cosine_scale(t: Tensor, cfg_scale: float, diffusion_steps: int = 1000, scale_pow: float = 4.0) -> Tensor:
    """mdt/model.py:515-517: (cfg - 1) * (1 - cos(pi (1 - t / steps)^pow)) / 2 + 1, in the reference's operand order."""
    scale_step = (1 - torch.cos(((1 - t / diffusion_steps) ** scale_pow) * math.pi)) * 1 / 2
    return (cfg_scale - 1) * scale_step + 1


class RelativePositionBias(nn.Module):
    """mdt/model.py:61-99 parameters: the (2W - 1)^2 + 3 x heads table (the last 3 rows are BEiT's cls entries,
    never indexed) and the int64 index buffer."""

    def __init__(self, window_size, num_heads):
        super().__init__()
        self.window_size = window_size
        self.num_relative_distance = (2 * window_size[0] - 1) * (2 * window_size[1] - 1) + 3
        self.relative_position_bias_table = nn.Parameter(torch.zeros(self.num_relative_distance, num_heads))
        self.register_buffer('relative_position_index', relative_position_index(window_size[0]))


class Attention(nn.Module):
    """mdt/model.py:13-26 parameters: qkv Linear(D, 3D), proj Linear(D, D), rel_pos_bias."""

    def __init__(self, dim, num_heads=8, qkv_bias=True, num_patches=None):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        w = int(num_patches ** 0.5)
        self.rel_pos_bias = RelativePositionBias(window_size=[w, w], num_heads=num_heads)


class MDTBlock(nn.Module):
    """mdt/model.py:187-208 parameters (norm1 / norm2 have none); skip_linear Linear(2D, D) where skip."""

    def __init__(self, hidden_size, num_heads, mlp_ratio=4.0, skip=False, num_patches=None):
        super().__init__()
        self.attn = Attention(hidden_size, num_heads=num_heads, qkv_bias=True, num_patches=num_patches)
        self.mlp = Mlp(hidden_size, int(hidden_size * mlp_ratio))
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(hidden_size, 6 * hidden_size, bias=True))
        self.skip_linear = nn.Linear(2 * hidden_size, hidden_size) if skip else None


class MDTv2(TokenMath, NativeDenoiser):
    """Masked Diffusion Transformer v2 (mdt/model.py:246-526), inference path."""

    _abi = 'dm_mdt'

    def __init__(self, input_size=32, patch_size=2, in_channels=4, hidden_size=1152, depth=28, num_heads=16,
                 mlp_ratio=4.0, class_dropout_prob=0.1, num_classes=1000, learn_sigma=True, mask_ratio=None,
                 decode_layer=4):
        super().__init__()
        self.learn_sigma = learn_sigma
        self.in_channels = in_channels
        self.out_channels = in_channels * 2 if learn_sigma else in_channels
        self.patch_size = patch_size
        self.num_heads = num_heads
        self.num_classes = num_classes
        decode_layer = int(decode_layer)
        self.supports_null_label = class_dropout_prob > 0
        self.arch = dict(in_channels=in_channels, out_channels=self.out_channels, input_size=input_size,
                         patch_size=patch_size, hidden_size=hidden_size, depth=depth, num_heads=num_heads,
                         mlp_hidden=int(hidden_size * mlp_ratio), num_classes=num_classes,
                         null_class=class_dropout_prob > 0, learn_sigma=learn_sigma, decode_layer=decode_layer,
                         label_rows=num_classes + int(class_dropout_prob > 0))

        self.x_embedder = PatchEmbed(input_size, patch_size, in_channels, hidden_size, bias=True)
        self.t_embedder = TimestepEmbedder(hidden_size)
        self.y_embedder = LabelEmbedder(num_classes, hidden_size, class_dropout_prob)
        num_patches = self.x_embedder.num_patches
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches, hidden_size), requires_grad=False)

        half_depth = (depth - decode_layer) // 2
        self.half_depth = half_depth

        def block(skip=False):
            return MDTBlock(hidden_size, num_heads, mlp_ratio=mlp_ratio, num_patches=num_patches, skip=skip)

        self.en_inblocks = nn.ModuleList([block() for _ in range(half_depth)])
        self.en_outblocks = nn.ModuleList([block(skip=True) for _ in range(half_depth)])
        self.de_blocks = nn.ModuleList([block(skip=True) for _ in range(decode_layer)])
        self.sideblocks = nn.ModuleList([block() for _ in range(1)])
        self.final_layer = FinalLayer(hidden_size, patch_size, self.out_channels)

        self.decoder_pos_embed = nn.Parameter(torch.zeros(1, num_patches, hidden_size), requires_grad=False)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, hidden_size), requires_grad=False)
        self.mask_ratio = float(mask_ratio) if mask_ratio is not None else None
        self.decode_layer = decode_layer

        pos = torch.from_numpy(get_2d_sincos_pos_embed(hidden_size, int(num_patches ** 0.5))).float().unsqueeze(0)
        self.pos_embed.data.copy_(pos)
        self.decoder_pos_embed.data.copy_(pos)

    # ----------------------------------------------------------- native side
    def _arch_struct(self) -> MDTArch:
        a = MDTArch()
        for k in ('input_size', 'patch_size', 'in_channels', 'hidden_size', 'depth', 'num_heads', 'mlp_hidden',
                  'num_classes', 'decode_layer'):
            setattr(a, k, int(self.arch[k]))
        a.null_class = int(self.arch['null_class'])
        a.learn_sigma = int(self.arch['learn_sigma'])
        return a

    def native_param_names(self):
        """The state_dict keys the C ABI takes, in order: every float32 tensor; the int64 index buffers stay here."""
        return [k for k in self.state_dict().keys() if not k.endswith('relative_position_index')]

    def native_handle(self, device: torch.device):
        if getattr(self, '_param_list', None) is None:
            sd = self.state_dict(keep_vars=True)
            self._param_list = [v for k, v in sd.items() if not k.endswith('relative_position_index')]
        return super().native_handle(device)

    def native_param_count(self) -> int:
        n = ctypes.c_int()
        a = self._arch_struct()
        check(load().dm_mdt_param_count(ctypes.byref(a), ctypes.byref(n)), 'dm_mdt_param_count')
        return n.value

    def _time_freqs(self) -> Tensor:
        # mdt/model.py:131-135 (frequency_embedding_size 256, max_period 10000)
        half = 128
        return torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / half)

    def _launch(self, handle, X: Tensor, T: Tensor, y_ptr, out: Tensor):
        if X.shape[2] != self.arch['input_size'] or X.shape[3] != self.arch['input_size']:
            raise ValueError(f'expected {self.arch["input_size"]}x{self.arch["input_size"]} latents, '
                             f'got {tuple(X.shape)}')
        check(load().dm_mdt_forward(handle, X.data_ptr(), T.data_ptr(), y_ptr, X.shape[0], out.data_ptr(),
                                    stream_handle(X.device)), 'dm_mdt_forward')

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """As nn.Module.load_state_dict; first, every ``relative_position_index`` of the checkpoint must equal the
        arithmetic index the kernels use (ValueError otherwise)."""
        W = int(self.x_embedder.num_patches ** 0.5)
        want = relative_position_index(W)
        for k, v in state_dict.items():
            if k.endswith('relative_position_index'):
                v = torch.as_tensor(v)
                if tuple(v.shape) != tuple(want.shape) or not torch.equal(v.cpu().long(), want):
                    raise ValueError(f'{k}: the checkpoint\'s relative position index differs from '
                                     f'(qy - ky + W - 1)(2W - 1) + (qx - kx + W - 1), W = {W}, which the native '
                                     f'attention computes')
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    # --------------------------------------------------------------- forward
    def forward(self, x: Tensor, t: Tensor, y: Tensor = None, enable_mask: bool = False):
        """mdt/model.py:441-501 with enable_mask False. y None -> the null class (requires class_dropout_prob > 0)."""
        if enable_mask:
            raise NotImplementedError('MDTv2: enable_mask=True is the training-time masking (random token dropping '
                                      'and the side interpolater); the native engine runs inference only')
        if y is None and not self.arch['null_class']:
            raise IndexError('index out of range in self')  # nn.Embedding on label num_classes
        return self._run(x, t, y)

    def forward_with_cfg(self, x: Tensor, t: Tensor, y: Tensor, cfg_scale: float = None, diffusion_steps: int = 1000,
                         scale_pow: float = 4.0):
        """mdt/model.py:503-526: CFG on the first 3 channels with the power-cosine scale, both halves from one
        batched forward; cfg_scale None: the plain forward."""
        if cfg_scale is None:
            return self.forward(x, t, y)
        half = x[: len(x) // 2]
        combined = torch.cat([half, half], dim=0)
        model_out = self.forward(combined, t, y)
        eps, rest = model_out[:, :3], model_out[:, 3:]
        cond_eps, uncond_eps = torch.split(eps, len(eps) // 2, dim=0)
        real_cfg_scale = power_cosine_scale(t, cfg_scale, diffusion_steps, scale_pow)
        real_cfg_scale = real_cfg_scale[: len(x) // 2].view(-1, 1, 1, 1)
        half_eps = uncond_eps + real_cfg_scale * (cond_eps - uncond_eps)
        eps = torch.cat([half_eps, half_eps], dim=0)
        return torch.cat([eps, rest], dim=1)


def MDTv2_XL_2(**kwargs):
    return MDTv2(depth=28, hidden_size=1152, patch_size=2, num_heads=16, **kwargs)


def MDTv2_L_2(**kwargs):
    return MDTv2(depth=24, hidden_size=1024, patch_size=2, num_heads=16, **kwargs)


def MDTv2_B_2(**kwargs):
    return MDTv2(depth=12, hidden_size=768, patch_size=2, num_heads=12, **kwargs)


def MDTv2_S_2(**kwargs):
    return MDTv2(depth=12, hidden_size=384, patch_size=2, num_heads=6, **kwargs)
