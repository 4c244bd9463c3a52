"""The DDPM UNet of the official CelebA-HQ 256 / LSUN 256 checkpoints (pesser's pytorch_diffusion port) on the
MI355X engine.

Drop-in for the reference models/pesser/model.py:190-327 at inference: the same constructor (ch, out_ch, ch_mult,
num_res_blocks, attn_resolutions, dropout, resamp_with_conv, in_channels, resolution) and the same state_dict names
and shapes (``down.4.attn.1.q.weight [512, 512, 1, 1]``, ``up.0.block.2.nin_shortcut.weight``, ...), so the
converted checkpoints load unchanged. ``forward(x [B, C, R, R] f32, t [B] int64) -> [B, out_ch, R, R]`` with
R = ``resolution`` (any other size raises, as the reference's assert does).

The modules are parameter containers; the forward pass is one dm_unet_forward call on variant 3 of the UNet
executor (csrc/unet_exec.hip), which differs from models/unet.py's variant 0 in four things: GroupNorm eps 1e-6,
a Downsample that pads the bottom and right only before its stride-2 conv, one attention head of C channels
after every ResnetBlock of a listed resolution, and the registration order (a level's blocks, then its attention
blocks, then its resample conv; ``up`` stored by level and run from the deepest), which the executor maps onto
its own walk. ``resamp_with_conv=False`` (pooling / nearest resampling without convs) is used by no shipped config
and raises NotImplementedError; ``conv_shortcut`` is never set by the reference's Model.
"""
from typing import Sequence

import torch.nn as nn
from torch import Tensor

from ..unet import ConvHalf, NativeDenoiser


def _gn(C: int) -> nn.GroupNorm:
    return nn.GroupNorm(32, C, eps=1e-6)


def _conv(cin: int, cout: int, k: int, stride: int = 1, padding: int = None) -> nn.Conv2d:
    return nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2 if padding is None else padding)


def _holder(**children) -> nn.Module:
    """A bare module whose children are registered under the given names, in the given order (the checkpoints'
    ``temb.*``, ``mid.*`` and per-level ``down.N.*`` / ``up.N.*`` prefixes)."""
    m = nn.Module()
    for name, child in children.items():
        m.add_module(name, child)
    return m


class ResnetBlock(nn.Module):
    """Parameters of a residual block under the checkpoint's names: norm1, conv1, temb_proj, norm2, conv2 and, where
    the width changes, the 1x1 nin_shortcut."""

    def __init__(self, cin: int, cout: int, embed_dim: int):
        super().__init__()
        self.norm1 = _gn(cin)
        self.conv1 = _conv(cin, cout, 3)
        self.temb_proj = nn.Linear(embed_dim, cout)
        self.norm2 = _gn(cout)
        self.conv2 = _conv(cout, cout, 3)
        if cin != cout:
            self.nin_shortcut = _conv(cin, cout, 1)


class AttnBlock(nn.Module):
    """Parameters of a single-head attention block: norm and the 1x1 convs q, k, v, proj_out."""

    def __init__(self, C: int):
        super().__init__()
        self.norm = _gn(C)
        for name in ('q', 'k', 'v', 'proj_out'):
            self.add_module(name, _conv(C, C, 1))


class Resample(nn.Module):
    """The 3x3 conv of a Downsample (stride 2 over the bottom/right-padded map, no padding of its own) or of an
    Upsample (stride 1 after the nearest 2x), under the name ``conv``."""

    def __init__(self, C: int, down: bool):
        super().__init__()
        self.conv = _conv(C, C, 3, stride=2, padding=0) if down else _conv(C, C, 3)


class Model(ConvHalf, NativeDenoiser):
    def __init__(self, *, ch: int, out_ch: int, ch_mult: Sequence[int] = (1, 2, 4, 8), num_res_blocks: int,
                 attn_resolutions: Sequence[int], dropout: float = 0.0, resamp_with_conv: bool = True,
                 in_channels: int, resolution: int):
        super().__init__()
        if not resamp_with_conv:
            raise NotImplementedError('resamp_with_conv=False (average-pool / nearest resampling without convs) is '
                                      'used by no shipped config and is not built')
        self.ch = ch
        self.resolution = resolution
        self.in_channels = in_channels
        listed = {int(r) for r in attn_resolutions}
        widths = [ch * int(m) for m in ch_mult]
        n_levels = len(widths)
        use_attn = [(resolution >> lvl) in listed for lvl in range(n_levels)]   # level lvl runs at resolution >> lvl
        self.arch = dict(in_channels=in_channels, out_channels=out_ch, dim=ch, dim_mults=[int(m) for m in ch_mult],
                         use_attn=use_attn, num_res_blocks=num_res_blocks, n_heads=1, variant=3)
        embed = 4 * ch

        def stage(lvl, cins, resample):
            """One level's holder: its blocks (input widths `cins`), then its attention blocks, then its resample
            conv -- the checkpoint's registration order (the executor's walk interleaves them, walk_order())."""
            w = widths[lvl]
            parts = dict(block=nn.ModuleList(ResnetBlock(c, w, embed) for c in cins),
                         attn=nn.ModuleList(AttnBlock(w) for _ in cins if use_attn[lvl]))
            parts.update(resample)
            return _holder(**parts)

        self.temb = _holder(dense=nn.ModuleList([nn.Linear(ch, embed), nn.Linear(embed, embed)]))
        self.conv_in = _conv(in_channels, ch, 3)

        # down path; `skips` holds the width of every tensor the up path will concatenate, in push order
        skips, cur = [ch], ch
        self.down = nn.ModuleList()
        for lvl, w in enumerate(widths):
            last = lvl == n_levels - 1
            self.down.append(stage(lvl, [cur] + [w] * (num_res_blocks - 1),
                                   {} if last else dict(downsample=Resample(w, down=True))))
            skips += [w] * (num_res_blocks + (0 if last else 1))
            cur = w

        self.mid = _holder(block_1=ResnetBlock(cur, cur, embed), attn_1=AttnBlock(cur),
                           block_2=ResnetBlock(cur, cur, embed))

        # up path: built from the deepest level (each block pops one skip), stored by level index
        ups = {}
        for lvl in reversed(range(n_levels)):
            cins = []
            for _ in range(num_res_blocks + 1):
                cins.append(cur + skips.pop())
                cur = widths[lvl]
            ups[lvl] = stage(lvl, cins, dict(upsample=Resample(cur, down=False)) if lvl else {})
        assert not skips
        self.up = nn.ModuleList(ups[lvl] for lvl in range(n_levels))

        self.norm_out = _gn(cur)
        self.conv_out = _conv(cur, out_ch, 3)

    def forward(self, x: Tensor, t: Tensor):
        """x [B, C, R, R] f32, t [B] int64 -> [B, out_ch, R, R]; any other spatial size is an AssertionError, as in
        the reference (pesser/model.py:288)."""
        if tuple(x.shape[2:]) != (self.resolution, self.resolution):
            raise AssertionError(f'expected {self.resolution} x {self.resolution} images, got {tuple(x.shape[2:])}')
        return self._run(x, t)
