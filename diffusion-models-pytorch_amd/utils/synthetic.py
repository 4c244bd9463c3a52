"""Deterministic synthetic weights.

No checkpoints are available offline, and the reference's own default init
makes some denoisers output exactly zero, so benchmarks and parity runs use
this rank-independent recipe over the reference state_dict keys, in order,
drawn from one numpy PCG64 stream (seed 0 by default):
  * tensors with ndim >= 2:   U(-1/sqrt(fan_in), +1/sqrt(fan_in)), fan_in = numel / shape[0]
  * 1-D '*.weight' (norms):   1
  * 1-D '*.bias':             U(-0.01, +0.01)
  * DiT 'pos_embed':          the fixed 2-D sin-cos table (dit/model.py:193-194), no draws
Each other tensor consumes numel float32 draws U[0,1) mapped to the range.
"""
import hashlib
from typing import Dict

import numpy as np
import torch


def _sincos_2d(embed_dim: int, grid_size: int) -> np.ndarray:
    """MAE / DiT fixed position table (dit/model.py:278-325), float64 [grid^2, embed_dim]."""
    def one_d(dim, pos):
        omega = np.arange(dim // 2, dtype=np.float64)
        omega /= dim / 2.
        omega = 1. / 10000 ** omega
        out = np.einsum('m,d->md', pos.reshape(-1), omega)
        return np.concatenate([np.sin(out), np.cos(out)], axis=1)
    gh = np.arange(grid_size, dtype=np.float32)
    gw = np.arange(grid_size, dtype=np.float32)
    grid = np.stack(np.meshgrid(gw, gh), axis=0).reshape([2, 1, grid_size, grid_size])
    return np.concatenate([one_d(embed_dim // 2, grid[0]), one_d(embed_dim // 2, grid[1])], axis=1)


def synthetic_state_dict(state_dict_like: Dict[str, torch.Tensor], seed: int = 0) -> Dict[str, torch.Tensor]:
    rng = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for name, ref in state_dict_like.items():
        shape = tuple(ref.shape)
        n = int(np.prod(shape)) if shape else 1
        if name == 'pos_embed' or name.endswith('.pos_embed'):
            grid = int(round(np.sqrt(shape[-2])))
            vals = _sincos_2d(shape[-1], grid).astype(np.float32)
        elif len(shape) >= 2:
            bound = 1.0 / np.sqrt(n / shape[0])
            u = rng.random(n, dtype=np.float32)
            vals = ((u * 2.0 - 1.0) * bound).astype(np.float32)
        elif name.endswith('weight'):
            vals = np.ones(n, dtype=np.float32)
        else:
            u = rng.random(n, dtype=np.float32)
            vals = ((u * 2.0 - 1.0) * 0.01).astype(np.float32)
        out[name] = torch.from_numpy(vals.reshape(shape))
    return out


def init_synthetic_(model: torch.nn.Module, seed: int = 0):
    """Load the synthetic weights into `model` in place; returns their sha256. An MDTv2 (a state_dict with
    ``relative_position_index`` buffers) takes synthetic_mdt_state_dict, the pesser DDPM UNet (``temb.dense.*`` keys)
    synthetic_pesser_state_dict."""
    ref = model.state_dict()
    if any(k.endswith('relative_position_index') for k in ref):
        sd = synthetic_mdt_state_dict(ref, seed)
    elif 'temb.dense.0.weight' in ref:
        sd = synthetic_pesser_state_dict(ref, seed)
    else:
        sd = synthetic_state_dict(ref, seed)
    model.load_state_dict(sd)
    return state_dict_sha256(sd)


def state_dict_sha256(sd: Dict[str, torch.Tensor]) -> str:
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def synthetic_mdt_state_dict(state_dict_like: Dict[str, torch.Tensor], seed: int = 0) -> Dict[str, torch.Tensor]:
    """Synthetic weights over an MDTv2 state_dict (models/mdt/model.py). The float tensors follow
    synthetic_state_dict (the int64 ``relative_position_index`` buffers are kept as they are and consume no draws);
    then the tensors that recipe would leave without influence are redrawn from a second PCG64 stream (seed + 1), in
    key order: every ``relative_position_bias_table`` ~ N(0, 1) (attention logits of synthetic weights are nearly
    flat, so a unit-scale bias decides the softmax), ``decoder_pos_embed`` ~ U(-1, 1) (the recipe's fan-in bound
    would make it 1e-2 of the tokens it is added to) and the blocks' ``adaLN_modulation.1.bias`` ~ U(-1, 1) (gates of
    order 1 instead of 1e-2: each block then changes the tokens enough that the long skips differ from one
    another, so their order matters)."""
    floats = {k: v for k, v in state_dict_like.items() if not k.endswith('relative_position_index')}
    syn = synthetic_state_dict(floats, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    out = {}
    for name, ref in state_dict_like.items():
        if name.endswith('relative_position_index'):
            out[name] = ref.detach().clone()
        elif name.endswith('relative_position_bias_table'):
            out[name] = torch.from_numpy(rng.standard_normal(tuple(ref.shape), dtype=np.float32))
        elif name == 'decoder_pos_embed' or (name.endswith('adaLN_modulation.1.bias') and 'blocks.' in name):
            out[name] = torch.from_numpy((rng.random(tuple(ref.shape), dtype=np.float32) * 2.0 - 1.0))
        else:
            out[name] = syn[name]
    return out


def synthetic_pesser_state_dict(state_dict_like: Dict[str, torch.Tensor], seed: int = 0) -> Dict[str, torch.Tensor]:
    """Synthetic weights over a pesser DDPM UNet state_dict (models/pesser/model.py): synthetic_state_dict, then from
    a second PCG64 stream (seed + 1), in key order: GroupNorm (``norm*``) weight ~ U(0.5, 1.5) and bias ~ U(-0.5, 0.5)
    (an affine that is not the identity, so a GroupNorm applied with the wrong statistics or eps shows), every other
    bias ~ U(-0.1, 0.1), and the attention blocks' ``q`` and ``k`` conv weights x 4 (consuming no draws): with the
    recipe's fan-in bound the scores are nearly flat and uniform attention would move the output by 0.03 only; x 4
    makes the softmax decide it (x 8 raises the reference's own float32 error to 1.6e-4)."""
    syn = synthetic_state_dict(state_dict_like, seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    out = {}
    for name, ref in state_dict_like.items():
        shape = tuple(ref.shape)
        mod, _, leaf = name.rpartition('.')
        is_norm = mod.rpartition('.')[2].startswith('norm')
        if len(shape) == 1 and is_norm:
            u = rng.random(shape, dtype=np.float32)
            out[name] = torch.from_numpy(u + np.float32(0.5) if leaf == 'weight' else u - np.float32(0.5))
        elif len(shape) == 1 and leaf == 'bias':
            u = rng.random(shape, dtype=np.float32)
            out[name] = torch.from_numpy((u * np.float32(2.0) - np.float32(1.0)) * np.float32(0.1))
        elif leaf == 'weight' and mod.rpartition('.')[2] in ('q', 'k'):
            out[name] = syn[name] * 4.0
        else:
            out[name] = syn[name]
    return out
