"""Latent DiT wrapper (models/dit/dit.py:10-36, models/base_latent.py:6-28).

Same constructor (vae_config, vit_config, scale_factor) and forward
(x, timesteps, y=None) -> vit(x, timesteps, y); state_dict loads go to the
transformer, as upstream. The VAE (``models.dit.autoencoder.AutoEncoderKL``:
the native latent decoder, built from a local checkpoint directory; a hub id
raises NotImplementedError) is outside the denoising hot path, so it is
instantiated lazily, only when ``decode_latent`` or ``encode_latent`` is
called.
"""
from typing import Any, Mapping

import torch
from torch import Tensor

from utils.misc import instantiate_from_config
from ..base_latent import BaseLatent


class DiT(BaseLatent):
    def __init__(self, vae_config, vit_config, scale_factor: float = 0.18215):
        super().__init__(scale_factor=scale_factor)
        self.vae_config = vae_config
        self.vae = None
        self.vit = instantiate_from_config(vit_config)

    @property
    def supports_null_label(self):
        return getattr(self.vit, 'supports_null_label', False)

    def _vae(self):
        if self.vae is None:
            self.vae = instantiate_from_config(self.vae_config)
        return self.vae

    def encode_latent(self, x: Tensor, sample_posterior: bool = True, generator=None):
        """``scale_factor * z`` of images ``x`` (reference models/stablediffusion/stablediffusion.py:29-38): z a sample
        of the VAE posterior (noise from torch.randn with `generator`), or its mode with sample_posterior=False.
        scale_factor is the float32 buffer's value, multiplied on the device by the native posterior kernel."""
        vae = self._vae()
        noise = None
        if sample_posterior:
            f = vae.upscale
            shape = (x.shape[0], vae.arch['z_channels'], x.shape[2] // f, x.shape[3] // f)
            gdev = generator.device if generator is not None else x.device
            noise = torch.randn(shape, generator=generator, device=gdev, dtype=torch.float32).to(x.device)
        return vae.encode_to_latent(x, scale=float(self.scale_factor), noise=noise)

    def decode_latent(self, z: Tensor):
        self._vae()
        z = 1. / self.scale_factor * z
        return self.vae.decode(z).sample

    def set_math(self, kind: str) -> str:
        """The arithmetic of the transformer's token GEMMs ('fp16x2', 'fp32' or the half-precision 'fp16':
        ``models.dit.model.TokenMath.set_math``). The VAE keeps its own arithmetic."""
        return self.vit.set_math(kind)

    def vit_forward(self, x: Tensor, t: Tensor, y: Tensor):
        return self.vit(x, t, y)

    def forward(self, x: Tensor, timesteps: Tensor, y: Tensor = None):
        return self.vit_forward(x, timesteps, y)

    def load_state_dict(self, state_dict: Mapping[str, Any], strict: bool = True, assign: bool = False):
        return self.vit.load_state_dict(state_dict, strict=strict, assign=assign)
