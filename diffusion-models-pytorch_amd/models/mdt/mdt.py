"""Latent MDT wrapper (models/mdt/mdt.py:10-36): the constructor (vae_config, vit_config, scale_factor), forward and
load_state_dict of the reference, with models/dit/dit.py's lazy VAE, ``encode_latent`` and ``decode_latent``."""
from ..dit.dit import DiT as _LatentDiT


class MDT(_LatentDiT):
    pass
