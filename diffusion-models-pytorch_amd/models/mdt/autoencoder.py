"""models/mdt/autoencoder.py: the KL autoencoder the reference's MDT wraps -- the same one as DiT's, so the native
``AutoEncoderKL`` of models/dit/autoencoder.py under the module path the reference's MDT configs name."""
from ..dit.autoencoder import AutoEncoderKL, DecoderOutput, DiagonalGaussianDistribution  # noqa: F401
