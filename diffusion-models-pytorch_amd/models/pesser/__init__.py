"""DDPM UNet of the official CelebA-HQ / LSUN checkpoints with the reference's module path (models.pesser.model.Model)."""
