"""MDTv2 denoiser with the reference's module paths (models.mdt.model.MDTv2, models.mdt.mdt.MDT)."""
