"""Explicit guidance on the engine (reference diffusions/guidance/): BaseGuidance, MaskGuidance (inpainting,
RePaint resampling) and ILVR. CLIP guidance needs a CLIP network and autograd and is not provided."""
from diffusions.guidance.base import BaseGuidance  # noqa: F401
from diffusions.guidance.mask_guidance import MaskGuidance  # noqa: F401
from diffusions.guidance.ilvr import ILVR  # noqa: F401
