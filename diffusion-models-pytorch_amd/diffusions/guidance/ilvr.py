"""Iterative Latent Variable Refinement (reference diffusions/guidance/ilvr.py) on the engine."""
import torch
from torch import Tensor

import dmhip
from diffusions.guidance import lowpass
from diffusions.guidance.base import BaseGuidance


class ILVR(BaseGuidance):
    def __init__(self, ref_images: Tensor = None, downsample_factor: int = 8, interp_method: str = 'cubic',
                 *args, **kwargs):
        """ILVR (Choi et al. 2021): x_{t-1} + phi(noisy reference) - phi(x_{t-1}) with phi a low-pass filter
        (down- then upsampling by `downsample_factor`).

        Args:
            ref_images: The reference images of shape [B, C, H, W].
            downsample_factor: The downsample factor; it must divide H and W.
            interp_method: The interpolation method. Options: 'cubic', 'lanczos2', 'lanczos3', 'linear', 'box'.
        """
        super().__init__(*args, **kwargs)
        if interp_method not in lowpass.INTERP_METHODS:
            raise ValueError(f'Invalid interp_method: {interp_method} (options: {sorted(lowpass.INTERP_METHODS)})')
        self.ref_images = ref_images
        self.downsample_factor = int(downsample_factor)
        self.interp_method = interp_method
        self._plans = {}

    def set_ref_images(self, ref_images: Tensor):
        self.ref_images = ref_images

    def _plan(self, x: Tensor) -> dmhip.LowpassPlan:
        """The device plan for x's planes (host tables cached per shape, plans per shape and device)."""
        if x.ndim < 2:
            raise ValueError('low_pass_filter expects [..., H, W]')
        H, W = int(x.shape[-2]), int(x.shape[-1])
        key = (H, W, x.device)
        plan = self._plans.get(key)
        if plan is None:
            tables = lowpass.axis_tables(H, W, self.downsample_factor, self.interp_method)
            plan = dmhip.LowpassPlan(H, W, self.downsample_factor, tables, x.device)
            self._plans[key] = plan
        return plan

    def low_pass_filter(self, x: Tensor):
        """resize(resize(x, 1 / N), N) over the last two dims (reference ilvr.py:48-52); N must divide both."""
        plan = self._plan(x)
        dmhip.require_device_tensor(x.contiguous(), 'x')
        return plan.apply(x.contiguous())

    def cond_fn_sample(self, t: int, t_prev: int, sample: Tensor, **kwargs):
        if self.ref_images is None:
            raise RuntimeError('Please call `set_ref_images()` before sampling.')
        ref = self.ref_images.to(sample.device)
        if t == 0:
            noisy_ref = ref
        else:
            noisy_ref = self.diffuse(x0=ref, t=torch.full((sample.shape[0], ), t_prev, dtype=torch.long),
                                     eps=self._draw_noise(ref, True))
        return self.low_pass_filter(noisy_ref) - self.low_pass_filter(sample)

    def _guide_desc(self, xt: Tensor, t: int, t_prev: int):
        if self.ref_images is None:
            raise RuntimeError('Please call `set_ref_images()` before sampling.')
        if xt.ndim != 4:
            raise ValueError('ILVR expects images of shape [B, C, H, W]')
        ref = self.ref_images.to(device=xt.device, dtype=torch.float32).contiguous()
        if ref.shape != xt.shape:
            raise ValueError(f'ref_images {tuple(ref.shape)} do not match the samples {tuple(xt.shape)}')
        plan = self._plan(xt)
        scratch = plan.scratch(xt.shape[0] * xt.shape[1])
        g = dmhip.GuideDesc()
        g.kind = 2
        g.known = ref.data_ptr()
        g.lowpass = plan.handle.value
        g.scratch = scratch.data_ptr() if scratch is not None else None
        eps = None
        if t != 0:
            eps = self._draw_noise(ref, True)
            g.noise_known, g.noise_known_eps = 1, eps.data_ptr()
            g.sqrt_ac_prev, g.sqrt_one_minus_ac_prev = self._known_coefs(t_prev, xt.shape[0])
        return g, (ref, scratch, eps, plan)


ILVR._fused_owner = ILVR
