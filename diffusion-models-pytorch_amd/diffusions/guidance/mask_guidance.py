"""Mask guidance / RePaint (reference diffusions/guidance/mask_guidance.py) on the engine."""
from typing import Dict

import torch
import tqdm
from torch import Tensor

import dmhip
from diffusions.guidance.base import BaseGuidance


class MaskGuidance(BaseGuidance):
    def __init__(self, masked_image: Tensor = None, mask: Tensor = None, *args, **kwargs):
        """Diffusion models with mask guidance (Song & Ermon 2019; Avrahami et al. 2022; RePaint, Lugmayr et
        al. 2022): in each reverse step x_{t-1} = m * x^known_{t-1} + (1 - m) * x^unknown_{t-1}.

        Args:
            masked_image: The masked input images of shape [B, C, H, W].
            mask: The masks of shape [B, 1, H, W] or [B, C, H, W] (float; 1 denotes known areas, 0 unknown).
        """
        super().__init__(*args, **kwargs)
        self.masked_image = masked_image
        self.mask = mask

    def set_mask_and_image(self, masked_image: Tensor, mask: Tensor):
        self.masked_image = masked_image
        self.mask = mask

    def _require_inputs(self):
        if self.masked_image is None or self.mask is None:
            raise RuntimeError('Please call `set_mask_and_image()` before sampling.')

    def cond_fn_sample(self, t: int, t_prev: int, sample: Tensor, **kwargs):
        """(noisy_known - sample) * mask; the known part is left un-noised when t == 0 (the reference's
        condition, not t_prev == -1)."""
        self._require_inputs()
        known = self.masked_image.to(sample.device)
        if t == 0:
            noisy_known = known
        else:
            noisy_known = self.diffuse(x0=known, t=torch.full((sample.shape[0], ), t_prev, dtype=torch.long),
                                       eps=self._draw_noise(known, True))
        return (noisy_known - sample) * self.mask.to(sample.device)

    def _guide_desc(self, xt: Tensor, t: int, t_prev: int):
        self._require_inputs()
        dev = dict(device=xt.device, dtype=torch.float32)
        known = self.masked_image.to(**dev).contiguous()
        mask = self.mask.to(**dev).contiguous()
        B, C = xt.shape[0], xt.shape[1]
        if known.shape != xt.shape:
            raise ValueError(f'masked_image {tuple(known.shape)} does not match the samples {tuple(xt.shape)}')
        if mask.ndim != xt.ndim or mask.shape[0] != B or mask.shape[1] not in (1, C) or mask.shape[2:] != xt.shape[2:]:
            raise ValueError(f'mask must have shape [B, 1, H, W] or [B, C, H, W], got {tuple(mask.shape)}')
        g = dmhip.GuideDesc()
        g.kind = 1
        g.known = known.data_ptr()
        g.mask, g.mask_channels = mask.data_ptr(), mask.shape[1]
        eps = None
        if t != 0:
            eps = self._draw_noise(known, True)
            g.noise_known, g.noise_known_eps = 1, eps.data_ptr()
            g.sqrt_ac_prev, g.sqrt_one_minus_ac_prev = self._known_coefs(t_prev, B)
        return g, (known, mask, eps)

    def q_sample_one_step(self, xt: Tensor, t: int, t_next: int):
        """Sample from q(x{t+1} | xt) (reference mask_guidance.py:64-69; coefficients from the host's 0-dim ops)."""
        key = ('qstep', t, t_next)
        c = self._coef_cache.get(key)
        if c is None:
            ac_t = self._ac(t)
            ac_n = self._ac(t_next) if t_next < self.total_steps else torch.tensor(0.0)
            a = ac_n / ac_t
            c = (torch.sqrt(a).item(), torch.sqrt(1. - a).item())
            self._coef_cache[key] = c
        return dmhip.lincomb(0, xt.contiguous(), self._draw_noise(xt, True), c[0], c[1])

    def resample_loop(self, model, init_noise: Tensor, resample_r: int = 10, resample_j: int = 10,
                      tqdm_kwargs: Dict = None, model_kwargs: Dict = None):
        """Sample following RePaint paper. """
        tqdm_kwargs = dict() if tqdm_kwargs is None else tqdm_kwargs
        model_kwargs = dict() if model_kwargs is None else model_kwargs
        img = init_noise
        seq1 = self.get_resample_seq(resample_r, resample_j)
        seq2 = seq1[1:] + [-1]
        pbar = tqdm.tqdm(total=len(seq1), **tqdm_kwargs)
        for t1, t2 in zip(seq1, seq2):
            if t1 > t2:
                t_batch = torch.full((img.shape[0], ), t1, device=img.device, dtype=torch.long)
                model_output = model(img, t_batch, **model_kwargs)
                out = self.guided_denoise(model_output, img, t1, t2)
                img = out['sample']
                yield out
            else:
                img = self.q_sample_one_step(img, t1, t2)
                yield {'sample': img}
            pbar.update(1)
        pbar.close()

    def resample(self, model, init_noise: Tensor, resample_r: int = 10, resample_j: int = 10,
                 tqdm_kwargs: Dict = None, model_kwargs: Dict = None):
        def run():
            sample = None
            for out in self.resample_loop(model, init_noise, resample_r, resample_j, tqdm_kwargs, model_kwargs):
                sample = out['sample']
            return sample
        return self._range_guarded(run, init_noise)

    def get_resample_seq(self, resample_r: int = 10, resample_j: int = 10):
        """Figure 9 in RePaint paper.

        Args:
            resample_r: Number of resampling, as proposed in RePaint paper.
            resample_j: Jump lengths of resampling, as proposed in RePaint paper.
        """
        seq = self.respaced_seq.tolist()
        t_T = len(seq)
        jumps = {j: resample_r - 1 for j in range(0, t_T - resample_j, resample_j)}
        t = t_T
        ts = []
        while t >= 1:
            t = t - 1
            ts.append(seq[t])
            if jumps.get(t, 0) > 0:
                jumps[t] = jumps[t] - 1
                for _ in range(resample_j):
                    t = t + 1
                    ts.append(seq[t])
        return ts


MaskGuidance._fused_owner = MaskGuidance
