"""DDPM with explicit guidance (reference diffusions/guidance/base.py) on the engine.

The hooks and their order are the reference's: guidance on the predicted eps, the predicted x0, the mean of
p(x_{t-1} | x_t) and the sampled x_{t-1}, each with the reference's recomputation of the other quantities.
This generic path serves subclasses that override any hook; it is composed from dm_lincomb launches (the
closed-form conversions, separately rounded float32 products) and torch device ops. MaskGuidance and ILVR,
which act on the sample alone, run one fused step instead (dm_guided_step)."""
from typing import Dict, Optional

import torch
import tqdm
from torch import Tensor

import dmhip
from diffusions.ddpm import DDPM


class BaseGuidance(DDPM):
    def __init__(self, *args, **kwargs):
        """Denoising Diffusion Probabilistic Models with explicit guidance (Dhariwal & Nichol 2021)."""
        super().__init__(*args, **kwargs)

    # ------------------------------------------------- closed-form conversions
    def pred_mu_from_x0(self, xt: Tensor, t: int, t_prev: int, x0: Tensor):
        c = self._coefs(int(t), int(t_prev))
        return dmhip.lincomb(0, x0.contiguous(), xt.contiguous(), c['coef1'], c['coef2'])

    def pred_x0_from_mu(self, xt: Tensor, t: int, t_prev: int, mu: Tensor):
        c = self._coefs(int(t), int(t_prev))
        return dmhip.lincomb(3, mu.contiguous(), xt.contiguous(), c['coef2'], c['coef1'])

    # ------------------------------------------------------------------ hooks
    def cond_fn_eps(self, sample: Tensor, mean: Tensor, var: Tensor, pred_x0: Tensor, pred_eps: Tensor,
                    xt: Tensor, t: int, t_prev: int) -> Optional[Tensor]:
        """Apply guidance to predicted eps. """
        pass

    def cond_fn_x0(self, sample: Tensor, mean: Tensor, var: Tensor, pred_x0: Tensor, pred_eps: Tensor,
                   xt: Tensor, t: int, t_prev: int) -> Optional[Tensor]:
        """Apply guidance to predicted x0. """
        pass

    def cond_fn_mean(self, sample: Tensor, mean: Tensor, var: Tensor, pred_x0: Tensor, pred_eps: Tensor,
                     xt: Tensor, t: int, t_prev: int) -> Optional[Tensor]:
        """Apply guidance to mean of p(x{t-1} | xt). """
        pass

    def cond_fn_sample(self, sample: Tensor, mean: Tensor, var: Tensor, pred_x0: Tensor, pred_eps: Tensor,
                       xt: Tensor, t: int, t_prev: int) -> Optional[Tensor]:
        """Apply guidance to sampled x{t-1}. """
        pass

    def apply_guidance(self, sample: Tensor, mean: Tensor, var: Tensor, pred_x0: Tensor, pred_eps: Tensor,
                       reverse_eps: Tensor, xt: Tensor, t: int, t_prev: int):
        """Apply guidance to p_theta(x{t-1} | xt) (reference base.py:75-143, same order and recomputations)."""
        new_sample, new_mean, new_x0, new_eps = sample, mean, pred_x0, pred_eps
        kw = dict(sample=sample, mean=mean, var=var, pred_x0=pred_x0, pred_eps=pred_eps, xt=xt, t=t, t_prev=t_prev)

        def resample(mu):
            if t == 0 or reverse_eps is None:   # reverse_eps is None only where its factor is zero
                return mu
            return mu + torch.sqrt(var) * reverse_eps

        guidance = self.cond_fn_eps(**kw)
        if guidance is not None:
            new_eps = pred_eps + guidance
            new_x0 = self.pred_x0_from_eps(xt, t, new_eps)
            new_mean = self.pred_mu_from_x0(xt, t, t_prev, new_x0)
            new_sample = resample(new_mean)

        guidance = self.cond_fn_x0(**kw)
        if guidance is not None:
            new_x0 = pred_x0 + guidance
            new_eps = self.pred_eps_from_x0(xt, t, new_x0)
            new_mean = self.pred_mu_from_x0(xt, t, t_prev, new_x0)
            new_sample = resample(new_mean)

        guidance = self.cond_fn_mean(**kw)
        if guidance is not None:
            new_mean = mean + guidance
            new_x0 = self.pred_x0_from_mu(xt, t, t_prev, new_mean)
            new_eps = self.pred_eps_from_x0(xt, t, new_x0)
            new_sample = resample(new_mean)

        guidance = self.cond_fn_sample(**kw)
        if guidance is not None:
            new_sample = sample + guidance

        return {'sample': new_sample, 'mean': new_mean, 'var': var, 'pred_x0': new_x0, 'pred_eps': new_eps,
                'reverse_eps': reverse_eps}

    # ------------------------------------------------------------------ steps
    # The class whose cond_fn_sample the fused step implements (MaskGuidance / ILVR set it to themselves).
    _fused_owner = None

    def _fused(self) -> bool:
        """The fused step computes this object's guidance: no hook (nor apply_guidance) is overridden
        beyond the owner's own cond_fn_sample."""
        cls, own = type(self), self._fused_owner
        return (own is not None and cls.cond_fn_sample is own.cond_fn_sample
                and cls.apply_guidance is BaseGuidance.apply_guidance
                and all(getattr(cls, h) is getattr(BaseGuidance, h) for h in ('cond_fn_eps', 'cond_fn_x0',
                                                                              'cond_fn_mean')))

    def _guide_desc(self, xt: Tensor, t: int, t_prev: int):
        """(dmhip.GuideDesc, tensors to keep alive until the launch) of the fused step; may draw noise."""
        raise NotImplementedError

    def _known_coefs(self, t_prev: int, B: int):
        """sqrt(ac), sqrt(1 - ac) at t_prev as DDPM.diffuse computes them for a [B] timestep vector
        (t_prev == -1 indexes the last timestep, as the reference's tensor index does)."""
        key = ('known', t_prev, B)
        c = self._coef_cache.get(key)
        if c is None:
            a = self._ac_cpu[torch.full((B, ), t_prev, dtype=torch.long)]
            c = ((a ** 0.5)[0].item(), ((1. - a) ** 0.5)[0].item())
            self._coef_cache[key] = c
        return c

    def guided_denoise(self, model_output: Tensor, xt: Tensor, t: int, t_prev: int):
        """denoise() followed by apply_guidance(): one fused launch (two for ILVR beyond 64 x 64) where the
        guidance is the class's own cond_fn_sample, else the generic composition."""
        if self._fused():
            return self._step(model_output, xt, t, t_prev, guide=lambda: self._guide_desc(xt, t, t_prev))
        out = self.denoise(model_output, xt, t, t_prev)
        return self.apply_guidance(**out, xt=xt, t=t, t_prev=t_prev)

    def sample_loop(self, model, init_noise: Tensor, tqdm_kwargs: Dict = None, model_kwargs: Dict = None):
        tqdm_kwargs = dict() if tqdm_kwargs is None else tqdm_kwargs
        model_kwargs = dict() if model_kwargs is None else model_kwargs
        img = init_noise
        seq = self.respaced_seq.tolist()
        seq_prev = [-1] + seq[:-1]
        pbar = tqdm.tqdm(total=len(seq), **tqdm_kwargs)
        for t, t_prev in zip(reversed(seq), reversed(seq_prev)):
            t_batch = torch.full((img.shape[0], ), t, device=img.device, dtype=torch.long)
            model_output = model(img, t_batch, **model_kwargs)
            out = self.guided_denoise(model_output, img, t, t_prev)
            img = out['sample']
            pbar.update(1)
            yield out
        pbar.close()
