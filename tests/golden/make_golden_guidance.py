"""Golden fixtures of the guided samplers, generated from the REFERENCE (diffusions/guidance/, utils/resize_right).

Runs only where the reference checkout exists (make_golden.REF):
    python tests/golden/make_golden_guidance.py
Like make_golden.py it imports the reference through a bare `diffusions` package shim; `diffusions.guidance` is
shimmed as a bare package too, so clip_guidance.py (CLIP, transformers) is never imported. Writes
tests/golden/guidance.npz / guidance.json:

  * seq_<steps>_<r>_<j>        MaskGuidance.get_resample_seq
  * mat_<dir>_<size>_<N>_<m>   dense per-axis matrices of resize_right.resize (the resize of an identity)
  * lp_<H>_<W>_<N>_<m>_{x,y}   ILVR.low_pass_filter inputs / outputs
  * mstep<i>_*, istep_*, toy_* single guided steps (MaskGuidance, ILVR, a toy BaseGuidance subclass) with both
                               noises recorded (noise0: reverse_eps, noise1: the diffusion of the known image)
  * traj_<name>_*              trajectories on the tiny UNet with every noise draw recorded, and the drift of the
                               reference's own fp32 run from its float64 run per step (asserted <= 5e-5 here, so
                               the tests' flat 1e-4 bound measures the engine and not chaos)
"""
import os
import sys
import types
from contextlib import contextmanager

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
from make_golden_r2 import Float64Reference  # noqa: E402

REF = mg.REF
DRIFT_BOUND = 5e-5

LP_CASES = [(16, 16, 2, 'cubic'), (32, 32, 8, 'cubic'), (32, 32, 4, 'lanczos3'), (64, 32, 4, 'linear'),
            (32, 32, 4, 'box'), (64, 64, 16, 'lanczos2')]
MAT_EXTRA = [(256, 8, 'cubic')]
SEQ_CASES = [(4, 2, 2), (20, 2, 5), (10, 1, 3), (10, 3, 2), (50, 10, 10)]
TOY_SCALES = dict(eps=0.05, x0=-0.1, mean=0.02)


def import_guidance():
    schedule, ddpm, ddim, unet = mg.import_reference()
    pkg = types.ModuleType('diffusions.guidance')
    pkg.__path__ = [os.path.join(REF, 'diffusions', 'guidance')]
    sys.modules['diffusions.guidance'] = pkg
    import diffusions.guidance.base as base  # noqa: E402
    import diffusions.guidance.mask_guidance as mask_guidance  # noqa: E402
    import diffusions.guidance.ilvr as ilvr  # noqa: E402
    from utils.resize_right import resize_right, interp_methods  # noqa: E402
    return base, mask_guidance, ilvr, resize_right, interp_methods, unet


class Recorder:
    """randn_like replacement drawing from a seeded CPU generator and keeping every draw in order."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.draws = []

    def __call__(self, x):
        n = torch.randn(x.shape, generator=self.g)
        self.draws.append(n)
        return n.to(x.dtype)


class Replayer:
    def __init__(self, draws):
        self.draws, self.k = draws, 0

    def __call__(self, x):
        n = self.draws[self.k]
        self.k += 1
        assert n.shape == x.shape
        return n.to(x.dtype)


@contextmanager
def patched_randn_like(source):
    orig = torch.randn_like
    torch.randn_like = lambda x, *a, **k: source(x)
    try:
        yield
    finally:
        torch.randn_like = orig


def make_toy(base):
    class ToyGuidance(base.BaseGuidance):
        """cond_fn_eps / x0 / mean return fixed multiples of a stored tensor (the tests define the same class on
        the engine's BaseGuidance)."""

        def __init__(self, g, *a, **k):
            super().__init__(*a, **k)
            self.g = g

        def cond_fn_eps(self, **kw):
            return TOY_SCALES['eps'] * self.g

        def cond_fn_x0(self, **kw):
            return TOY_SCALES['x0'] * self.g

        def cond_fn_mean(self, **kw):
            return TOY_SCALES['mean'] * self.g
    return ToyGuidance


def main():
    torch.set_num_threads(8)
    base, mgd, ilvr, resize_right, interp_methods, unet = import_guidance()
    meta = dict(torch=torch.__version__, threads=torch.get_num_threads(), coef_probe_sha=mg.coef_probe_sha(),
                reference='xyfJASON/diffusion-models-pytorch @ 2024-12-20',
                lp_cases=[list(c) for c in LP_CASES], seq_cases=[list(c) for c in SEQ_CASES],
                toy_scales=TOY_SCALES, drift_bound=DRIFT_BOUND)
    arr = {}

    # 1. RePaint resample sequences
    for steps, r, j in SEQ_CASES:
        d = mgd.MaskGuidance(respace_type='uniform', respace_steps=steps)
        arr[f'seq_{steps}_{r}_{j}'] = np.asarray(d.get_resample_seq(r, j), dtype=np.int64)

    # 2. dense per-axis matrices: the reference resize of an identity along one axis
    mats = sorted({(s, n, m) for (h, w, n, m) in LP_CASES for s in (h, w)} | set(MAT_EXTRA))
    for size, n, m in mats:
        method = getattr(interp_methods, m)
        eye = torch.eye(size)[None, None]
        arr[f'mat_down_{size}_{n}_{m}'] = resize_right.resize(eye, scale_factors=[1. / n, 1.],
                                                              interp_method=method)[0, 0]       # [size / n, size]
        eye = torch.eye(size // n)[None, None]
        arr[f'mat_up_{size}_{n}_{m}'] = resize_right.resize(eye, scale_factors=[n, 1.], interp_method=method)[0, 0]
    meta['mats'] = [list(c) for c in mats]

    # 3. low_pass_filter at the small shapes
    g = torch.Generator().manual_seed(41)
    for h, w, n, m in LP_CASES:
        d = ilvr.ILVR(downsample_factor=n, interp_method=m)
        x = torch.randn((1, 2, h, w), generator=g)
        arr[f'lp_{h}_{w}_{n}_{m}_x'] = x
        arr[f'lp_{h}_{w}_{n}_{m}_y'] = d.low_pass_filter(x)

    # 4. single guided steps: denoise + apply_guidance with both noises recorded
    def one_step(d, mo, xt, t, tp, seed):
        rec = Recorder(seed)
        with patched_randn_like(rec):
            out = d.denoise(mo, xt, t, tp)
            unguided = out['sample']
            out = d.apply_guidance(**out, xt=xt, t=t, t_prev=tp)
        return out, unguided, rec.draws

    mask_cases = [
        dict(shape=(2, 3, 16, 16), mask_c=1, binary=True, t=999, tp=899, var_type='fixed_large'),
        dict(shape=(3, 1, 5, 7), mask_c=1, binary=True, t=100, tp=0, var_type='fixed_small'),
        dict(shape=(2, 3, 16, 16), mask_c=3, binary=True, t=0, tp=-1, var_type='fixed_large'),
        dict(shape=(3, 1, 5, 7), mask_c=1, binary=False, t=999, tp=899, var_type='fixed_large'),
        dict(shape=(2, 3, 16, 16), mask_c=1, binary=False, t=100, tp=0, var_type='learned_range'),
    ]
    meta['mask_cases'] = mask_cases
    for i, c in enumerate(mask_cases):
        B, C, H, W = c['shape']
        learned = c['var_type'] == 'learned_range'
        xt = torch.randn(c['shape'], generator=g) * 1.2
        mo = torch.randn((B, 2 * C if learned else C, H, W), generator=g)
        if learned:
            mo[:, C:] = mo[:, C:].clamp(-1, 1)
        img = torch.rand(c['shape'], generator=g) * 2 - 1
        mask = torch.rand((B, c['mask_c'], H, W), generator=g)
        mask = (mask > 0.4).float() if c['binary'] else mask * 1.5 - 0.25
        d = mgd.MaskGuidance(var_type=c['var_type'])
        d.set_mask_and_image(img * mask, mask)
        out, unguided, draws = one_step(d, mo, xt, c['t'], c['tp'], 100 + i)
        arr[f'mstep{i}_xt'], arr[f'mstep{i}_out'] = xt, mo
        arr[f'mstep{i}_masked'], arr[f'mstep{i}_mask'] = img * mask, mask
        for k, n in enumerate(draws):
            arr[f'mstep{i}_noise{k}'] = n
        for k in ('sample', 'mean', 'pred_x0', 'pred_eps'):
            arr[f'mstep{i}_{k}'] = out[k]
        arr[f'mstep{i}_unguided'] = unguided

    ilvr_steps = [dict(shape=(2, 3, 32, 32), N=8, method='cubic', t=500, tp=400),
                  dict(shape=(2, 3, 16, 16), N=4, method='lanczos2', t=0, tp=-1)]
    meta['ilvr_steps'] = ilvr_steps
    for i, c in enumerate(ilvr_steps):
        xt = torch.randn(c['shape'], generator=g)
        mo = torch.randn(c['shape'], generator=g)
        ref = torch.rand(c['shape'], generator=g) * 2 - 1
        d = ilvr.ILVR(ref_images=ref, downsample_factor=c['N'], interp_method=c['method'])
        out, unguided, draws = one_step(d, mo, xt, c['t'], c['tp'], 200 + i)
        arr[f'istep{i}_xt'], arr[f'istep{i}_out'], arr[f'istep{i}_ref'] = xt, mo, ref
        for k, n in enumerate(draws):
            arr[f'istep{i}_noise{k}'] = n
        arr[f'istep{i}_sample'] = out['sample']

    toy_steps = [(700, 600), (0, -1)]
    meta['toy_steps'] = toy_steps
    Toy = make_toy(base)
    for i, (t, tp) in enumerate(toy_steps):
        shape = (2, 3, 8, 8)
        xt = torch.randn(shape, generator=g)
        mo = torch.randn(shape, generator=g)
        gt = torch.randn(shape, generator=g)
        d = Toy(gt, var_type='fixed_small')
        out, _, draws = one_step(d, mo, xt, t, tp, 300 + i)
        arr[f'toy{i}_xt'], arr[f'toy{i}_out'], arr[f'toy{i}_g'] = xt, mo, gt
        arr[f'toy{i}_noise0'] = draws[0]
        for k in ('sample', 'mean', 'pred_x0', 'pred_eps'):
            arr[f'toy{i}_{k}'] = out[k]

    # 5. trajectories on the tiny UNet (16 x 16, the synthetic weights forward.json names)
    model = unet.UNet(**mg.ARCHS['tiny']).eval()
    meta['tiny_weights_sha256'] = mg.synthetic(model)
    model64 = Float64Reference(model)
    shape = (2, 3, 16, 16)
    img = torch.rand(shape, generator=g) * 2 - 1
    mask = torch.zeros((2, 1, 16, 16))
    mask[0, :, :, :9] = 1
    mask[1, :, 4:12, 4:12] = 1
    arr['traj_image'], arr['traj_mask'] = img, mask

    trajs = {
        'mask5': dict(make=lambda: mgd.MaskGuidance(respace_type='uniform', respace_steps=5),
                      loop=lambda d, m, x: d.sample_loop(m, x, tqdm_kwargs=dict(disable=True))),
        'repaint4': dict(make=lambda: mgd.MaskGuidance(respace_type='uniform', respace_steps=4),
                         loop=lambda d, m, x: d.resample_loop(m, x, resample_r=2, resample_j=2,
                                                              tqdm_kwargs=dict(disable=True))),
        'ilvr5': dict(make=lambda: ilvr.ILVR(respace_type='uniform', respace_steps=5, downsample_factor=4),
                      loop=lambda d, m, x: d.sample_loop(m, x, tqdm_kwargs=dict(disable=True))),
    }
    for name, tr in trajs.items():
        torch.manual_seed(13)
        init = torch.randn(shape)
        # fp32 run, recording every noise draw
        d = tr['make']()
        if name == 'ilvr5':
            d.set_ref_images(img)
        else:
            d.set_mask_and_image(img * mask, mask)
        rec = Recorder(500)
        with patched_randn_like(rec), torch.no_grad():
            out32 = [o['sample'].clone() for o in tr['loop'](d, model, init)]
        # float64 run of the same reference code on the same noise
        d = tr['make']()
        if name == 'ilvr5':
            d.set_ref_images(img.double())
        else:
            d.set_mask_and_image((img * mask).double(), mask.double())
        with patched_randn_like(Replayer(rec.draws)), torch.no_grad():
            out64 = [o['sample'].clone() for o in tr['loop'](d, model64, init.double())]
        assert all(o.dtype == torch.float64 for o in out64)
        drift = np.array([float((a.double() - b).abs().max()) for a, b in zip(out32, out64)])
        print(name, 'steps', len(out32), 'draws', len(rec.draws), 'drift', drift)
        assert drift.max() <= DRIFT_BOUND, (name, drift)   # else: shorten this trajectory
        arr[f'traj_{name}_init'] = init
        arr[f'traj_{name}_samples'] = torch.stack(out32)
        arr[f'traj_{name}_noises'] = torch.stack(rec.draws)
        arr[f'traj_{name}_drift'] = drift
        meta[f'traj_{name}_steps'] = len(out32)
    mg.save('guidance', meta, **arr)


if __name__ == '__main__':
    main()
