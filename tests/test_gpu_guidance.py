"""Guided sampling on the engine (diffusions/guidance/, csrc/guidance.hip): the fused MaskGuidance and ILVR
steps, the table-driven low-pass filter, the generic BaseGuidance path, trajectories and the two scripts.

Fixtures: tests/golden/guidance.npz from the reference modules (tests/golden/make_golden_guidance.py), every
noise draw recorded and replayed here through `noise_fn` in the reference's order (reverse_eps, then the
diffusion of the known image).
"""
import os

import numpy as np
import pytest
import torch

from diffusions import DDPM, ILVR, BaseGuidance, MaskGuidance
from diffusions.guidance import lowpass
from tests.conftest import TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Replay:
    """noise_fn replaying recorded draws in order."""

    def __init__(self, draws):
        self.draws, self.k = [torch.as_tensor(d) for d in draws], 0

    def __call__(self, x):
        n = self.draws[self.k]
        self.k += 1
        assert n.shape == x.shape, (n.shape, x.shape)
        return n.to(x.device)


def _t(a, cuda=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(cuda) if cuda is not None else t


# ------------------------------------------------------------------------------------------------ mask step
@pytest.mark.parametrize('i', range(5))
def test_mask_step(cuda, golden, i):
    """Fused MaskGuidance step: mean / pred_x0 / pred_eps are the unguided step's bits; the guided sample is
    bit-identical to the torch CPU float32 expression sample + (noisy_known - sample) * mask on the engine's own
    unguided sample with the same host coefficients, and matches the reference fixture."""
    arrays, meta = golden('guidance')
    c = meta['mask_cases'][i]
    t, tp = c['t'], c['tp']
    xt, mo, masked, mask = (_t(arrays[f'mstep{i}_{k}']) for k in ('xt', 'out', 'masked', 'mask'))
    noises = [arrays[f'mstep{i}_noise{k}'] for k in range(2) if f'mstep{i}_noise{k}' in arrays]
    assert len(noises) == (1 if t == 0 else 2)
    if c['var_type'] == 'learned_range':
        assert mo.shape[1] == 2 * xt.shape[1]

    plain = DDPM(var_type=c['var_type'], device=cuda)
    plain.noise_fn = Replay(noises[:1])
    un = plain.denoise(mo.to(cuda), xt.to(cuda), t, tp)

    d = MaskGuidance(var_type=c['var_type'], device=cuda)
    d.set_mask_and_image(masked.to(cuda), mask.to(cuda))
    d.noise_fn = Replay(noises)
    assert d._fused()
    out = d.guided_denoise(mo.to(cuda), xt.to(cuda), t, tp)
    assert d.noise_fn.k == len(noises)
    for k in ('mean', 'pred_x0', 'pred_eps'):
        assert torch.equal(out[k], un[k]), k
    assert torch.equal(out['reverse_eps'].cpu(), _t(noises[0]))

    s = un['sample'].cpu()
    if t == 0:
        noisy = masked
    else:
        sa, s1m = d._known_coefs(tp, xt.shape[0])
        noisy = sa * masked + s1m * _t(noises[1])
    expect = s + (noisy - s) * mask
    got = out['sample'].cpu()
    assert torch.equal(got, expect), (got - expect).abs().max().item()
    assert np.allclose(got.numpy(), arrays[f'mstep{i}_sample'], rtol=1e-5, atol=2e-5)
    for k in ('mean', 'pred_x0', 'pred_eps'):
        assert np.allclose(out[k].cpu().numpy(), arrays[f'mstep{i}_{k}'], rtol=1e-5, atol=2e-5), k

    # the generic path (denoise + apply_guidance with the class's cond_fn_sample) gives the same bits
    d.noise_fn = Replay(noises)
    gen = d.apply_guidance(**d.denoise(mo.to(cuda), xt.to(cuda), t, tp), xt=xt.to(cuda), t=t, t_prev=tp)
    assert torch.equal(gen['sample'], out['sample'])


def test_mask_step_needs_mask_and_image(cuda):
    d = MaskGuidance(device=cuda)
    x = torch.zeros((1, 3, 8, 8), device=cuda)
    with pytest.raises(RuntimeError, match='set_mask_and_image'):
        d.guided_denoise(x, x, 10, 9)
    d.set_mask_and_image(x, torch.ones((1, 2, 8, 8), device=cuda))
    with pytest.raises(ValueError):
        d.guided_denoise(x, x, 10, 9)


# ------------------------------------------------------------------------------------------ low-pass filter
def _truth64(tables, x, h, w, n):
    dh, dw, uh, uw = tables
    mh = lowpass.densify(uh, h // n) @ lowpass.densify(dh, h)
    mw = lowpass.densify(uw, w // n) @ lowpass.densify(dw, w)
    return mh @ x.double() @ mw.T


@pytest.mark.parametrize('h,w,n,method', [(16, 16, 2, 'cubic'), (32, 32, 8, 'cubic'), (32, 32, 4, 'lanczos3'),
                                          (64, 32, 4, 'linear'), (32, 32, 4, 'box'), (64, 64, 16, 'lanczos2')])
def test_low_pass_filter(cuda, golden, report, h, w, n, method):
    """Engine low_pass_filter against the reference output and against the float64 evaluation of the densified
    tables: its max-abs error to float64 at most 2x the reference fp32 output's own (the reference's reduction
    order is torch's, one of many equally valid ones), hard cap TOL."""
    arrays, _ = golden('guidance')
    x = _t(arrays[f'lp_{h}_{w}_{n}_{method}_x'])
    ref = _t(arrays[f'lp_{h}_{w}_{n}_{method}_y'])
    d = ILVR(downsample_factor=n, interp_method=method, device=cuda)
    y = d.low_pass_filter(x.to(cuda)).cpu()
    truth = _truth64(lowpass.axis_tables(h, w, n, method), x, h, w, n)
    e_eng = (y.double() - truth).abs().max().item()
    e_ref = (ref.double() - truth).abs().max().item()
    e_fix = (y - ref).abs().max().item()
    key = f'lowpass_{h}x{w}_N{n}_{method}'
    report(key + '_engine_vs_float64', e_eng)
    report(key + '_reference_vs_float64', e_ref)
    report(key + '_engine_vs_reference', e_fix)
    print(key, 'engine', e_eng, 'reference', e_ref, 'engine vs reference', e_fix)
    assert e_fix <= TOL, (key, e_fix)
    assert e_eng <= TOL, (key, e_eng)
    assert e_eng <= 2 * e_ref, (key, e_eng, e_ref)


def test_low_pass_filter_two_launch_256(cuda, report):
    """(256, 256, 8, cubic), one plane: the two-launch path (the H/N x W/N intermediate in global scratch) against
    the float64 evaluation of the tables (pinned against the reference on the host, tests/test_guidance_host.py).

    Bound: each pass is a float32 sum of `taps` separately rounded products, error <= (taps + 1) u |w|.|x| with
    u = 2^-24; over the four passes <= sum(taps_i + 1) u A max|x| with A the product of the tables' largest row
    abs-sums (the amplification of an earlier pass's error by the later ones is below A). Hard cap TOL."""
    h = w = 256
    n, method = 8, 'cubic'
    g = torch.Generator().manual_seed(77)
    x = torch.randn((1, 1, h, w), generator=g)
    tables = lowpass.axis_tables(h, w, n, method)
    d = ILVR(downsample_factor=n, interp_method=method, device=cuda)
    plan = d._plan(x.to(cuda))
    assert plan.scratch(1) is not None and plan.scratch(1).numel() == (h // n) * (w // n) * 4
    y = d.low_pass_filter(x.to(cuda)).cpu()
    truth = _truth64(tables, x, h, w, n)
    err = (y.double() - truth).abs().max().item()
    amp = float(np.prod([tw.abs().sum(1).max().item() for tw, _ in tables]))
    bound = sum(tw.shape[1] + 1 for tw, _ in tables) * 2.0 ** -24 * amp * x.abs().max().item()
    report('lowpass_256x256_N8_cubic_engine_vs_float64', err)
    report('lowpass_256x256_N8_cubic_rounding_bound', bound)
    print('lowpass 256', err, 'bound', bound)
    assert err <= min(bound, TOL), (err, bound)


def test_low_pass_filter_rejects_non_dividing_factor(cuda):
    with pytest.raises(ValueError):
        ILVR(downsample_factor=8, device=cuda).low_pass_filter(torch.zeros((1, 1, 36, 32), device=cuda))


# -------------------------------------------------------------------------------------------- ILVR / toy steps
@pytest.mark.parametrize('i', range(2))
def test_ilvr_step(cuda, golden, report, i):
    arrays, meta = golden('guidance')
    c = meta['ilvr_steps'][i]
    noises = [arrays[f'istep{i}_noise{k}'] for k in range(2) if f'istep{i}_noise{k}' in arrays]
    xt, mo, ref = (_t(arrays[f'istep{i}_{k}'], cuda) for k in ('xt', 'out', 'ref'))
    d = ILVR(ref_images=ref, downsample_factor=c['N'], interp_method=c['method'], device=cuda)
    d.noise_fn = Replay(noises)
    assert d._fused()
    out = d.guided_denoise(mo, xt, c['t'], c['tp'])
    assert d.noise_fn.k == len(noises)
    err = np.abs(out['sample'].cpu().numpy() - arrays[f'istep{i}_sample']).max()
    report(f'ilvr_step{i}_maxabs_vs_reference', err)
    print('ilvr step', i, err)
    assert err <= TOL, err
    # the generic composition phi(noisy_ref) - phi(sample) agrees with the fused phi(noisy_ref - sample)
    d.noise_fn = Replay(noises)
    un = d.denoise(mo, xt, c['t'], c['tp'])
    gen = d.apply_guidance(**un, xt=xt, t=c['t'], t_prev=c['tp'])
    lin = (gen['sample'] - out['sample']).abs().max().item()
    report(f'ilvr_step{i}_fused_vs_generic', lin)
    assert lin <= 1e-5, lin   # the linearity identity holds to fp32 rounding (measured 1e-7 .. 8e-7 on the CPU)
    for k in ('mean', 'pred_x0', 'pred_eps'):
        assert torch.equal(out[k], un[k]), k


def test_ilvr_step_two_launch(cuda, report):
    """Planes beyond 64 x 64 (72 x 96: non-square, a partial tile of 16 rows in the second launch), learned
    variance: the fused two-launch step against the engine's own generic composition (unguided denoise, then
    phi(noisy_ref) - phi(sample) with the low-pass filter checked above); the update's other outputs are the
    unguided step's bits, each written once."""
    g = torch.Generator().manual_seed(5)
    shape = (2, 2, 72, 96)
    xt = torch.randn(shape, generator=g).to(cuda)
    mo = torch.randn((2, 4, 72, 96), generator=g).clamp(-1, 1).to(cuda)
    ref = (torch.rand(shape, generator=g) * 2 - 1).to(cuda)
    noises = [torch.randn(shape, generator=g) for _ in range(2)]
    d = ILVR(ref_images=ref, downsample_factor=8, var_type='learned_range', device=cuda)
    assert d._plan(xt).scratch(4) is not None
    d.noise_fn = Replay(noises)
    out = d.guided_denoise(mo, xt, 300, 200)
    d.noise_fn = Replay(noises)
    un = d.denoise(mo, xt, 300, 200)
    gen = d.apply_guidance(**un, xt=xt, t=300, t_prev=200)
    for k in ('mean', 'pred_x0', 'pred_eps', 'var'):
        assert torch.equal(out[k], un[k]), k
    err = (gen['sample'] - out['sample']).abs().max().item()
    report('ilvr_two_launch_fused_vs_generic', err)
    print('ilvr two-launch fused vs generic', err)
    assert err <= 1e-5, err
    assert (out['sample'] - un['sample']).abs().max().item() > 1e-2   # the guidance acted


class ToyGuidance(BaseGuidance):
    """The generator's toy subclass on the engine's BaseGuidance: fixed multiples of a stored tensor."""

    def __init__(self, g, scales, *a, **k):
        super().__init__(*a, **k)
        self.g, self.scales = g, scales

    def cond_fn_eps(self, **kw):
        return self.scales['eps'] * self.g

    def cond_fn_x0(self, **kw):
        return self.scales['x0'] * self.g

    def cond_fn_mean(self, **kw):
        return self.scales['mean'] * self.g


@pytest.mark.parametrize('i', range(2))
def test_toy_subclass_step(cuda, golden, report, i):
    """The generic hook path (cond_fn_eps, cond_fn_x0, cond_fn_mean in the reference's order, with its
    recomputations: the last hook that fires decides each output)."""
    arrays, meta = golden('guidance')
    t, tp = meta['toy_steps'][i]
    xt, mo, gt = (_t(arrays[f'toy{i}_{k}'], cuda) for k in ('xt', 'out', 'g'))
    d = ToyGuidance(gt, meta['toy_scales'], var_type='fixed_small', device=cuda)
    assert not d._fused()
    d.noise_fn = Replay([arrays[f'toy{i}_noise0']])
    out = d.guided_denoise(mo, xt, t, tp)
    worst = 0.0
    for k in ('sample', 'mean', 'pred_x0', 'pred_eps'):
        err = np.abs(out[k].cpu().numpy() - arrays[f'toy{i}_{k}']).max()
        worst = max(worst, err)
        assert err <= TOL, (k, err)
    report(f'toy_guidance_step{i}_maxabs_vs_reference', worst)


def test_pred_x0_from_mu_inverts_pred_mu_from_x0(cuda):
    """dm_lincomb mode 3, bit-identical to the torch CPU expression (mu - coef2 xt) / coef1."""
    g = torch.Generator().manual_seed(3)
    xt, mu = torch.randn((2, 3, 5, 7), generator=g), torch.randn((2, 3, 5, 7), generator=g)
    d = BaseGuidance(device=cuda)
    for t, tp in ((999, 899), (100, 0), (0, -1)):
        c = d._coefs(t, tp)
        got = d.pred_x0_from_mu(xt.to(cuda), t, tp, mu.to(cuda)).cpu()
        c1, c2 = torch.tensor(c['coef1']), torch.tensor(c['coef2'])
        assert torch.equal(got, (mu - c2 * xt) / c1), (t, tp)
        x0 = d.pred_mu_from_x0(xt.to(cuda), t, tp, mu.to(cuda)).cpu()
        assert torch.equal(x0, c1 * mu + c2 * xt), (t, tp)


# ---------------------------------------------------------------------------------------------- trajectories
@pytest.mark.parametrize('name', ['mask5', 'repaint4', 'ilvr5'])
def test_tiny_trajectories(cuda, golden, report, name):
    """MaskGuidance sample_loop (uniform-5), resample_loop (4 steps, r = 2, j = 2: 8 steps, two forward) and ILVR
    sample_loop (uniform-5, N = 4) on the tiny UNet, free running with pinned noise: every step within TOL of the
    reference (whose own fp32 run stays within 5e-5 of its float64 run on these, asserted by the generator)."""
    from tests.test_gpu_parity import _model
    arrays, meta = golden('guidance')
    model, sha = _model(golden('forward')[1], 'tiny', cuda)
    assert sha == meta['tiny_weights_sha256']
    assert float(arrays[f'traj_{name}_drift'].max()) <= meta['drift_bound']
    img, mask = _t(arrays['traj_image'], cuda), _t(arrays['traj_mask'], cuda)
    init = _t(arrays[f'traj_{name}_init'], cuda)
    tq = dict(disable=True)
    if name == 'ilvr5':
        d = ILVR(ref_images=img, downsample_factor=4, respace_type='uniform', respace_steps=5, device=cuda)
        loop = d.sample_loop(model, init, tqdm_kwargs=tq)
    else:
        d = MaskGuidance(respace_type='uniform', respace_steps=5 if name == 'mask5' else 4, device=cuda)
        d.set_mask_and_image(img * mask, mask)
        loop = (d.sample_loop(model, init, tqdm_kwargs=tq) if name == 'mask5' else
                d.resample_loop(model, init, resample_r=2, resample_j=2, tqdm_kwargs=tq))
    d.noise_fn = Replay(arrays[f'traj_{name}_noises'])
    ref = arrays[f'traj_{name}_samples']
    worst, steps = 0.0, 0
    for i, out in enumerate(loop):
        err = np.abs(out['sample'].cpu().numpy() - ref[i]).max()
        worst = max(worst, err)
        steps += 1
        assert err <= TOL, (name, i, err)
    assert steps == meta[f'traj_{name}_steps'] == len(ref)
    assert d.noise_fn.k == len(arrays[f'traj_{name}_noises'])
    report(f'guidance_{name}_tiny_worst_step_maxabs_vs_reference', worst)
    print(name, 'worst step', worst)


def test_sample_goes_through_range_guard(cuda, golden):
    """sample() / resample() return the loop's last sample (device RNG, range check deferred to the loop's end)."""
    from tests.test_gpu_parity import _model
    arrays, _ = golden('guidance')
    model, _ = _model(golden('forward')[1], 'tiny', cuda)
    img, mask = _t(arrays['traj_image'], cuda), _t(arrays['traj_mask'], cuda)
    d = MaskGuidance(respace_type='uniform', respace_steps=2, device=cuda)
    d.set_mask_and_image(img * mask, mask)
    init = _t(arrays['traj_mask5_init'], cuda)
    for fn in (lambda: d.sample(model, init, tqdm_kwargs=dict(disable=True)),
               lambda: d.resample(model, init, resample_r=2, resample_j=1, tqdm_kwargs=dict(disable=True))):
        x = fn()
        assert x.shape == init.shape and torch.isfinite(x).all()
        # the last step has t == 0: the known area is the image itself (s + (known - s) rounds twice)
        assert torch.allclose(x * mask, img * mask, rtol=0, atol=1e-5)


# --------------------------------------------------------------------------------------------------- scripts
def _write_inputs(path, n=3, size=32):
    from utils.png import save_image
    os.makedirs(path, exist_ok=True)
    g = torch.Generator().manual_seed(9)
    for i in range(n):
        save_image(torch.rand((3, size, size), generator=g), os.path.join(path, f'in{i}.png'), nrow=1, padding=0)


@pytest.mark.parametrize('resample', [False, True])
def test_sample_mask_guidance_script(cuda, tmp_path, resample):
    from scripts import sample_mask_guidance
    cfg = os.path.join(ROOT, 'diffusion-models-pytorch_amd', 'configs', 'ddpm_cifar10.yaml')
    _write_inputs(str(tmp_path / 'in'))
    argv = ['-c', cfg, '--weights', 'synthetic', '--respace_steps', '2', '--input_dir', str(tmp_path / 'in'),
            '--save_dir', str(tmp_path / 'out'), '--batch_size', '2']
    if resample:
        argv += ['--resample', '--resample_r', '2', '--resample_j', '1', '--mask_type', 'rect']
    sample_mask_guidance.main(argv)
    assert sorted(os.listdir(tmp_path / 'out')) == ['0.png', '1.png', '2.png']
    from utils.png import read_png_rgb
    assert read_png_rgb(str(tmp_path / 'out' / '0.png')).shape[1] > 3 * 32   # a row of [masked, input, result]
    with pytest.raises(ValueError, match='brush'):
        sample_mask_guidance.main(argv + ['--mask_type', 'brush'])


def test_sample_ilvr_script(cuda, tmp_path):
    from scripts import sample_ilvr
    cfg = os.path.join(ROOT, 'diffusion-models-pytorch_amd', 'configs', 'ddpm_cifar10.yaml')
    _write_inputs(str(tmp_path / 'in'))
    sample_ilvr.main(['-c', cfg, '--weights', 'synthetic', '--respace_steps', '2', '--input_dir',
                      str(tmp_path / 'in'), '--save_dir', str(tmp_path / 'out'), '--batch_size', '2',
                      '--downsample_factor', '4', '--interp_method', 'lanczos2'])
    assert sorted(os.listdir(tmp_path / 'out')) == ['0.png', '1.png', '2.png']
