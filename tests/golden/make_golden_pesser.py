"""Generate the pesser DDPM UNet / SDEdit fixtures (tests/golden/pesser.npz/.json) from the REFERENCE implementation on
the CPU.

The reference models/pesser/model.py and diffusions/ddpm.py are imported from /root/reference and run: these fixtures
are reference outputs (build container only; nothing on the GPU box runs this file).
    python tests/golden/make_golden_pesser.py

Weights: utils.synthetic.synthetic_pesser_state_dict over the reference state_dict (sha256 recorded). The npz holds
inputs and expected outputs only. Per architecture: x ~ N(0, 1) [2, 3, 32, 32], t = [999, 12], out = model(x, t), and
x_small = scale * x with out_small (a small input makes the GroupNorm variances small, so eps shows). The generator
also checks, and records in pesser.json, how far breaking each mechanism that differs from models/unet.py moves the
reference output: symmetric padding in Downsample, [cos, sin] embedding order, uniform and transposed attention
(each >= 100 x the forward tolerance 1e-4), and eps 1e-5 in place of 1e-6 on x_small (>= 50 x 1e-4; the input scale
is lowered from 0.01 until it is, and recorded). It records the reference's own float32-vs-float64 error and the
state_dict names and shapes of the three architectures and of the two shipped 256^2 configs.

The SDEdit trajectory (pesser_c, linear-1000 DDPM fixed_small, uniform respacing to 10 steps, edit_steps 4) follows
the reference scripts/sample_sdedit.py:140-158 with the diffuse noise and the four step noises drawn once from a
seeded CPU generator and stored, run in float32 and in float64 (make_golden_r2.Float64Reference), with the per-step
drift between the two.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_golden_r2 import Float64Reference, patched_randn_like  # noqa: E402

REFERENCE = '/root/reference'
TOL = 1e-4
COMMON = dict(in_channels=3, out_ch=3, resolution=32)
ARCHS = {
    # the folded 256-channel block (16 x 16 map) at eps 1e-6 on the down path, in the middle and on the up path
    'pesser_a': dict(ch=128, ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=[16], **COMMON),
    # one head of 512 channels at L = 256; up-path concat widths 1024 and 640
    'pesser_b': dict(ch=128, ch_mult=(1, 4), num_res_blocks=1, attn_resolutions=[16], **COMMON),
    # two downsamples, L = 64 attention, level 0 without attention
    'pesser_c': dict(ch=32, ch_mult=(1, 2, 2), num_res_blocks=2, attn_resolutions=[8], **COMMON),
}
CONFIGS_256 = {
    'lsun_church_256': 'ema_diffusion_lsun_church_model-4432000.yaml',
    'celebahq_256': 'ema_diffusion_celebahq_model-560000.yaml',
}
SDEDIT = dict(respace_type='uniform', respace_steps=10, edit_steps=4, var_type='fixed_small')


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def import_reference():
    """(the reference pesser model module, the reference diffusions.ddpm module, this repo's utils.synthetic)."""
    pesser = _load('reference_pesser_model', os.path.join(REFERENCE, 'models', 'pesser', 'model.py'))
    pkg = types.ModuleType('diffusions')
    pkg.__path__ = [os.path.join(REFERENCE, 'diffusions')]
    sys.modules['diffusions'] = pkg
    import diffusions.ddpm as ddpm
    syn = _load('dm_synthetic', os.path.join(REPO, 'diffusion-models-pytorch_amd', 'utils', 'synthetic.py'))
    return pesser, ddpm, syn


def reference_model(pesser, syn, arch):
    model = pesser.Model(**arch).eval()
    sd = syn.synthetic_pesser_state_dict(model.state_dict())
    model.load_state_dict(sd)
    return model, sd


class patched:
    """Replace attributes of an object for the duration of a with block."""

    def __init__(self, obj, **attrs):
        self.obj, self.attrs, self.saved = obj, attrs, {}

    def __enter__(self):
        for k, v in self.attrs.items():
            self.saved[k] = getattr(self.obj, k)
            setattr(self.obj, k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(self.obj, k, v)


def symmetric_downsample(self, x):
    """Downsample with the padding of models/unet.py's stride-2 conv (1 on every side) instead of (0, 1, 0, 1)."""
    return F.conv2d(x, self.conv.weight, self.conv.bias, stride=2, padding=1)


def broken_softmax(kind):
    """A stand-in for torch.nn.functional.softmax while the reference forward runs (only its attention blocks call
    it, on scores [B, queries, keys] over dim 2): 'uniform' weighs every key 1 / L whatever the scores, 'transposed'
    normalises the transposed score matrix (each query's weights are then its column's)."""
    real = F.softmax

    def uniform(w, dim):
        return torch.full_like(w, 1.0 / w.shape[dim])

    def transposed(w, dim):
        return real(w.transpose(1, 2), dim=dim)
    return dict(uniform=uniform, transposed=transposed)[kind]


class unscaled_scores:
    """For the duration of a with block the q convs of the attention blocks return q sqrt(C), which cancels the
    C^-1/2 the reference applies to the scores."""

    def __init__(self, pesser, model):
        self.convs = [m.q for m in model.modules() if isinstance(m, pesser.AttnBlock)]

    def __enter__(self):
        self.handles = [c.register_forward_hook(lambda mod, args, out: out * mod.out_channels ** 0.5)
                        for c in self.convs]

    def __exit__(self, *exc):
        for h in self.handles:
            h.remove()


def sensitivity(pesser, model, x, t, base):
    """max |reference output - output with one mechanism broken|, on (x, t)."""
    out = {}
    with patched(pesser.Downsample, forward=symmetric_downsample):
        out['symmetric_downsample'] = float((model(x, t) - base).abs().max())
    orig = pesser.get_timestep_embedding

    def cos_sin(timesteps, dim):
        e = orig(timesteps, dim)
        return torch.cat([e[:, dim // 2:], e[:, :dim // 2]], dim=1)
    with patched(pesser, get_timestep_embedding=cos_sin):
        out['cos_sin_embedding'] = float((model(x, t) - base).abs().max())
    for kind in ('uniform', 'transposed'):
        with patched(F, softmax=broken_softmax(kind)):
            out[f'{kind}_attention'] = float((model(x, t) - base).abs().max())
    with unscaled_scores(pesser, model):
        out['unscaled_attention'] = float((model(x, t) - base).abs().max())
    return out


def eps_sensitivity(model, x, t, base):
    norms = [m for m in model.modules() if isinstance(m, torch.nn.GroupNorm)]
    assert norms and all(m.eps == 1e-6 for m in norms)
    for m in norms:
        m.eps = 1e-5
    try:
        return float((model(x, t) - base).abs().max())
    finally:
        for m in norms:
            m.eps = 1e-6


def sdedit_reference(ddpm, model, x0, diffuse_noise, step_noise):
    """scripts/sample_sdedit.py:140-158 with stored noises, in float32 and float64. Returns (meta, arrays)."""
    p = SDEDIT
    runs = {}
    for tag, mdl, cast in (('32', model, lambda v: v), ('64', Float64Reference(model), lambda v: v.double())):
        d = ddpm.DDPM(var_type=p['var_type'], respace_type=p['respace_type'], respace_steps=p['respace_steps'])
        assert 0 < p['edit_steps'] < len(d.respaced_seq)
        time_seq = d.respaced_seq[:p['edit_steps']].tolist()
        time_seq_prev = [-1] + time_seq[:-1]
        noised = d.diffuse(x0=cast(x0), t=time_seq[-1], eps=cast(diffuse_noise))
        img = noised.clone()
        samples = []
        draws = iter(step_noise)
        with patched_randn_like(lambda x: next(draws).to(x.dtype)):
            for t, t_prev in zip(reversed(time_seq), reversed(time_seq_prev)):
                t_batch = torch.full((img.shape[0], ), t)
                img = d.denoise(mdl(img, t_batch), img, t, t_prev)['sample']
                samples.append(img.clone())
        assert next(draws, None) is None, 'one draw per step, the last included'
        runs[tag] = (noised, samples, time_seq)
    n32, s32, seq = runs['32']
    n64, s64, _ = runs['64']
    arr = dict(sdedit_x0=x0, sdedit_diffuse_noise=diffuse_noise, sdedit_step_noise=torch.stack(step_noise),
               sdedit_noised=n32, sdedit_noised64=n64.float(),
               sdedit_drift_sample=np.array([float((a.double() - b).abs().max()) for a, b in zip(s32, s64)]))
    for i, (a, b) in enumerate(zip(s32, s64)):
        arr[f'sdedit_step{i}_sample'] = a
        arr[f'sdedit_step{i}_sample64'] = b.float()   # float64 run, rounded for storage
    arr['sdedit_edited'] = s32[-1].clamp(-1, 1)
    meta = dict(p, time_seq=seq, max_drift_sample=float(arr['sdedit_drift_sample'].max()))
    return meta, arr


def main():
    torch.set_num_threads(8)
    pesser, ddpm, syn = import_reference()
    meta = dict(torch=torch.__version__, generator='reference models/pesser/model.py, diffusions/ddpm.py', tol=TOL,
                archs={k: dict(v, ch_mult=list(v['ch_mult'])) for k, v in ARCHS.items()})
    fx = {}
    g = torch.Generator().manual_seed(61)
    with torch.no_grad():
        for name, arch in ARCHS.items():
            model, sd = reference_model(pesser, syn, arch)
            meta[f'{name}_weights_sha256'] = syn.state_dict_sha256(sd)
            meta[f'{name}_state_dict'] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
            x = torch.randn((2, 3, 32, 32), generator=g)
            t = torch.tensor([999, 12])
            out = model(x, t)
            sens = sensitivity(pesser, model, x, t, out)
            for k in ('symmetric_downsample', 'cos_sin_embedding', 'uniform_attention', 'transposed_attention'):
                assert sens[k] >= 100 * TOL, (name, k, sens[k])
            scale = 0.01
            while True:
                xs = scale * x
                out_small = model(xs, t)
                sens['eps_1e-5_on_x_small'] = eps_sensitivity(model, xs, t, out_small)
                if sens['eps_1e-5_on_x_small'] >= 50 * TOL:
                    break
                scale /= 2
                assert scale > 1e-5, (name, sens)
            sens['eps_1e-5_on_x'] = eps_sensitivity(model, x, t, out)
            m64 = Float64Reference(model)
            sens['reference_f32_vs_f64'] = float((out.double() - m64(x.double(), t)).abs().max())
            sens['reference_f32_vs_f64_small'] = float((out_small.double() - m64(xs.double(), t)).abs().max())
            meta[f'{name}_sensitivity'] = sens
            meta[f'{name}_small_scale'] = scale
            fx[f'{name}_x'], fx[f'{name}_t'], fx[f'{name}_out'] = x, t, out
            fx[f'{name}_x_small'], fx[f'{name}_out_small'] = xs, out_small
            print(name, sens, 'scale', scale, flush=True)
        # names and shapes of the two shipped configs (no forward, no storage: meta tensors)
        import yaml
        for key, fname in CONFIGS_256.items():
            with open(os.path.join(REFERENCE, 'weights', 'pesser', 'pytorch_diffusion', fname)) as f:
                params = yaml.safe_load(f)['model']['params']
            with torch.device('meta'):
                big = pesser.Model(**params)
            meta[f'{key}_params'] = params
            meta[f'{key}_state_dict'] = [[k, list(v.shape)] for k, v in big.state_dict().items()]
        # SDEdit on pesser_c
        model, _ = reference_model(pesser, syn, ARCHS['pesser_c'])
        gs = torch.Generator().manual_seed(67)
        x0 = torch.tanh(torch.randn((2, 3, 32, 32), generator=gs))
        diffuse_noise = torch.randn((2, 3, 32, 32), generator=gs)
        step_noise = [torch.randn((2, 3, 32, 32), generator=gs) for _ in range(SDEDIT['edit_steps'])]
        meta['sdedit'], arr = sdedit_reference(ddpm, model, x0, diffuse_noise, step_noise)
        fx.update(arr)
        print('sdedit', meta['sdedit'], flush=True)
    arrays = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in fx.items()}
    np.savez_compressed(os.path.join(HERE, 'pesser.npz'), **arrays)
    with open(os.path.join(HERE, 'pesser.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print({k: v.shape for k, v in arrays.items()})


if __name__ == '__main__':
    main()
