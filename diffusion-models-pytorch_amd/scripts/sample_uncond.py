"""Unconditional sampling — drop-in for the reference scripts/sample_uncond.py.

Same CLI (config, seed, weights, n_samples, save_dir, batch_size, sampler,
respace_type, respace_steps, var_type, ddim_eta, mode) plus `--a.b value`
config overrides. Launch one process per GPU:

    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 \\
        diffusion-models-pytorch_amd/scripts/sample_uncond.py -c configs/ddpm_cifar10.yaml \\
        --weights ckpt.pt --n_samples 2048 --batch_size 256 --sampler ddim --respace_steps 50 --save_dir out

`--weights synthetic` uses the deterministic synthetic weights (no checkpoint
offline). Samplers: ddpm, ddim, euler, heun. Modes: sample, denoise, progressive, interpolate,
reconstruction (DDIM inversion of the images under --input_dir, then sampling back).

Latent denoisers (the DiT config) are sampled by scripts/sample_cfg.py, which builds its model with this
script's `build_model`: the override `--model.params.vae_config.params.from_pretrained /path/to/dir` (a local
diffusers-layout VAE directory) is all it takes for decoded PNGs; there is no new flag.

`--conv_half` (not a reference option) turns on the engine's conv-half option of a conv UNet (`set_conv_half`): the
covered 3x3 convs spend one fp16 matrix-core product per MAC; faster, without fp32 parity.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import diffusions  # noqa: E402
from utils.harness import DistEnv, per_process_batch  # noqa: E402
from utils.load import load_weights  # noqa: E402
from utils.misc import amortize, image_norm_to_float, instantiate_from_config, load_config  # noqa: E402
from utils.png import save_image  # noqa: E402
from utils.synthetic import init_synthetic_  # noqa: E402


def get_parser():
    p = argparse.ArgumentParser()
    p.add_argument('-c', '--config', type=str, required=True, help='Path to inference configuration file')
    p.add_argument('--seed', type=int, default=2022, help='Set random seed')
    p.add_argument('--weights', type=str, required=True, help="Path to model weights, or 'synthetic'")
    p.add_argument('--n_samples', type=int, required=True, help='Number of samples')
    p.add_argument('--save_dir', type=str, required=True, help='Path to directory saving samples')
    p.add_argument('--batch_size', type=int, default=500, help='Batch size on each process')
    p.add_argument('--sampler', type=str, choices=['ddpm', 'ddim', 'euler', 'heun'], default='ddpm',
                   help='Type of sampler')
    p.add_argument('--respace_type', type=str, default='uniform', help='Type of respaced timestep sequence')
    p.add_argument('--respace_steps', type=int, default=None, help='Length of respaced timestep sequence')
    p.add_argument('--var_type', type=str, default=None, help='Type of variance of the reverse process')
    p.add_argument('--ddim_eta', type=float, default=0.0, help='Parameter eta in DDIM sampling')
    p.add_argument('--mode', type=str, default='sample', choices=['sample', 'denoise', 'progressive', 'interpolate',
                                                                          'reconstruction'])
    p.add_argument('--n_denoise', type=int, default=20)
    p.add_argument('--n_progressive', type=int, default=20)
    p.add_argument('--n_interpolate', type=int, default=16, help='Number of intermediate images (interpolate)')
    p.add_argument('--input_dir', type=str, required=False, help='Directory of images (reconstruction)')
    p.add_argument('--conv_half', action='store_true',
                   help="the engine's conv-half option (not in the reference): one fp16 product per MAC in the covered 3x3 "
                        "convs of a conv UNet; faster, no fp32 parity")
    return p


def build_diffuser(args, conf, device):
    """Reference sample_uncond.py:140-160."""
    dp = conf.diffusion.params
    params = dict(
        total_steps=dp.total_steps, beta_schedule=dp.beta_schedule, beta_start=dp.beta_start,
        beta_end=dp.beta_end, objective=dp.objective,
        respace_type=None if args.respace_steps is None else args.respace_type,
        respace_steps=args.respace_steps or dp.total_steps, device=device,
    )
    if args.sampler == 'ddpm':
        return diffusions.ddpm.DDPM(var_type=args.var_type or dp.get('var_type', None), **params)
    if args.sampler == 'ddim':
        return diffusions.ddim.DDIM(eta=args.ddim_eta, **params)
    if args.sampler == 'euler':
        return diffusions.euler.EulerSampler(**params)
    if args.sampler == 'heun':
        return diffusions.heun.HeunSampler(**params)
    raise ValueError(f'Unknown sampler: {args.sampler}')


# reference sample_uncond.py:22-27
COMPATIBLE_SAMPLER_MODE = dict(
    ddpm=['sample', 'denoise', 'progressive'],
    ddim=['sample', 'denoise', 'progressive', 'interpolate', 'reconstruction'],
    euler=['sample', 'denoise', 'progressive', 'interpolate'],
    heun=['sample', 'denoise', 'progressive', 'interpolate'],
)


def slerp(t, z1, z2):
    """Spherical interpolation of two noise batches (reference sample_uncond.py:253-255)."""
    theta = torch.acos(torch.sum(z1 * z2) / (torch.linalg.norm(z1) * torch.linalg.norm(z2)))
    return torch.sin((1 - t) * theta) / torch.sin(theta) * z1 + torch.sin(t * theta) / torch.sin(theta) * z2


def build_model(conf, weights, device):
    from models.base_latent import BaseLatent
    model = instantiate_from_config(conf.model)
    if weights == 'synthetic':
        # a latent wrapper's checkpoint is its denoiser's (models/dit/dit.py load_state_dict -> vit)
        init_synthetic_(model.vit if isinstance(model, BaseLatent) else model)
    else:
        model.load_state_dict(load_weights(weights))
    return model.to(device).eval()


def apply_conv_half(model, on: bool):
    """`--conv_half` of the sampling scripts: the conv UNets take it; a token model points at its own switch."""
    if not on:
        return
    if hasattr(model, 'set_math'):
        raise SystemExit(f'--conv_half is the conv UNets\' option; {type(model).__name__} is a token model: '
                         f'use --math fp16 (scripts/sample_cfg.py) for its half-precision mode')
    if not hasattr(model, 'set_conv_half'):
        raise SystemExit(f'--conv_half: {type(model).__name__} has no native conv path')
    model.set_conv_half(True)


def parse_with_overrides(argv=None):
    args, unknown = get_parser().parse_known_args(argv)
    unknown = [(a[2:] if a.startswith('--') else a) for a in unknown]
    dotlist = [f'{k}={v}' for k, v in zip(unknown[::2], unknown[1::2])]
    return args, load_config(args.config, dotlist)


@torch.no_grad()
def reconstruction(args, conf, env, diffuser, model):
    """Reference sample_uncond.py:279-312: DDIM-invert each batch of input images to noise, sample it back,
    save [input, reconstruction] side by side. Batches are dealt to ranks round-robin as accelerate's
    prepared DataLoader does (batch k*world + rank), gathered in rank order, and the padding of the last
    round is dropped (gather_for_metrics)."""
    from utils.imagedir import ImageDir
    dataset = ImageDir(args.input_dir, conf.data.params.img_size)
    n = min(args.n_samples, len(dataset))
    bspp = min(args.batch_size, math.ceil(n / env.world))
    n_batches = math.ceil(n / bspp)
    idx = 0
    for rnd in range(math.ceil(n_batches / env.world)):
        b = rnd * env.world + env.rank
        lo = b * bspp
        ids = [(lo + j) % n for j in range(bspp)]   # padding wraps to the start, like even_batches
        X = torch.stack([dataset[k] for k in ids]).to(env.device)
        tq = dict(desc=f'img2noise {rnd}', disable=not env.is_main)
        noise = diffuser.sample_inversion(model=model, img=X, tqdm_kwargs=tq)
        recX = diffuser.sample(model=model, init_noise=noise, tqdm_kwargs=dict(tq, desc=f'noise2img {rnd}'))
        keep = max(0, min(n - rnd * env.world * bspp, env.world * bspp))
        X, recX = env.gather(X)[:keep], env.gather(recX)[:keep]
        if env.is_main:
            for x, r in zip(X, recX):
                save_image([image_norm_to_float(x).cpu(), image_norm_to_float(r).cpu()],
                           os.path.join(args.save_dir, f'{idx}.png'), nrow=2)
                idx += 1


@torch.no_grad()
def main(argv=None):
    args, conf = parse_with_overrides(argv)
    env = DistEnv()
    torch.manual_seed(args.seed + env.rank)   # set_seed(seed, device_specific=True)
    diffuser = build_diffuser(args, conf, env.device)
    model = build_model(conf, args.weights, env.device)
    apply_conv_half(model, args.conv_half)
    os.makedirs(args.save_dir, exist_ok=True)
    img_shape = (conf.data.img_channels, conf.data.params.img_size, conf.data.params.img_size)
    bspp = per_process_batch(args.n_samples, args.batch_size, env.world)
    folds = amortize(args.n_samples, bspp * env.world)
    n_seq = len(diffuser.respaced_seq)
    if args.mode not in COMPATIBLE_SAMPLER_MODE[args.sampler] and env.is_main:
        print(f'`{args.mode}` mode is not designed for `{args.sampler}` sampler, unexpected behavior may occur.')
    if args.mode == 'reconstruction':
        if args.input_dir is None:
            raise ValueError('input_dir is required for mode `reconstruction`')
        reconstruction(args, conf, env, diffuser, model)
        env.barrier()
        env.close()
        return
    idx = 0
    for i, bs in enumerate(folds):
        tq = dict(desc=f'Fold {i}/{len(folds)}', disable=not env.is_main)
        if args.mode == 'interpolate':  # reference sample_uncond.py:248-276
            z1 = torch.randn((bspp, *img_shape), device=env.device)
            z2 = torch.randn((bspp, *img_shape), device=env.device)
            samples = torch.stack([
                diffuser.sample(model=model, init_noise=slerp(t, z1, z2), tqdm_kwargs=tq).clamp(-1, 1)
                for t in torch.linspace(0, 1, args.n_interpolate)
            ], dim=1)
            samples = env.gather(samples)[:bs]
            if env.is_main:
                for x in samples:
                    save_image(image_norm_to_float(x.float().cpu()), os.path.join(args.save_dir, f'{idx}.png'),
                               nrow=len(x))
                    idx += 1
            continue
        init_noise = torch.randn((bspp, *img_shape), device=env.device)
        if args.mode == 'sample':
            samples = diffuser.sample(model=model, init_noise=init_noise, tqdm_kwargs=tq).clamp(-1, 1)
        else:
            key = 'sample' if args.mode == 'denoise' else 'pred_x0'
            freq = n_seq // (args.n_denoise if args.mode == 'denoise' else args.n_progressive)
            keep = [out[key] for k, out in enumerate(diffuser.sample_loop(model=model, init_noise=init_noise,
                                                                         tqdm_kwargs=tq))
                    if (n_seq - k - 1) % freq == 0]
            samples = torch.stack(keep, dim=1).clamp(-1, 1)
        samples = env.gather(samples)[:bs]
        if env.is_main:
            for x in samples:   # a row of intermediate images is one nrow=len(x) grid
                save_image(image_norm_to_float(x.float().cpu()), os.path.join(args.save_dir, f'{idx}.png'),
                           nrow=len(x) if x.ndim == 4 else 1)
                idx += 1
    env.barrier()
    env.close()


if __name__ == '__main__':
    main()
