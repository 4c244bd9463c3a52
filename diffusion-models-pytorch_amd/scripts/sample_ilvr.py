"""ILVR sampling (generation conditioned on reference images) — drop-in for the reference scripts/sample_ilvr.py.

Same CLI (config, seed, weights, var_type, respace_type, respace_steps, downsample_factor, interp_method,
input_dir, save_dir, batch_size) plus `--a.b value` config overrides and `--weights synthetic`:

    python diffusion-models-pytorch_amd/scripts/sample_ilvr.py -c configs/ddpm_cifar10.yaml \\
        --weights ckpt.pt --input_dir images --save_dir out --respace_steps 100 --downsample_factor 8

Each output PNG is the row [input, result]. Every reverse step is the fused DDPM update + low-pass guidance
(dm_guided_step: one launch up to 64 x 64 images, two beyond).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import argparse  # noqa: E402

import torch  # noqa: E402

import diffusions  # noqa: E402
from diffusions.guidance.lowpass import INTERP_METHODS  # noqa: E402
from scripts.sample_mask_guidance import add_common_arguments, diffusion_params, parse  # noqa: E402
from scripts.sample_uncond import build_model  # noqa: E402
from utils.harness import DistEnv, dataset_rounds  # noqa: E402
from utils.imagedir import ImageDir  # noqa: E402
from utils.misc import image_norm_to_float  # noqa: E402
from utils.png import save_image  # noqa: E402


def get_parser():
    p = add_common_arguments(argparse.ArgumentParser())
    p.add_argument('--downsample_factor', type=int, default=8, help='Downsample factor of the low-pass filter')
    p.add_argument('--interp_method', type=str, default='cubic', choices=sorted(INTERP_METHODS),
                   help='Interpolation method of the low-pass filter')
    return p


@torch.no_grad()
def main(argv=None):
    args, conf = parse(get_parser(), argv)
    env = DistEnv()
    torch.manual_seed(args.seed + env.rank)   # set_seed(seed, device_specific=True)
    diffuser = diffusions.ILVR(downsample_factor=args.downsample_factor, interp_method=args.interp_method,
                               **diffusion_params(args, conf, env.device))
    dataset = ImageDir(args.input_dir, conf.data.params.img_size)
    model = build_model(conf, args.weights, env.device)
    os.makedirs(args.save_dir, exist_ok=True)
    if len(dataset) == 0:
        raise ValueError(f'no images found in {args.input_dir}')
    idx = 0
    for i, (ids, keep) in enumerate(dataset_rounds(len(dataset), args.batch_size, env.world, env.rank)):
        X = torch.stack([dataset[k] for k in ids]).to(env.device)
        init_noise = torch.randn_like(X)
        diffuser.set_ref_images(ref_images=X)
        out = diffuser.sample(model=model, init_noise=init_noise,
                              tqdm_kwargs=dict(desc=f'Fold {i}', disable=not env.is_main)).clamp(-1, 1)
        X, out = env.gather(X)[:keep], env.gather(out)[:keep]
        if env.is_main:
            for x, o in zip(X, out):
                save_image([image_norm_to_float(x).cpu(), image_norm_to_float(o).cpu()],
                           os.path.join(args.save_dir, f'{idx}.png'), nrow=2)
                idx += 1
    env.barrier()
    env.close()


if __name__ == '__main__':
    main()
