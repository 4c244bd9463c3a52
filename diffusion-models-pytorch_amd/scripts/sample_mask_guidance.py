"""Inpainting with mask guidance / RePaint — drop-in for the reference scripts/sample_mask_guidance.py.

Same CLI (config, seed, weights, var_type, respace_type, respace_steps, resample, resample_r, resample_j,
input_dir, save_dir, batch_size) plus `--a.b value` config overrides, `--weights synthetic` and `--mask_type`:

    python diffusion-models-pytorch_amd/scripts/sample_mask_guidance.py -c configs/ddpm_cifar10.yaml \\
        --weights ckpt.pt --input_dir images --save_dir out --respace_steps 250 --resample

Each output PNG is the row [masked input, input, result], as the reference writes it. Every reverse step is one
fused launch (DDPM update + mask blend, dm_guided_step).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import diffusions  # noqa: E402
from scripts.sample_uncond import build_model  # noqa: E402
from utils.harness import DistEnv, dataset_rounds  # noqa: E402
from utils.imagedir import ImageDir  # noqa: E402
from utils.mask import MASK_TYPES, DatasetWithMask  # noqa: E402
from utils.misc import image_norm_to_float, load_config  # noqa: E402
from utils.png import save_image  # noqa: E402


def add_common_arguments(p: argparse.ArgumentParser):
    """The arguments sample_mask_guidance.py and sample_ilvr.py share (reference get_parser of both)."""
    p.add_argument('-c', '--config', type=str, required=True, help='Path to inference configuration file')
    p.add_argument('--seed', type=int, default=2022, help='Set random seed')
    p.add_argument('--weights', type=str, required=True, help="Path to pretrained model weights, or 'synthetic'")
    p.add_argument('--var_type', type=str, default=None, help='Type of variance of the reverse process')
    p.add_argument('--respace_type', type=str, default='uniform', help='Type of respaced timestep sequence')
    p.add_argument('--respace_steps', type=int, default=None, help='Length of respaced timestep sequence')
    p.add_argument('--input_dir', type=str, required=True, help='Path to the directory containing input images')
    p.add_argument('--save_dir', type=str, required=True, help='Path to directory saving samples')
    p.add_argument('--batch_size', type=int, default=32, help='Batch size on each process')
    return p


def get_parser():
    p = add_common_arguments(argparse.ArgumentParser())
    p.add_argument('--resample', action='store_true', help='Use resample strategy proposed in RePaint paper')
    p.add_argument('--resample_r', type=int, default=10, help='Number of resampling, as proposed in RePaint paper')
    p.add_argument('--resample_j', type=int, default=10,
                   help='Jump lengths of resampling, as proposed in RePaint paper')
    p.add_argument('--mask_type', type=str, default='center',
                   help=f"Type of the masks: one of {MASK_TYPES} ('dir' reads mask images from --mask_dir). The "
                        "reference's 'brush' type draws with PIL and is not provided")
    p.add_argument('--mask_dir', type=str, default=None, help="Directory of mask images for --mask_type dir")
    return p


def parse(parser, argv=None):
    args, unknown = parser.parse_known_args(argv)
    unknown = [(a[2:] if a.startswith('--') else a) for a in unknown]
    dotlist = [f'{k}={v}' for k, v in zip(unknown[::2], unknown[1::2])]
    return args, load_config(args.config, dotlist)


def diffusion_params(args, conf, device):
    """Reference sample_mask_guidance.py:107-113."""
    params = dict(conf.diffusion.params)
    params.update(var_type=args.var_type or params.get('var_type', None),
                  respace_type=None if args.respace_steps is None else args.respace_type,
                  respace_steps=args.respace_steps or params['total_steps'], device=device)
    return params


@torch.no_grad()
def main(argv=None):
    args, conf = parse(get_parser(), argv)
    env = DistEnv()
    torch.manual_seed(args.seed + env.rank)   # set_seed(seed, device_specific=True)
    diffuser = diffusions.MaskGuidance(**diffusion_params(args, conf, env.device))
    dataset = DatasetWithMask(ImageDir(args.input_dir, conf.data.params.img_size), mask_type=args.mask_type,
                              dir_path=args.mask_dir)
    model = build_model(conf, args.weights, env.device)
    os.makedirs(args.save_dir, exist_ok=True)
    if len(dataset) == 0:
        raise ValueError(f'no images found in {args.input_dir}')
    idx = 0
    for i, (ids, keep) in enumerate(dataset_rounds(len(dataset), args.batch_size, env.world, env.rank)):
        items = [dataset[k] for k in ids]
        X = torch.stack([x for x, _ in items]).to(env.device)
        mask = torch.stack([m for _, m in items]).to(env.device).float()
        init_noise = torch.randn_like(X)
        masked_image = X * mask
        diffuser.set_mask_and_image(masked_image, mask)
        tq = dict(desc=f'Fold {i}', disable=not env.is_main)
        if args.resample:
            recX = diffuser.resample(model=model, init_noise=init_noise, resample_r=args.resample_r,
                                     resample_j=args.resample_j, tqdm_kwargs=tq)
        else:
            recX = diffuser.sample(model=model, init_noise=init_noise, tqdm_kwargs=tq)
        recX = recX.clamp(-1, 1)
        M, X, recX = (env.gather(v)[:keep] for v in (masked_image, X, recX))
        if env.is_main:
            for m, x, r in zip(M, X, recX):
                save_image([image_norm_to_float(v).cpu() for v in (m, x, r)],
                           os.path.join(args.save_dir, f'{idx}.png'), nrow=3)
                idx += 1
    env.barrier()
    env.close()


if __name__ == '__main__':
    main()
