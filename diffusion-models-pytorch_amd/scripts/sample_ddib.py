"""Image-to-image translation with Dual Diffusion Implicit Bridges — drop-in for the reference scripts/sample_ddib.py.

Same CLI (config, seed, input_dir, weights, class_A, class_B, respace_type, respace_steps, save_dir, batch_size) plus
`--a.b value` config overrides and `--weights synthetic`:

    python diffusion-models-pytorch_amd/scripts/sample_ddib.py -c configs/ddpm_cfg_cifar10.yaml \\
        --weights ckpt.pt --input_dir images --class_A 3 --class_B 5 --save_dir out --respace_steps 100

Each input is DDIM-inverted to noise under class A (DDIM.sample_inversion, eta = 0) and sampled back under class B
(DDIM.sample); each output PNG is the row [input, translation]. A latent model (models.base_latent.BaseLatent, the
DiT) encodes the inputs with its VAE first -- the posterior's mode, so a translation is deterministic -- and decodes
the result; it needs a local VAE checkpoint directory (model.params.vae_config.params.from_pretrained).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import diffusions  # noqa: E402
from scripts.sample_mask_guidance import parse  # noqa: E402
from scripts.sample_uncond import build_model  # noqa: E402
from utils.harness import DistEnv, dataset_rounds  # noqa: E402
from utils.imagedir import ImageDir  # noqa: E402
from utils.misc import image_norm_to_float  # noqa: E402
from utils.png import save_image  # noqa: E402

CFG_ONLY_KEYS = ('guidance_scale', 'cond_kwarg')


def get_parser():
    p = argparse.ArgumentParser()
    p.add_argument('-c', '--config', type=str, required=True, help='Path to inference configuration file')
    p.add_argument('--seed', type=int, default=2001, help='Set random seed')
    p.add_argument('--input_dir', type=str, required=True, help='Input directory containing images in domain A')
    p.add_argument('--weights', type=str, required=True, help="Path to model weights, or 'synthetic'")
    p.add_argument('--class_A', type=int, required=True, help='Class label of domain A')
    p.add_argument('--class_B', type=int, required=True, help='Class label of domain B')
    p.add_argument('--respace_type', type=str, default='uniform', help='Type of respaced timestep sequence')
    p.add_argument('--respace_steps', type=int, default=None, help='Length of respaced timestep sequence')
    p.add_argument('--save_dir', type=str, required=True, help='Path to directory saving samples')
    p.add_argument('--batch_size', type=int, default=32, help='Batch size on each process')
    return p


def build_ddim(args, conf, device):
    """Reference sample_ddib.py:97-103: DDIM over the config's diffusion parameters (the keys only its
    classifier-free-guidance classes take are dropped)."""
    params = {k: v for k, v in dict(conf.diffusion.params).items() if k not in CFG_ONLY_KEYS}
    params.update(respace_type=None if args.respace_steps is None else args.respace_type,
                  respace_steps=args.respace_steps or params['total_steps'], device=device)
    return diffusions.ddim.DDIM(**params)


def check_latent_vae(conf):
    """A latent model translates through its VAE in both directions: fail before anything is built when the config
    names no local checkpoint directory (the message is AutoEncoderKL's own)."""
    import importlib
    from models.base_latent import BaseLatent
    module, cls = conf.model.target.rsplit('.', 1)
    if not issubclass(getattr(importlib.import_module(module), cls), BaseLatent):
        return
    from models.dit.autoencoder import AutoEncoderKL
    try:
        fp = conf.model.params.vae_config.params.from_pretrained
    except (AttributeError, KeyError):
        fp = None
    if not isinstance(fp, (str, os.PathLike)) or not os.path.isdir(fp):
        AutoEncoderKL(from_pretrained=fp)  # raises NotImplementedError with the instructions


@torch.no_grad()
def translate(diffuser, model, X, class_A, class_B, tqdm_kwargs=None):
    """[B, C, H, W] images of domain A -> their translations to domain B (both in [-1, 1] image space)."""
    from models.base_latent import BaseLatent
    tq = dict(tqdm_kwargs or {})
    latent = isinstance(model, BaseLatent)
    yA = torch.full((X.shape[0], ), class_A, device=X.device).long()
    yB = torch.full((X.shape[0], ), class_B, device=X.device).long()
    x = model.encode_latent(X, sample_posterior=False) if latent else X
    noise = diffuser.sample_inversion(model=model, img=x, model_kwargs=dict(y=yA),
                                      tqdm_kwargs=dict(tq, desc='img2noise ' + tq.get('desc', '')))
    tX = diffuser.sample(model=model, init_noise=noise, model_kwargs=dict(y=yB),
                         tqdm_kwargs=dict(tq, desc='noise2img ' + tq.get('desc', '')))
    return model.decode_latent(tX) if latent else tX


@torch.no_grad()
def main(argv=None):
    args, conf = parse(get_parser(), argv)
    check_latent_vae(conf)
    env = DistEnv()
    torch.manual_seed(args.seed + env.rank)   # set_seed(seed, device_specific=True)
    diffuser = build_ddim(args, conf, env.device)
    dataset = ImageDir(args.input_dir, conf.data.params.img_size)
    model = build_model(conf, args.weights, env.device)
    os.makedirs(args.save_dir, exist_ok=True)
    if len(dataset) == 0:
        raise ValueError(f'no images found in {args.input_dir}')
    idx = 0
    for i, (ids, keep) in enumerate(dataset_rounds(len(dataset), args.batch_size, env.world, env.rank)):
        X = torch.stack([dataset[k] for k in ids]).to(env.device)
        tX = translate(diffuser, model, X, args.class_A, args.class_B,
                       dict(desc=str(i), disable=not env.is_main)).clamp(-1, 1)
        X, tX = env.gather(X)[:keep], env.gather(tX)[:keep]
        if env.is_main:
            for x, tx in zip(X, tX):
                save_image([image_norm_to_float(x).cpu(), image_norm_to_float(tx).cpu()],
                           os.path.join(args.save_dir, f'{idx}.png'), nrow=2)
                idx += 1
    env.barrier()
    env.close()


if __name__ == '__main__':
    main()
