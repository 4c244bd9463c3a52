"""The latent MDT wrapper end to end: models.mdt.mdt.MDT from a config dict, scripts/sample_cfg.py's latent driver for
3 DDIMCFG steps on the mdt_a geometry, and decode_latent through the tiny synthetic VAE of the VAE tests."""
import os

import numpy as np
import pytest
import torch

from tests import vae_ref

pytestmark = pytest.mark.gpu

CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'diffusion-models-pytorch_amd',
                       'configs')
V = '--model.params.vit_config.params.'
MDT_A = ['--data.params.img_size', '128', '--data.num_classes', '10', V + 'input_size', '16', V + 'hidden_size', '128',
         V + 'depth', '6', V + 'num_heads', '4', V + 'num_classes', '10', V + 'decode_layer', '2']


def test_mdt_latent_sample_cfg_and_decode(cuda, tmp_path):
    from models.base_latent import BaseLatent
    from models.mdt.autoencoder import AutoEncoderKL
    from models.mdt.mdt import MDT
    from models.mdt.model import MDTv2
    from scripts import sample_cfg
    from utils.png import read_png_rgb
    from utils.synthetic import init_synthetic_
    vdir = str(tmp_path / 'vae')
    vae_ref.write_checkpoint_dir(vdir, 'T1')
    arch = dict(input_size=16, patch_size=2, hidden_size=128, depth=6, num_heads=4, num_classes=10, decode_layer=2)
    model = MDT(vae_config=dict(target='models.mdt.autoencoder.AutoEncoderKL', params=dict(from_pretrained=vdir)),
                vit_config=dict(target='models.mdt.model.MDTv2', params=arch), scale_factor=0.18215)
    assert isinstance(model, BaseLatent) and isinstance(model.vit, MDTv2) and model.vae is None
    assert model.supports_null_label
    init_synthetic_(model.vit)
    model = model.to(cuda).eval()

    cfg = os.path.join(CONFIGS, 'mdt_xl2_256.yaml')
    common = ['-c', cfg, '--weights', 'synthetic', '--guidance_scale', '4', '--class_ids', '7',
              '--n_samples_each_class', '2', '--batch_size', '2', '--sampler', 'ddim', '--respace_steps', '3']
    sample_cfg.main(common + ['--save_dir', str(tmp_path / 'lat')] + MDT_A)
    sample_cfg.main(common + ['--save_dir', str(tmp_path / 'img')] + MDT_A +
                    ['--model.params.vae_config.params.from_pretrained', vdir])
    assert sorted(os.listdir(tmp_path / 'lat' / 'class7')) == ['0.npy', '1.npy']
    assert sorted(os.listdir(tmp_path / 'img' / 'class7')) == ['0.png', '1.png']
    lat = torch.from_numpy(np.stack([np.load(tmp_path / 'lat' / 'class7' / f'{i}.npy') for i in range(2)]))
    assert lat.shape == (2, 4, 16, 16) and torch.isfinite(lat).all()

    # the wrapper's forward is the transformer's; its decode_latent gives the script's PNGs within one 8-bit level
    x = lat.to(cuda)
    t = torch.tensor([500, 20], device=cuda)
    y = torch.tensor([7, 7], device=cuda)
    assert torch.equal(model(x, t, y), model.vit(x, t, y))
    img = model.decode_latent(x).clamp(-1, 1).cpu()
    assert isinstance(model.vae, AutoEncoderKL)
    want = ((img + 1) / 2).mul(255).add_(0.5).clamp_(0, 255).permute(0, 2, 3, 1).to(torch.uint8).numpy()
    for i in range(2):
        got = read_png_rgb(str(tmp_path / 'img' / 'class7' / f'{i}.png'))
        assert got.shape == want[i].shape, got.shape
        assert np.abs(got.astype(np.int16) - want[i].astype(np.int16)).max() <= 1
