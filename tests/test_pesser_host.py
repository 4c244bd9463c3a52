"""Host-side checks of the pesser DDPM UNet (models/pesser/model.py), variant 3 of the UNet executor, and the SDEdit
script's surface: no GPU.

tests/golden/pesser.json records what the REFERENCE module registers (names and shapes of its state_dict, for the
three fixture architectures and for the two shipped 256^2 configs) and how far breaking each mechanism that
distinguishes this model from models/unet.py moves the reference's output (tests/golden/make_golden_pesser.py).
"""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.conftest import TOL, load_golden

ARCH_NAMES = ['pesser_a', 'pesser_b', 'pesser_c']
CONFIG_NAMES = ['lsun_church_256', 'celebahq_256']
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, 'diffusion-models-pytorch_amd', 'configs')


@pytest.fixture(scope='module')
def meta():
    return load_golden('pesser')[1]


def _build(name, meta):
    """The model of a fixture architecture or of a shipped config (on the meta device: names and shapes only)."""
    from models.pesser.model import Model
    from utils.misc import instantiate_from_config, load_config
    with torch.device('meta'):
        if name in ARCH_NAMES:
            return Model(**meta['archs'][name])
        conf = load_config(os.path.join(CONFIGS, f'pesser_{name}.yaml'))
        assert conf.model.target == 'models.pesser.model.Model'
        return instantiate_from_config(conf.model)


@pytest.mark.parametrize('name', ARCH_NAMES + CONFIG_NAMES)
def test_state_dict_names_and_shapes(meta, name):
    """The parameter container registers exactly the reference's tensors, in its order."""
    got = [[k, list(v.shape)] for k, v in _build(name, meta).state_dict().items()]
    assert got == meta[f'{name}_state_dict']


@pytest.mark.parametrize('name', ARCH_NAMES + CONFIG_NAMES)
def test_param_count_variant3(meta, name):
    """dm_unet_param_count knows variant 3 and returns the reference's tensor count."""
    from dmhip._lib import check, load
    model = _build(name, meta)
    arch = model._arch_struct()
    assert arch.variant == 3
    n = ctypes.c_int(-1)
    check(load().dm_unet_param_count(ctypes.byref(arch), ctypes.byref(n)), 'dm_unet_param_count')
    assert n.value == len(meta[f'{name}_state_dict'])


def _walk_names(names, model):
    """The tensors in the order the executor's walk consumes them (unet_exec.hip: a block, then its attention, ...,
    then the level's resample conv; the up path from the deepest level), from the recorded state_dict names."""
    def under(prefix):
        return [n for n in names if n.startswith(prefix + '.')]
    L, R, attn = len(model.arch['dim_mults']), model.arch['num_res_blocks'], model.arch['use_attn']
    seq = under('temb.dense.0') + under('temb.dense.1') + under('conv_in')
    for i in range(L):
        for j in range(R):
            seq += under(f'down.{i}.block.{j}') + (under(f'down.{i}.attn.{j}') if attn[i] else [])
        seq += under(f'down.{i}.downsample') if i < L - 1 else []
    seq += under('mid.block_1') + under('mid.attn_1') + under('mid.block_2')
    for i in reversed(range(L)):
        for j in range(R + 1):
            seq += under(f'up.{i}.block.{j}') + (under(f'up.{i}.attn.{j}') if attn[i] else [])
        seq += under(f'up.{i}.upsample') if i > 0 else []
    return seq + under('norm_out') + under('conv_out')


@pytest.mark.parametrize('name', ARCH_NAMES + CONFIG_NAMES)
def test_param_order_table(meta, name):
    """The executor's order table for variant 3 (dm_debug_unet_param_order) is a permutation of the state_dict that
    yields the walk's sequence -- on the 256^2 configs too, where an attention level is followed by a downsample
    (down.4.block.*, down.4.attn.*, down.4.downsample) and `up` is stored against the order it runs in. Inside a
    block the tensors keep the order the executor reads them in."""
    from dmhip._lib import UNetArch, check, load
    model = _build(name, meta)
    names = [k for k, _ in meta[f'{name}_state_dict']]
    n = len(names)
    order = (ctypes.c_int * n)()
    f = load().dm_debug_unet_param_order
    f.argtypes = [ctypes.POINTER(UNetArch), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    arch = model._arch_struct()
    check(f(ctypes.byref(arch), order, n), 'dm_debug_unet_param_order')
    assert sorted(order) == list(range(n))
    want = _walk_names(names, model)
    assert len(want) == n and [names[i] for i in order] == want
    assert list(order) != list(range(n))   # not the identity: the registration order is not the walk's
    first = [k.split('.', 4)[-1] for k in want if k.startswith('down.0.block.0.')]
    assert first == [f'{m}.{p}' for m in ('norm1', 'conv1', 'temb_proj', 'norm2', 'conv2') for p in ('weight', 'bias')]
    assert [k.split('.')[-2] for k in want if k.startswith('mid.attn_1.')][::2] == ['norm', 'q', 'k', 'v', 'proj_out']
    assert f(ctypes.byref(arch), order, n - 1) != 0


def test_shipped_configs_match_the_reference(meta):
    """Both configs carry the reference's hyper-parameters and the DDPM block with var_type fixed_small."""
    from utils.misc import load_config
    for name in CONFIG_NAMES:
        conf = load_config(os.path.join(CONFIGS, f'pesser_{name}.yaml'))
        assert dict(conf.model.params) == meta[f'{name}_params']
        assert conf.diffusion.target == 'diffusions.ddpm.DDPM'
        assert conf.diffusion.params.var_type == 'fixed_small'
        assert conf.data.params.img_size == 256
    model = _build('lsun_church_256', meta)
    assert model.arch['use_attn'] == [False, False, False, False, True, False]


def test_resamp_without_conv_is_not_built(meta):
    from models.pesser.model import Model
    with pytest.raises(NotImplementedError):
        Model(**dict(meta['archs']['pesser_c'], resamp_with_conv=False))


def test_forward_rejects_other_resolutions(meta):
    """The reference asserts x.shape[2] == x.shape[3] == resolution before anything else; so does the container."""
    from models.pesser.model import Model
    model = Model(**meta['archs']['pesser_c'])
    for shape in ((1, 3, 16, 16), (1, 3, 32, 64)):
        with pytest.raises(AssertionError):
            model(torch.zeros(shape), torch.zeros((1, ), dtype=torch.long))


def test_synthetic_recipe(meta):
    """synthetic_pesser_state_dict reproduces the fixture weights (sha256) and is what init_synthetic_ loads."""
    from models.pesser.model import Model
    from utils.synthetic import init_synthetic_, state_dict_sha256, synthetic_pesser_state_dict
    model = Model(**meta['archs']['pesser_c'])
    sd = synthetic_pesser_state_dict(model.state_dict())
    assert state_dict_sha256(sd) == meta['pesser_c_weights_sha256']
    assert init_synthetic_(model) == meta['pesser_c_weights_sha256']
    g = sd['mid.attn_1.norm.weight']
    assert 0.5 <= float(g.min()) and float(g.max()) <= 1.5 and float(g.std()) > 0.1


def test_sdedit_parser_matches_the_reference():
    """Option names, defaults and required flags of the reference scripts/sample_sdedit.py:23-65."""
    from scripts.sample_sdedit import get_parser
    want = {
        'config': (None, True), 'seed': (2022, False), 'weights': (None, True), 'var_type': (None, False),
        'respace_type': ('uniform', False), 'respace_steps': (None, False), 'edit_steps': (None, True),
        'input_dir': (None, True), 'save_dir': (None, True), 'batch_size': (32, False),
    }
    got = {a.dest: (a.default, a.required) for a in get_parser()._actions if not isinstance(a, argparse._HelpAction)}
    assert got == want
    args = get_parser().parse_args(['-c', 'x.yaml', '--weights', 'w', '--edit_steps', '400', '--input_dir', 'i',
                                    '--save_dir', 'o'])
    assert args.config == 'x.yaml' and args.edit_steps == 400


def test_edit_steps_bounds():
    """1 <= edit_steps < len(respaced_seq), else ValueError (the reference's assert admits 0 and then fails on an
    empty list)."""
    from diffusions.ddpm import DDPM
    from scripts.sample_sdedit import edit_time_seq
    d = DDPM(var_type='fixed_small', respace_type='uniform', respace_steps=10)
    assert edit_time_seq(d, 4) == [0, 100, 200, 300]
    assert len(edit_time_seq(d, 9)) == 9
    for bad in (0, -1, 10, 11):
        with pytest.raises(ValueError):
            edit_time_seq(d, bad)


@pytest.mark.parametrize('name', ARCH_NAMES)
def test_recorded_sensitivities(meta, name):
    """Each mechanism is worth >= 100 x the forward tolerance on the fixture inputs (eps: >= 50 x, on x_small), so a
    forward within 1e-4 of the fixture has them right; the reference's own float32 error stays far below it."""
    s = meta[f'{name}_sensitivity']
    for key in ('symmetric_downsample', 'cos_sin_embedding', 'uniform_attention', 'transposed_attention'):
        assert s[key] >= 100 * TOL, (key, s[key])
    assert s['eps_1e-5_on_x_small'] >= 50 * TOL
    assert 0 < meta[f'{name}_small_scale'] <= 0.01
    assert s['reference_f32_vs_f64'] <= TOL / 5 and s['reference_f32_vs_f64_small'] <= TOL / 5


def test_fixture_inputs(meta):
    g = load_golden('pesser')[0]
    for name in ARCH_NAMES:
        assert g[f'{name}_x'].shape == (2, 3, 32, 32) and list(g[f'{name}_t']) == [999, 12]
        np.testing.assert_array_equal(g[f'{name}_x_small'],
                                      np.float32(meta[f'{name}_small_scale']) * g[f'{name}_x'])
    assert g['sdedit_step_noise'].shape == (meta['sdedit']['edit_steps'], 2, 3, 32, 32)
    assert np.abs(g['sdedit_x0']).max() < 1.0


def test_resize_square_is_identity_at_size(tmp_path):
    """resize_square_normalize leaves an image already at img_size untouched ((v / 255 - 0.5) / 0.5 per pixel) and
    maps any other size to img_size x img_size without keeping the aspect ratio."""
    from PIL import Image
    from utils.imagedir import ImageDir, resize_square_normalize
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    x = resize_square_normalize(Image.fromarray(a), 32)
    want = (torch.from_numpy(a).permute(2, 0, 1).float().div(255) - 0.5) / 0.5
    assert x.shape == (3, 32, 32) and torch.equal(x, want)
    wide = Image.fromarray(rng.integers(0, 256, (20, 48, 3), dtype=np.uint8))
    assert resize_square_normalize(wide, 32).shape == (3, 32, 32)
    Image.fromarray(a).save(tmp_path / 'a.png')
    ds = ImageDir(str(tmp_path), 32, transform=resize_square_normalize)
    assert len(ds) == 1 and torch.equal(ds[0], want)


def test_png_normalize_value_range(tmp_path):
    """save_image(normalize=True, value_range=(-1, 1)): clamp to the range, then [-1, 1] -> [0, 255]."""
    from utils.png import read_png_rgb, save_image
    x = torch.tensor([-3.0, -1.0, 0.0, 1.0, 2.0]).view(1, 1, 5).expand(3, 2, 5).contiguous()
    save_image([x, x, x], str(tmp_path / 'g.png'), nrow=3, normalize=True, value_range=(-1, 1))
    img = read_png_rgb(str(tmp_path / 'g.png'))
    assert img.shape == (2 + 4, 3 * 5 + 4 * 2, 3)
    assert list(img[2, 2:7, 0]) == [0, 0, 128, 255, 255]
    assert torch.equal(x[0, 0], torch.tensor([-3.0, -1.0, 0.0, 1.0, 2.0]))   # the caller's tensor is untouched
