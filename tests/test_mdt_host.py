"""Host-side checks of the MDTv2 port (models/mdt/model.py) against the reference fixtures (tests/golden/mdt.npz /
mdt.json, written by tests/golden/make_golden_mdt.py from the reference module itself), and of the biased-attention
reference cases (tests/mdt_attention_ref.py). No GPU.
"""
import ctypes
import hashlib
import math

import pytest
import torch

from models.mdt.model import MDTv2, MDTv2_B_2, MDTv2_L_2, MDTv2_S_2, MDTv2_XL_2, power_cosine_scale, \
    relative_position_index
from tests import attention_ref as ar
from tests import mdt_attention_ref as mr
from utils.synthetic import state_dict_sha256, synthetic_mdt_state_dict

NAMES = ['mdt_a', 'mdt_b', 'mdt_c']


@pytest.mark.parametrize('name', NAMES)
def test_mdt_state_dict_layout_and_param_count(golden, name):
    """Keys, order and shapes (buffers included) equal the reference's own state_dict; dm_mdt_param_count counts its
    float tensors (everything but the int64 relative_position_index buffers)."""
    _, meta = golden('mdt')
    m = MDTv2(**meta['archs'][name])
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == meta[f'{name}_state_dict']
    assert all(v.dtype == (torch.int64 if k.endswith('relative_position_index') else torch.float32)
               for k, v in m.state_dict().items())
    assert m.native_param_count() == len(m.native_param_names())
    assert len(m.native_param_names()) == sum(1 for k, _ in meta[f'{name}_state_dict']
                                              if not k.endswith('relative_position_index'))


@pytest.mark.parametrize('name', NAMES)
def test_mdt_synthetic_weights_match_fixture(golden, name):
    _, meta = golden('mdt')
    m = MDTv2(**meta['archs'][name])
    sd = synthetic_mdt_state_dict(m.state_dict())
    assert state_dict_sha256(sd) == meta[f'{name}_weights_sha256']
    m.load_state_dict(sd)


def test_mdt_factories_and_param_count_xl2():
    from dmhip._lib import MDTArch, load
    a = MDTArch()
    a.input_size, a.patch_size, a.in_channels, a.hidden_size, a.depth, a.num_heads = 32, 2, 4, 1152, 28, 16
    a.mlp_hidden, a.num_classes, a.null_class, a.learn_sigma, a.decode_layer = 4608, 1000, 1, 1, 4
    n = ctypes.c_int()
    assert load().dm_mdt_param_count(ctypes.byref(a), ctypes.byref(n)) == 0
    # 10 leading tensors, 29 blocks of 11, skip_linear.{weight,bias} in 12 + 4 of them, 4 of the final layer
    assert n.value == 10 + 29 * 11 + 16 * 2 + 4
    a.decode_layer = 27   # no en_inblock / en_outblock pair left
    assert load().dm_mdt_param_count(ctypes.byref(a), ctypes.byref(n)) != 0
    for f, (depth, D, heads) in ((MDTv2_S_2, (12, 384, 6)), (MDTv2_B_2, (12, 768, 12))):
        m = f(input_size=8, num_classes=4)
        assert (m.arch['depth'], m.arch['hidden_size'], m.arch['num_heads']) == (depth, D, heads)
        assert m.half_depth == 4 and len(m.de_blocks) == 4 and len(m.sideblocks) == 1
    assert MDTv2_XL_2.__name__ == 'MDTv2_XL_2' and MDTv2_L_2.__name__ == 'MDTv2_L_2'


@pytest.mark.parametrize('W', [8, 16, 32])
def test_rel_index_equals_reference_buffer(golden, W):
    g, meta = golden('mdt')
    idx = relative_position_index(W)
    assert idx.dtype == torch.int64 and idx.shape == (W * W, W * W)
    assert hashlib.sha256(idx.contiguous().numpy().tobytes()).hexdigest() == meta['rel_index_sha256'][str(W)]
    assert torch.equal(idx, mr.rel_index(W))
    if W == 8:
        assert torch.equal(idx, torch.from_numpy(g['rel_index_8']).long())
    assert idx.min() == 0 and idx.max() == (2 * W - 1) ** 2 - 1


def test_power_cosine_scale_matches_reference(golden):
    g, meta = golden('mdt')
    c = meta['cfg']
    t = torch.from_numpy(g['scale_t'])
    assert t.tolist() == [0, 500, 999]
    got = power_cosine_scale(t, c['cfg_scale'], c['diffusion_steps'], c['scale_pow'])
    assert torch.equal(got, torch.from_numpy(g['scale_real']))
    # t = 0: the full scale; t -> steps: 1
    assert abs(got[0].item() - c['cfg_scale']) < 1e-6 and abs(got[2].item() - 1.0) < 1e-6
    want = (c['cfg_scale'] - 1) * 0.5 * (1 - math.cos(math.pi * 0.5 ** c['scale_pow'])) + 1
    assert abs(got[1].item() - want) < 1e-6


def test_enable_mask_raises(golden):
    _, meta = golden('mdt')
    m = MDTv2(**meta['archs']['mdt_c'])
    x = torch.zeros((1, 4, 8, 8))
    with pytest.raises(NotImplementedError):
        m(x, torch.zeros((1, ), dtype=torch.long), torch.zeros((1, ), dtype=torch.long), enable_mask=True)


def test_corrupted_relative_position_index_raises(golden):
    _, meta = golden('mdt')
    m = MDTv2(**meta['archs']['mdt_c'])
    sd = synthetic_mdt_state_dict(m.state_dict())
    m.load_state_dict(sd)
    key = 'en_outblocks.1.attn.rel_pos_bias.relative_position_index'
    bad = dict(sd)
    bad[key] = sd[key].clone()
    bad[key][3, 5] += 1
    with pytest.raises(ValueError, match='relative position index'):
        m.load_state_dict(bad)
    bad[key] = sd[key].t().contiguous()   # i <-> j
    with pytest.raises(ValueError, match='relative position index'):
        m.load_state_dict(bad)


@pytest.mark.parametrize('name', NAMES)
def test_fixture_sensitivity_conditions(golden, name):
    """Each MDT-specific mechanism, broken, moves the reference output by >= 100 x the forward tolerance (checked by
    the generator on the CPU, recorded in mdt.json): a forward test cannot pass with the feature broken."""
    _, meta = golden('mdt')
    s = meta[f'{name}_sensitivity']
    want = {'zero_bias', 'transposed_bias', 'head0_bias', 'no_decoder_pos_embed'}
    a = meta['archs'][name]
    if (a['depth'] - a['decode_layer']) // 2 >= 2:
        want.add('fifo_skips')
    assert set(s) == want
    assert meta['tol'] == 1e-4
    for k, v in s.items():
        assert v >= 100 * meta['tol'], (k, v)


def test_latent_wrapper_and_config_targets():
    """configs/mdt_xl2_256.yaml's targets resolve; MDT is a BaseLatent with the lazy VAE of models/dit/dit.py."""
    import os
    from models.base_latent import BaseLatent
    from models.mdt.autoencoder import AutoEncoderKL
    from models.mdt.mdt import MDT
    from models.dit.autoencoder import AutoEncoderKL as DitKL
    assert AutoEncoderKL is DitKL and issubclass(MDT, BaseLatent)
    import models
    cfg = open(os.path.join(os.path.dirname(models.__file__), '..', 'configs', 'mdt_xl2_256.yaml')).read()
    for target in ('models.mdt.mdt.MDT', 'models.mdt.autoencoder.AutoEncoderKL', 'models.mdt.model.MDTv2'):
        assert f'target: {target}' in cfg


# ---------------------------------------------------------------- tests/mdt_attention_ref.py
HOST_SHAPES = mr.SHAPES[:3]   # the L = 1024 case's references are left to the GPU test's one computation


@pytest.mark.parametrize('dist', mr.DISTS)
@pytest.mark.parametrize('shape', HOST_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bias_cases_bound_not_vacuous(shape, dist):
    """torch float32 on the decoded operands stays within the bound with margin (<= bound / 2 by construction, and
    the bound itself is fp32-sized: <= 2^-14 max|ref|), and the kernel's arithmetic restated in fp32 (bias added
    before the running maximum) meets it."""
    c = mr.case(shape, dist)
    assert c['e32'] > 0 and c['e32'] <= 0.5 * c['bound']
    assert c['bound'] <= 2.0 ** -14 * c['scale'], (c['bound'], c['scale'])
    emu = mr.flash_bias_emulation(c['pq'], c['pk'], c['pv'], mr.kernel_table(c['table']), c['W'])
    err = (emu.double() - c['ref']).abs().max().item()
    assert torch.isfinite(emu).all()
    assert err <= c['bound'], (err, c['e32'], c['bound'])


def test_bias_cases_decide_the_result():
    """The cases are sensitive to what they are meant to catch: dropping the bias, transposing it or using another
    head's table moves the float64 result by far more than the bound; in 'cross' the raw scores' maximum and the
    biased maximum lie in different key blocks."""
    shape = mr.SHAPES[0]
    for dist in ('rand', 'cross'):
        c = mr.case(shape, dist)
        qd, kd, vd = c['dec']
        b = mr.bias_matrix(c['table'], c['W'])
        for other in (torch.zeros_like(b), b.transpose(-1, -2), b.roll(1, 0) if dist == 'rand' else b * 0.5):
            moved = (mr.attention_bias_f64(qd, kd, vd, other) - c['ref']).abs().max().item()
            assert moved >= 1e3 * c['bound'], (dist, moved, c['bound'])
    c = mr.case((1, 2, 256, 72), 'cross')
    qd, kd, vd = c['dec']
    s = qd @ kd.transpose(-1, -2)
    raw, biased = s.argmax(-1) // ar.KB, (s + mr.bias_matrix(c['table'], c['W']).double()[None]).argmax(-1) // ar.KB
    assert (raw != biased).float().mean() > 0.9


@pytest.mark.parametrize('shape', HOST_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_bias_select_case(shape):
    """'select': every query's winner is ahead by >= 128 nats, winners differ between heads, and the emulation
    returns v[pi] to 2^-20 max|v|."""
    c = mr.case(shape, 'select')
    b = mr.bias_matrix(c['table'], c['W'])
    top2 = b.topk(2, dim=-1).values
    assert (top2[..., 0] - top2[..., 1]).min() >= 128.0
    assert not torch.equal(c['pi'][0], c['pi'][1])
    emu = mr.flash_bias_emulation(c['pq'], c['pk'], c['pv'], mr.kernel_table(c['table']), c['W'])
    want = mr.selected_rows(c['v'], c['pi'])
    assert (emu - want).abs().max().item() <= 2.0 ** -20 * c['v'].abs().max().item()
