"""Host side of the VAE latent decoder (no GPU): the tests' reference against the fixture generated from the
reference module, the state-dict key mapping of the three layouts, config validation, the safetensors reader and the
hub-id behaviour."""
import json
import os

import numpy as np
import pytest
import torch

from tests import vae_ref
from models.dit import autoencoder as ae
from utils.safetensors_io import load_safetensors


@pytest.mark.parametrize('name', ['T1', 'T2'])
def test_vae_ref_matches_reference_fixture(golden, name):
    """tests/vae_ref.py float32 == the reference AutoEncoderKL.decode (tests/golden/vae.npz) within the bound
    tests/test_oracle_golden.py uses for network forwards (oneDNN's summation order varies with the thread count)."""
    g, meta = golden('vae')
    sd = vae_ref.weights(name)
    assert vae_ref.sha256(sd) == meta[name]['sha256']
    assert list(sd) == meta[name]['keys'] == list(vae_ref.decoder_shapes(vae_ref.CONFIGS[name]))
    z = vae_ref.latents(name)
    assert np.array_equal(z.numpy(), g[f'{name}_z'])
    with torch.no_grad():
        out = vae_ref.decode(sd, z)
    err = np.abs(out.numpy() - g[f'{name}_out']).max()
    print(f'{name}: vae_ref vs fixture {err:.3e}')
    assert err <= 2e-6


def test_recipe_norms_are_not_trivial():
    sd = vae_ref.weights('T1')
    for k, v in sd.items():
        if '.norm' in k and k.endswith('weight'):
            assert 0.5 <= v.min() and v.max() <= 1.5 and v.std() > 0.1, k
        elif '.norm' in k:
            assert -0.5 <= v.min() and v.max() <= 0.5 and v.std() > 0.1, k
        elif v.ndim == 1:
            assert v.abs().max() <= 0.1 and v.abs().max() > 0.05, k


def test_abi_order_is_reference_state_dict_order(golden):
    _, meta = golden('vae')
    for name in ('T1', 'T2'):
        arch = ae.arch_from_config(vae_ref.diffusers_config(name))
        assert [n for n, _ in ae.abi_param_names(arch)] == meta[name]['keys']
        assert arch['ch'] == meta[name]['ch'] and list(arch['ch_mult']) == meta[name]['ch_mult']
        assert arch['num_res_blocks'] == meta[name]['num_res_blocks']


@pytest.mark.parametrize('name', ['T1', 'T3'])
def test_three_key_layouts_give_identical_abi_parameters(name):
    arch = ae.arch_from_config(vae_ref.diffusers_config(name))
    sd = vae_ref.weights(name)
    lists = [ae.abi_params(arch, sd), ae.abi_params(arch, vae_ref.to_diffusers(sd)),
             ae.abi_params(arch, vae_ref.to_diffusers(sd, legacy_attention=True))]
    want = ae.abi_param_names(arch)
    for got in lists:
        assert len(got) == len(want) == len(sd)
        for t, ref, (n, shape) in zip(got, lists[0], want):
            assert t.dtype == torch.float32 and t.is_contiguous()
            assert torch.equal(t, ref), n
            assert torch.equal(t.reshape(-1), sd[n].reshape(-1)), n
            if n.startswith('decoder.mid.attn_1.') and n.endswith('.weight') and '.norm.' not in n:
                assert tuple(t.shape) == shape[:2]  # [C][C] matrices


def test_loader_rejects_missing_surplus_and_wrong_size():
    arch = ae.arch_from_config(vae_ref.diffusers_config('T1'))
    sd = vae_ref.to_diffusers(vae_ref.weights('T1'))
    miss = dict(sd)
    del miss['decoder.mid_block.attentions.0.to_k.weight']
    with pytest.raises(ValueError, match=r'missing keys.*decoder\.mid\.attn_1\.k\.weight'):
        ae.abi_params(arch, miss)
    extra = dict(sd)
    extra['decoder.up_blocks.0.attentions.0.to_q.weight'] = torch.zeros(4, 4)
    with pytest.raises(ValueError, match=r'unexpected keys.*decoder\.up_blocks\.0\.attentions\.0\.to_q\.weight'):
        ae.abi_params(arch, extra)
    wrong = dict(sd)
    wrong['decoder.conv_out.bias'] = torch.zeros(5)
    with pytest.raises(ValueError, match=r'decoder\.conv_out\.bias'):
        ae.abi_params(arch, wrong)


@pytest.mark.parametrize('change, word', [
    (dict(block_out_channels=[48, 96]), 'block_out_channels'),
    (dict(block_out_channels=[64, 96]), 'block_out_channels'),
    (dict(norm_num_groups=16), 'norm_num_groups'),
    (dict(act_fn='relu'), 'act_fn'),
    (dict(latent_channels=16), 'latent_channels'),
    (dict(out_channels=12), 'out_channels'),
    (dict(layers_per_block=-1), 'layers_per_block'),
    (dict(up_block_types=['UpDecoderBlock2D', 'AttnUpDecoderBlock2D', 'UpDecoderBlock2D']), 'up_block_types'),
    (dict(mid_block_add_attention=False), 'mid_block_add_attention'),
    (dict(attention_head_dim=8), 'attention_head_dim'),
])
def test_unsupported_config_names_the_entry(change, word):
    cfg = vae_ref.diffusers_config('T1')
    cfg.update(change)
    with pytest.raises(ValueError, match=word):
        ae.arch_from_config(cfg)
    with pytest.raises(ValueError, match=word):
        ae.AutoEncoderKL.from_state_dict(cfg, vae_ref.weights('T1'))


def _write_with_package_or_local(path, sd):
    try:
        from safetensors.torch import save_file
    except ImportError:
        vae_ref.write_safetensors(path, sd)
        return 'local'
    save_file({k: v.contiguous() for k, v in sd.items()}, path)
    return 'package'


def test_safetensors_reader_round_trip(tmp_path):
    g = torch.Generator().manual_seed(3)
    sd = {'a.weight': torch.randn(5, 3, 3, 3, generator=g), 'b': torch.randn(7, generator=g),
          'scalar': torch.tensor(2.5), 'empty': torch.zeros(0, 4)}
    path = str(tmp_path / 'x.safetensors')
    print('writer:', _write_with_package_or_local(path, sd))
    got = load_safetensors(path)
    assert sorted(got) == sorted(sd)
    for k, v in sd.items():
        assert got[k].dtype == torch.float32 and got[k].shape == v.shape and torch.equal(got[k], v), k
    # half-precision storage and the metadata entry
    import struct
    h16 = torch.randn(4, 6, generator=g).to(torch.float16)
    b16 = torch.randn(3, 2, generator=g).to(torch.bfloat16)
    blob = h16.numpy().tobytes() + b16.view(torch.int16).numpy().tobytes()
    header = json.dumps({'__metadata__': {'format': 'pt'},
                         'h': dict(dtype='F16', shape=[4, 6], data_offsets=[0, 48]),
                         'b': dict(dtype='BF16', shape=[3, 2], data_offsets=[48, 60])}).encode()
    p2 = str(tmp_path / 'y.safetensors')
    with open(p2, 'wb') as f:
        f.write(struct.pack('<Q', len(header)) + header + blob)
    got = load_safetensors(p2)
    assert torch.equal(got['h'], h16) and torch.equal(got['b'], b16)
    with open(p2, 'wb') as f:
        f.write(struct.pack('<Q', len(header)) + header + blob[:-2])
    with pytest.raises(ValueError, match='outside the file'):
        load_safetensors(p2)


def test_checkpoint_directory_loads_on_the_host(tmp_path):
    """config.json + safetensors in the diffusers layout -> the ABI-ordered parameters (the native decoder itself
    is created on first decode, on the latents' device)."""
    vae_ref.write_checkpoint_dir(str(tmp_path / 'vae'), 'T1')
    m = ae.AutoEncoderKL(str(tmp_path / 'vae'), decode_batch=2)
    arch = ae.arch_from_config(vae_ref.diffusers_config('T1'))
    for t, ref in zip(m.params, ae.abi_params(arch, vae_ref.weights('T1'))):
        assert torch.equal(t, ref)
    assert m.upscale == 4 and m.decode_batch == 2
    with pytest.raises(RuntimeError, match='ROCm'):
        m.decode(torch.zeros(1, 4, 8, 8))
    os.remove(tmp_path / 'vae' / 'diffusion_pytorch_model.safetensors')
    torch.save(vae_ref.to_diffusers(vae_ref.weights('T1'), legacy_attention=True),
               tmp_path / 'vae' / 'diffusion_pytorch_model.bin')
    m2 = ae.AutoEncoderKL(str(tmp_path / 'vae'))
    for t, ref in zip(m2.params, m.params):
        assert torch.equal(t, ref)


def test_hub_id_still_raises_not_implemented():
    with pytest.raises(NotImplementedError):
        ae.AutoEncoderKL('stabilityai/sd-vae-ft-ema')
    with pytest.raises(NotImplementedError):
        ae.AutoEncoderKL(from_pretrained='stabilityai/sd-vae-ft-ema')
    with pytest.raises(NotImplementedError):
        ae.AutoEncoderKL()


def test_param_count_and_argument_errors_without_a_gpu():
    """dm_vae_decoder_param_count equals the reference registration; bad channels, levels and a parameter count off
    by one are refused with a message before anything is launched."""
    import ctypes
    import dmhip
    from dmhip._lib import DM_ERR_ARG, VaeArch

    def arch(ch=32, mult=(1, 2, 4), nrb=1):
        a = VaeArch()
        a.z_channels, a.out_channels, a.ch, a.n_levels, a.num_res_blocks = 4, 3, ch, len(mult), nrb
        for i, m in enumerate(mult):
            a.ch_mult[i] = m
        a.norm_groups, a.norm_eps, a.post_quant = 32, 1e-6, 1
        return a
    L = dmhip.load()
    n = ctypes.c_int()
    for name, c in vae_ref.CONFIGS.items():
        assert L.dm_vae_decoder_param_count(ctypes.byref(arch(c['ch'], c['ch_mult'], c['num_res_blocks'])),
                                            ctypes.byref(n)) == 0
        assert n.value == len(vae_ref.decoder_shapes(c)), name
    assert L.dm_vae_decoder_param_count(ctypes.byref(arch(ch=48)), ctypes.byref(n)) == DM_ERR_ARG
    assert b'multiple of 32' in L.dm_last_error()
    assert L.dm_vae_decoder_param_count(ctypes.byref(arch()), ctypes.byref(n)) == 0
    h = ctypes.c_void_p()
    ptrs = (ctypes.c_void_p * 1)()
    nums = (ctypes.c_int64 * 1)()
    assert L.dm_vae_decoder_create(ctypes.byref(arch()), ptrs, nums, n.value - 1, None, ctypes.byref(h)) == DM_ERR_ARG
    assert b'parameter tensors' in L.dm_last_error() and not h.value
