"""The contract every native model handle carries through csrc/exec_core.h (the shared forward driver, range fallback
and C ABI bodies), stated once over the five handles: dm_unet, dm_dit, dm_mdt, dm_vae_decoder, dm_vae_encoder.

Models: the smallest each handle's own test file builds -- the 'tiny' UNet of tests/golden/forward.json (B = 2 at
16 x 16), dit_tiny and mdt_c of tests/golden/dit.json / mdt.json, the T1 decoder and E1 encoder of tests/vae_ref.py /
vae_enc_ref.py (B = 1).

The input that leaves the fp16 range ("hot"): for the conv nets the ordinary input times 1e6, as
tests/test_gpu_parity.py::test_range_fallback_not_sticky scales it -- the raw-input consumers (shortcut K segments,
up / downsample convs) then read ~1e5 .. 1e6 > 65504. DiT and MDT normalise every token GEMM's input, so no scaling of
x reaches an fp16x2 operand; there class 3's row of the label table is scaled by 1e5 before the handle is made and
the hot input is label 3: SiLU(t_emb + y_emb) ~ 1e4 is the adaLN GEMM's A operand (times 2^6 > 65504). Labels 1 / 2
stay ordinary. Every equality below is bit for bit: a fallback pass runs the plan the fallback arithmetic builds.
"""
import ctypes

import pytest
import torch

import dmhip
from dmhip._lib import CONV_MATH, DM_ERR_ARG, DM_ERR_STATE, DM_OK, check, load, stream_handle

pytestmark = pytest.mark.gpu

FP32, FP16X2, BF16X3 = CONV_MATH['fp32'], CONV_MATH['fp16x2'], CONV_MATH['bf16x3']
NAME = {v: k for k, v in CONV_MATH.items()}


class Case:
    """One handle: `run(inp)` is a forward through the model's Python surface, `cold` / `hot` / `other_b` its inputs."""
    deferred = False
    setter, getter = '_set_math', '_get_math'
    legal, illegal, fallback = (FP32, FP16X2, BF16X3), (7, -1), BF16X3


def _unet(cuda, golden):
    from models.unet import UNet
    from utils.synthetic import init_synthetic_
    _, meta = golden('forward')
    m = UNet(**meta['archs']['tiny']).eval()
    init_synthetic_(m)
    m = m.to(cuda)
    g = torch.Generator().manual_seed(6)
    x = torch.randn((3, 3, 16, 16), generator=g).to(cuda)
    t = torch.tensor([30, 800, 410], device=cuda)
    c = Case()
    c.abi, c.deferred = 'dm_unet', True
    c.setter, c.getter = '_set_conv_math', '_get_conv_math'
    c.handle = lambda: m.native_handle(cuda)
    c.run = lambda inp: m(*inp)
    c.cold, c.hot, c.other_b = (x[:2], t[:2]), (x[:2] * 1e6, t[:2]), (x, t)
    c.numel = lambda: sum(p.numel() for p in m._param_list)
    c.keep = m
    return c


def _token_model(cuda, golden, mdt):
    from utils.synthetic import init_synthetic_
    if mdt:
        from models.mdt.model import MDTv2
        m = MDTv2(**golden('mdt')[1]['archs']['mdt_c']).eval()
    else:
        from models.dit.model import DiT
        m = DiT(**golden('dit')[1]['archs']['dit_tiny']).eval()
    init_synthetic_(m)
    with torch.no_grad():
        m.state_dict(keep_vars=True)['y_embedder.embedding_table.weight'][3].mul_(1e5)
    m = m.to(cuda)
    g = torch.Generator().manual_seed(8)
    x = torch.randn((2, 4, 8, 8), generator=g).to(cuda)
    t = torch.tensor([500, 20], device=cuda)
    c = Case()
    c.abi, c.deferred = 'dm_mdt' if mdt else 'dm_dit', True
    c.legal, c.illegal, c.fallback = (FP32, FP16X2), (BF16X3, 7, -1), FP32
    c.handle = lambda: m.native_handle(cuda)
    c.run = lambda inp: m(*inp)
    c.cold = (x[:1], t[:1], torch.tensor([1], device=cuda))
    c.hot = (x[:1], t[:1], torch.tensor([3], device=cuda))
    c.other_b = (x, t, torch.tensor([1, 2], device=cuda))
    c.numel = lambda: sum(p.numel() for p in m._param_list)
    c.keep = m
    return c


def _vae(cuda, encoder):
    from models.dit.autoencoder import AutoEncoderKL
    from tests import vae_enc_ref, vae_ref
    c = Case()
    if encoder:
        sd = dict(vae_enc_ref.weights('E1'))
        sd.update(vae_ref.recipe_state_dict(vae_ref.decoder_shapes(vae_enc_ref.CONFIGS['E1'])))
        m = AutoEncoderKL.from_state_dict(vae_enc_ref.diffusers_config('E1'), sd)
        x = vae_enc_ref.images('E1', 11).to(cuda)   # [2, 3, 32, 32], uniform in [-1, 1]
        c.abi = 'dm_vae_encoder'
        c.handle = lambda: m.encoder_handle(cuda)
        c.run = lambda inp: m.encode(inp).latent_dist.parameters
        c.numel = lambda: sum(p.numel() for p in m.enc_params)
    else:
        m = AutoEncoderKL.from_state_dict(vae_ref.diffusers_config('T1'), vae_ref.weights('T1'))
        x = torch.randn(vae_ref.CONFIGS['T1']['z_shape'], generator=torch.Generator().manual_seed(7)).to(cuda)
        c.abi = 'dm_vae_decoder'
        c.handle = lambda: m.native_handle(cuda)
        c.run = lambda inp: m.decode(inp).sample
        c.numel = lambda: sum(p.numel() for p in m.params)
    assert x.shape[0] == 2
    c.cold, c.hot, c.other_b = x[:1], x[:1] * 1e6, x
    c.keep = m
    return c


MAKE = {
    'dm_unet': _unet,
    'dm_dit': lambda cuda, golden: _token_model(cuda, golden, False),
    'dm_mdt': lambda cuda, golden: _token_model(cuda, golden, True),
    'dm_vae_decoder': lambda cuda, golden: _vae(cuda, False),
    'dm_vae_encoder': lambda cuda, golden: _vae(cuda, True),
}


@pytest.mark.parametrize('abi', list(MAKE))
def test_exec_contract(cuda, golden, abi):
    L = load()
    c = MAKE[abi](cuda, golden)
    h = c.handle()
    fn = lambda name: getattr(L, abi + name)   # noqa: E731

    def run(inp):
        out = c.run(inp)
        torch.cuda.synchronize()
        return out.cpu()

    def get_math():
        k = ctypes.c_int()
        check(fn(c.getter)(h, ctypes.byref(k)), abi + c.getter)
        return k.value

    def stats():
        return dmhip.range_stats(h, abi)

    def plans():
        return dmhip.plan_stats(h, abi)

    # --- profile: no plan before the first forward
    assert fn('_profile')(h, 1) == DM_ERR_STATE
    n_ops = ctypes.c_int()
    assert fn('_profile_count')(h, ctypes.byref(n_ops)) == DM_ERR_STATE
    assert plans() == (0, 0) and stats() == (0, 'fp16x2') and get_math() == FP16X2

    # --- plan cache: one plan per shape
    first = run(c.cold)
    assert torch.isfinite(first).all()
    assert torch.equal(run(c.cold), first)
    assert plans() == (1, 1)
    run(c.other_b)
    assert plans() == (2, 2)
    assert fn('_profile_count')(h, ctypes.byref(n_ops)) == DM_OK and n_ops.value > 0
    assert len(dmhip.unet_profile_read(h, abi)) == n_ops.value

    # --- memory: the fp32 arena holds every parameter (its split copies come on top), the plans a workspace
    wb, sb = ctypes.c_int64(), ctypes.c_int64()
    assert fn('_memory')(h, ctypes.byref(wb), ctypes.byref(sb)) == DM_OK
    assert wb.value >= 4 * c.numel() and sb.value > 0

    # --- arithmetic: a different kind drops the cached plans, the next forward rebuilds; the same kind keeps them
    assert fn(c.setter)(h, FP16X2) == DM_OK and plans() == (2, 2)
    for kind in c.legal:
        if kind == FP16X2:
            continue
        assert fn(c.setter)(h, kind) == DM_OK
        assert get_math() == kind and plans()[1] == 0 and stats() == (0, NAME[kind])
        b0 = plans()[0]
        assert torch.isfinite(run(c.cold)).all()
        assert plans() == (b0 + 1, 1)
        for bad in c.illegal:
            assert fn(c.setter)(h, bad) == DM_ERR_ARG
        assert get_math() == kind and plans() == (b0 + 1, 1)

    # --- range fallback: the flagged forward equals the fallback arithmetic's own, counts once, and is not sticky
    assert fn(c.setter)(h, c.fallback) == DM_OK
    want = run(c.hot)
    assert torch.isfinite(want).all()
    assert stats() == (0, NAME[c.fallback])
    assert fn(c.setter)(h, FP16X2) == DM_OK and plans()[1] == 0
    got = run(c.hot)
    assert torch.equal(got, want)
    assert stats() == (1, 'fp16x2') and get_math() == FP16X2
    assert torch.equal(run(c.cold), first)
    assert stats() == (1, 'fp16x2')

    if not c.deferred:
        return

    # --- deferred mode: the flagged forward is not re-run; the poll reports it and switches to the fallback
    flagged = ctypes.c_int(-1)
    st = stream_handle(cuda)
    assert fn('_set_range_deferred')(h, 1) == DM_OK
    assert fn('_range_poll')(h, st, ctypes.byref(flagged)) == DM_OK and flagged.value == 0
    raw = run(c.hot)
    assert stats() == (1, 'fp16x2')                 # no second pass
    assert not torch.equal(raw, want)               # (what fp16x2 made of it: the caller discards it)
    assert fn('_range_poll')(h, st, ctypes.byref(flagged)) == DM_OK and flagged.value == 1
    assert stats() == (2, NAME[c.fallback]) and get_math() == FP16X2
    assert torch.equal(run(c.hot), want)            # the caller's re-run
    assert fn('_range_poll')(h, st, ctypes.byref(flagged)) == DM_OK and flagged.value == 0
    assert fn('_range_fallback')(h, 0) == DM_OK
    assert stats() == (2, 'fp16x2')
    assert fn('_set_range_deferred')(h, 0) == DM_OK
    assert torch.equal(run(c.cold), first)
    assert stats() == (2, 'fp16x2')
