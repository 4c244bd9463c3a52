"""The conv-half option of the conv UNets (dm_unet_set_conv_half) at the model level, on the fixtures'
small models: 'tiny' (tests/golden/forward.json), 'tiny_updown' (adagn.json), 'adm_tiny' (adm.json), 'pesser_a'
(pesser.json) -- accuracy against a host emulation of the same roundings, plan routing, the switch contract, batch
invariance, the range fallback with and without the deferred poll, and the Python / script surface.

The option has no fp32 parity to assert. What is asserted instead (the rule of tests/test_gpu_dit_fp16.py): the
engine's error against the fp32 golden (err16) is at most twice the error of a HOST forward that makes the same
roundings at the same points (emu16: the oracle module's forward in float64 with torch.nn.functional.conv2d replaced
from tests/conv_h16_ref.py on exactly the covered layers and the 1x1 shortcuts of covered conv2s), and err16 exceeds
the fp16x2 error, so the option is the cheaper arithmetic.
"""
import ctypes
import os

import pytest
import torch

import dmhip
from dmhip._lib import DM_ERR_ARG, DM_OK, load, stream_handle
from tests import conv_h16_ref as cr

pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'diffusion-models-pytorch_amd',
                       'configs')
NAMES = list(cr.MODELS)


def _class(family):
    if family == 'unet':
        from models.unet import UNet as M
    elif family == 'adagn':
        from models.unet_categorial_adagn import UNetCategorialAdaGN as M
    elif family == 'adm':
        from models.adm.unet import UNetModel as M
    else:
        from models.pesser.model import Model as M
    return M


def _model(name, golden, scale_first=None):
    """-> (model on the host, arch, golden arrays, family)"""
    from utils.synthetic import init_synthetic_
    gfile, family = cr.MODELS[name]
    g, meta = golden(gfile)
    arch = dict(meta['archs'][name])
    m = _class(family)(**arch).eval()
    init_synthetic_(m)
    if scale_first is not None:
        with torch.no_grad():
            for k, v in m.state_dict(keep_vars=True).items():
                if k in ('first_conv.weight', 'input_blocks.0.0.weight', 'conv_in.weight'):
                    v.mul_(scale_first)
    return m, arch, g, family


def _inputs(g, name, cuda):
    x = torch.from_numpy(g[f'{name}_x']).to(cuda)
    t = torch.from_numpy(g[f'{name}_t']).to(cuda)
    y = torch.from_numpy(g[f'{name}_labels']).to(cuda) if f'{name}_labels' in g else None
    key = [k for k in (f'{name}_out_y', f'{name}_out', f'{name}_y') if k in g][0]
    return (x, t) if y is None else (x, t, y), torch.from_numpy(g[key]).double()


def _labels(h):
    return [op['label'] for op in dmhip.unet_profile_read(h)]


def _run(m, inp):
    out = m(*inp)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize('name', NAMES)
def test_accuracy_and_routing(cuda, golden, report, name):
    m, arch, g, family = _model(name, golden)
    m = m.to(cuda)
    h = m.native_handle(torch.device(cuda))
    inp, want = _inputs(g, name, cuda)
    out_x2 = _run(m, inp).double()
    labels_x2 = _labels(h)
    assert not [s for s in labels_x2 if s.startswith('conv_h16')], labels_x2
    assert m.set_conv_half(True) is True and dmhip.unet_conv_half(h) is True
    out16 = _run(m, inp).double()
    labels = _labels(h)

    # --- the emulation of the same roundings, and the number of covered convs it met
    emu, n_cov = cr.host_forward(family, m.state_dict(), arch, inp[0], inp[1], inp[2] if len(inp) == 3 else None,
                                 h16=True)
    assert n_cov > 0

    # --- routing: every covered conv on the new kernel behind an image pass, no Winograd kernel, the rest as before
    kern = [s for s in labels if s.startswith('conv_h16_kernel')]
    assert len(kern) == n_cov, (n_cov, labels)
    assert labels.count('conv_h16_image') == n_cov, labels
    for i, s in enumerate(labels):
        if s.startswith('conv_h16_kernel'):
            assert labels[i - 1] == 'conv_h16_image', (i, labels)
    assert not [s for s in labels if s.startswith('conv_wino')], labels

    # the two plans walk the same ops: without the image passes and the GroupNorm statistics / table launches (a
    # covered conv takes finalized tables, and its epilogue has its own statistics rule) they pair up one to one, and
    # differ exactly where a covered conv replaced an fp16x2 3x3 kernel
    aux = ('conv_h16_image', 'gn_finalize', 'gn_partial')
    seq, seq_x2 = [s for s in labels if s not in aux], [s for s in labels_x2 if s not in aux]
    assert len(seq) == len(seq_x2), (seq, seq_x2)
    swapped = [(a, b) for a, b in zip(seq, seq_x2) if a != b]
    assert len(swapped) == n_cov, swapped
    for a, b in swapped:
        assert a.startswith('conv_h16_kernel') and b.startswith(('conv_wino', 'conv_k32', 'conv_patch3')), (a, b)

    # --- accuracy
    err16 = (out16 - want).abs().max().item()
    emu16 = (emu - want).abs().max().item()
    direct = (out16 - emu).abs().max().item()
    err_x2 = (out_x2 - want).abs().max().item()
    print(f'{name} conv-half: err16 {err16:.3e} emu16 {emu16:.3e} engine-to-emulation {direct:.3e} fp16x2 {err_x2:.3e} '
          f'({n_cov} covered convs)')
    report(f'{name}_h16_err16_maxabs_vs_golden', err16)
    report(f'{name}_h16_emu16_maxabs_vs_golden', emu16)
    report(f'{name}_h16_engine_to_emulation_maxabs', direct)
    report(f'{name}_h16_fp16x2_maxabs_vs_golden', err_x2)
    assert err16 <= 2.0 * emu16, (err16, emu16)
    assert err16 > err_x2, (err16, err_x2)


def test_switch_contract(cuda, golden):
    L = load()
    m, arch, g, _ = _model('tiny', golden)
    assert m.set_conv_half(True) is True          # before the handle exists: applied at creation
    m = m.to(cuda)
    h = m.native_handle(torch.device(cuda))
    assert dmhip.unet_conv_half(h) is True
    assert dmhip.unet_conv_half(h, False) is False
    fresh, _, _, _ = _model('tiny', golden)
    fresh = fresh.to(cuda)                        # (a later .to() would re-pack the model: a new handle)
    hf = fresh.native_handle(torch.device(cuda))
    assert dmhip.unet_conv_half(hf) is False      # the default is off
    inp, _ = _inputs(g, 'tiny', cuda)
    off = _run(m, inp)
    assert dmhip.plan_stats(h) == (1, 1)
    assert dmhip.unet_conv_half(h, False) is False and dmhip.plan_stats(h) == (1, 1)   # the same value keeps the plans
    assert dmhip.unet_conv_half(h, True) is True and dmhip.plan_stats(h) == (1, 0)     # a different one drops them
    on = _run(m, inp)
    assert dmhip.plan_stats(h) == (2, 1) and not torch.equal(on, off)
    k = ctypes.c_int(-1)
    assert L.dm_unet_get_conv_half(h, ctypes.byref(k)) == DM_OK and k.value == 1
    for bad in (2, -1):
        assert L.dm_unet_set_conv_half(h, bad) == DM_ERR_ARG
    assert dmhip.unet_conv_half(h) is True and dmhip.plan_stats(h) == (2, 1)
    # not a fourth kind of the arithmetic: DM_MATH_FP16 stays the token models'
    assert L.dm_unet_set_conv_math(h, 1) == DM_ERR_ARG
    assert 'DM_MATH_FP16 is for the token models' in L.dm_last_error().decode()
    assert dmhip.unet_conv_math(h) == 'fp16x2' and dmhip.range_stats(h) == (0, 'fp16x2')
    # fp32 and bf16x3 plans are unchanged by the switch: bit-equal outputs, no conv_h16 launch
    for kind in ('fp32', 'bf16x3'):
        dmhip.unet_conv_math(h, kind)
        with_switch = _run(m, inp)
        assert not [s for s in _labels(h) if s.startswith('conv_h16')]
        dmhip.unet_conv_half(h, False)
        assert torch.equal(_run(m, inp), with_switch), kind
        dmhip.unet_conv_half(h, True)
    dmhip.unet_conv_math(h, 'fp16x2')
    assert torch.equal(_run(m, inp), on)
    # the image planes are plan workspace
    wb, sb0, sb1 = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert L.dm_unet_memory(h, ctypes.byref(wb), ctypes.byref(sb1)) == DM_OK
    _run(fresh, inp)
    assert fresh.native_handle(torch.device(cuda)) == hf
    assert L.dm_unet_memory(hf, ctypes.byref(wb), ctypes.byref(sb0)) == DM_OK
    assert sb1.value > sb0.value > 0              # (the conv-half plan's two planes come on top)


@pytest.mark.parametrize('name', ['tiny', 'pesser_a'])
def test_batch_invariance(cuda, golden, name):
    m, arch, g, _ = _model(name, golden)
    m.set_conv_half(True)
    m = m.to(cuda)
    inp, _ = _inputs(g, name, cuda)
    gen = torch.Generator().manual_seed(12)
    x3 = torch.randn((3, *inp[0].shape[1:]), generator=gen).to(cuda)
    t3 = torch.tensor([500, 20, 777], device=cuda)
    o3 = _run(m, (x3, t3))
    for i in range(3):
        o1 = _run(m, (x3[i:i + 1], t3[i:i + 1]))
        assert torch.equal(o3[i:i + 1], o1), i
        assert not torch.equal(o3[(i + 1) % 3:(i + 1) % 3 + 1], o1)
    assert [s for s in _labels(m.native_handle(torch.device(cuda))) if s.startswith('conv_h16_kernel')]


def test_range_fallback_and_deferred_poll(cuda, golden):
    """The first conv scaled by 1e5: the raw-input consumers read values beyond 65504. The flagged forward is the
    bf16x3 arithmetic's own, counted once; the next forward is conv-half again."""
    L = load()
    hot, arch, g, _ = _model('tiny', golden, scale_first=1e5)
    hot = hot.to(cuda)
    h = hot.native_handle(torch.device(cuda))
    inp, _ = _inputs(g, 'tiny', cuda)
    cold = (inp[0] * 1e-5, inp[1])                 # the same model on an input that stays in range
    dmhip.unet_conv_math(h, 'bf16x3')
    want = _run(hot, inp)
    assert torch.isfinite(want).all() and dmhip.range_stats(h) == (0, 'bf16x3')
    dmhip.unet_conv_math(h, 'fp16x2')
    assert hot.set_conv_half(True) is True
    got = _run(hot, inp)
    assert torch.equal(got, want)
    assert dmhip.range_stats(h) == (1, 'fp16x2') and dmhip.unet_conv_half(h) is True     # once, not sticky
    first = _run(hot, cold)
    assert dmhip.range_stats(h) == (1, 'fp16x2')
    assert [s for s in _labels(h) if s.startswith('conv_h16_kernel')]
    fresh, _, _, _ = _model('tiny', golden, scale_first=1e5)
    fresh.set_conv_half(True)
    fresh = fresh.to(cuda)
    assert torch.equal(_run(fresh, cold), first)
    assert dmhip.range_stats(fresh.native_handle(torch.device(cuda))) == (0, 'fp16x2')

    # deferred mode: no second pass; the poll reports the flag and switches to the fallback until told otherwise
    flagged = ctypes.c_int(-1)
    st = stream_handle(cuda)
    assert L.dm_unet_set_range_deferred(h, 1) == DM_OK
    assert L.dm_unet_range_poll(h, st, ctypes.byref(flagged)) == DM_OK and flagged.value == 0
    raw = _run(hot, inp)
    assert dmhip.range_stats(h) == (1, 'fp16x2') and not torch.equal(raw, want)
    assert L.dm_unet_range_poll(h, st, ctypes.byref(flagged)) == DM_OK and flagged.value == 1
    assert dmhip.range_stats(h) == (2, 'bf16x3') and dmhip.unet_conv_half(h) is True
    assert torch.equal(_run(hot, inp), want)
    assert L.dm_unet_range_poll(h, st, ctypes.byref(flagged)) == DM_OK and flagged.value == 0
    assert L.dm_unet_range_fallback(h, 0) == DM_OK and dmhip.range_stats(h) == (2, 'fp16x2')
    assert L.dm_unet_set_range_deferred(h, 0) == DM_OK
    assert torch.equal(_run(hot, cold), first) and dmhip.range_stats(h) == (2, 'fp16x2')


def test_ddim_steps_and_combined(cuda, golden, report):
    """Three DDIM steps on 'tiny' stay finite (the distance to the fp16x2 trajectory is reported, not asserted);
    UNetCombined hands the switch to both halves."""
    from diffusions import DDIM
    from models.adm.unet_combined import UNetCombined
    g, _ = golden('forward')
    last = {}
    for half in (False, True):
        m, arch, _, _ = _model('tiny', golden)
        m.set_conv_half(half)
        m = m.to(cuda)
        init = torch.randn((2, 3, 16, 16), generator=torch.Generator().manual_seed(4)).to(cuda)
        d = DDIM(respace_type='uniform-linspace', respace_steps=3, eta=0.0, device=cuda)
        steps = list(d.sample_loop(m, init))
        assert len(steps) == 3
        last[half] = steps[-1]['sample'].cpu()
        assert dmhip.unet_conv_half(m.native_handle(torch.device(cuda))) is half
    assert torch.isfinite(last[True]).all() and not torch.equal(last[True], last[False])
    dist = (last[True] - last[False]).abs().max().item()
    print(f'tiny DDIM-3: conv-half to fp16x2 {dist:.3e}')
    report('tiny_ddim3_h16_to_fp16x2_maxabs', dist)
    _, meta = golden('adm')
    c = UNetCombined(**meta['archs']['adm_tiny'])
    assert c.set_conv_half(True) is True and c.unet_cond._conv_half and c.unet_uncond._conv_half


def test_script_option(cuda, tmp_path):
    """scripts/sample_uncond.py --conv_half on a reduced config writes its samples, which differ from the default
    arithmetic's; scripts/sample_cfg.py --conv_half on a DiT config exits, pointing at --math fp16."""
    from scripts import sample_cfg, sample_uncond
    from tests.test_gpu_scripts import TINY_DIT
    tiny = ['--model.params.dim', '32', '--model.params.dim_mults', '[1,2]', '--model.params.use_attn', '[false,true]',
            '--model.params.num_res_blocks', '1']
    common = ['-c', os.path.join(CONFIGS, 'ddpm_cifar10.yaml'), '--weights', 'synthetic', '--n_samples', '2',
              '--batch_size', '2', '--sampler', 'ddim', '--respace_steps', '3'] + tiny
    sample_uncond.main(common + ['--save_dir', str(tmp_path / 'h'), '--conv_half'])
    sample_uncond.main(common + ['--save_dir', str(tmp_path / 'x')])
    assert sorted(os.listdir(tmp_path / 'h')) == ['0.png', '1.png'] == sorted(os.listdir(tmp_path / 'x'))
    for f in ('0.png', '1.png'):   # the flag reaches the engine: another arithmetic, other pixels
        assert (tmp_path / 'h' / f).read_bytes() != (tmp_path / 'x' / f).read_bytes(), f
    with pytest.raises(SystemExit, match='--math fp16'):
        sample_cfg.main(['-c', os.path.join(CONFIGS, 'dit_xl2_256.yaml'), '--weights', 'synthetic', '--guidance_scale',
                         '4', '--class_ids', '7', '--n_samples_each_class', '1', '--batch_size', '1', '--sampler', 'ddim',
                         '--respace_steps', '2', '--save_dir', str(tmp_path / 'd'), '--conv_half'] + TINY_DIT)
