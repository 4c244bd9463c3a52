"""MDTv2 (models/mdt/model.py) on the MI355X path against REFERENCE fixtures.

tests/golden/mdt.npz holds outputs of the reference module itself (tests/golden/make_golden_mdt.py runs
models/mdt/model.py on the CPU behind a stub of the three timm names it imports). Tolerance: fp32 max-abs <= 1e-4,
the project's forward tolerance. The fixtures' weights make each MDT-specific mechanism (bias tables, their
orientation and head, the skip order, decoder_pos_embed) worth >= 100 x that tolerance (tests/test_mdt_host.py).

  mdt_a  T = 64,  W = 8,  Dh = 32: the 2-wave biased flash kernel; two skips, so their order matters
  mdt_b  T = 256, W = 16, Dh = 72: the 8-wave biased flash kernel with the 16x16x32 tail, the K = 2 D skip GEMM on
                                   linear_k32 behind linear_presplit_cat
  mdt_c  T = 16: the unfused fallback (softmax_rows_bias) and the chained skip GEMMs
"""
import numpy as np
import pytest
import torch

from diffusions import DDIMCFG
from models.mdt.model import MDTv2
from utils.synthetic import state_dict_sha256, synthetic_mdt_state_dict

pytestmark = pytest.mark.gpu

TOL = 1e-4
NAMES = ['mdt_a', 'mdt_b', 'mdt_c']


def _model(meta, name, dev):
    m = MDTv2(**meta['archs'][name]).eval()
    sd = synthetic_mdt_state_dict(m.state_dict())
    assert state_dict_sha256(sd) == meta[f'{name}_weights_sha256']
    m.load_state_dict(sd)
    return m.to(dev)


def _inputs(g, name, dev):
    return (torch.from_numpy(g[f'{name}_{k}']).to(dev) for k in ('x', 't', 'labels'))


def _labels(model):
    import dmhip
    return [op['label'] for op in dmhip.unet_profile_read(model.native_handle(torch.device('cuda:0')), abi='dm_mdt')]


@pytest.mark.parametrize('math', ['fp16x2', 'fp32'])
@pytest.mark.parametrize('name', NAMES)
def test_mdt_forward_vs_reference(cuda, golden, report, name, math):
    """Forward with labels and with the null class against the reference outputs, in the default fp16x2 arithmetic
    and in fp32; the plan runs the kernels the architecture was chosen to reach."""
    import dmhip
    g, meta = golden('mdt')
    model = _model(meta, name, cuda)
    h = model.native_handle(torch.device(cuda))
    assert dmhip.dit_math(h, abi='dm_mdt') == 'fp16x2'
    assert dmhip.dit_math(h, math, abi='dm_mdt') == math
    x, t, y = _inputs(g, name, cuda)
    out_y = model(x, t, y).cpu()
    out_n = model(x, t, None).cpu()
    e_y = (out_y - torch.from_numpy(g[f'{name}_out_y'])).abs().max().item()
    e_n = (out_n - torch.from_numpy(g[f'{name}_out_null'])).abs().max().item()
    print(f'mdt_forward_{name}_{math}: y {e_y:.3e} null {e_n:.3e}')
    report(f'mdt_forward_{name}_{math}_y_maxabs_vs_reference', e_y)
    report(f'mdt_forward_{name}_{math}_null_maxabs_vs_reference', e_n)
    assert e_y <= TOL and e_n <= TOL, (e_y, e_n)
    labels = _labels(model)
    a = meta['archs'][name]
    n_blocks = (a['depth'] - a['decode_layer']) // 2 * 2 + a['decode_layer']
    flash = [s for s in labels if s.startswith('attn_flash_bias_kernel')]
    if math == 'fp16x2' and name != 'mdt_c':
        assert len(flash) == n_blocks, labels
        assert 'softmax_rows_bias' not in labels
    else:
        assert not flash and labels.count('softmax_rows_bias') == n_blocks, labels
    assert 'softmax_rows' not in labels and not [s for s in labels if s.startswith('attn_flash_kernel')]
    if name == 'mdt_b' and math == 'fp16x2':   # one K = 2 D GEMM per skip block behind the concat pre-split
        assert labels.count('linear_presplit_cat') == n_blocks - (a['depth'] - a['decode_layer']) // 2, labels
    assert labels.count('add_rows_mod') == 1


def test_mdt_unfused_attention_toggle(cuda, golden, report, monkeypatch):
    """DM_ATTN=unfused: mdt_a through the S GEMM, softmax_rows_bias and the PV GEMM instead of the flash kernel."""
    monkeypatch.setenv('DM_ATTN', 'unfused')
    g, meta = golden('mdt')
    model = _model(meta, 'mdt_a', cuda)
    x, t, y = _inputs(g, 'mdt_a', cuda)
    err = (model(x, t, y).cpu() - torch.from_numpy(g['mdt_a_out_y'])).abs().max().item()
    report('mdt_forward_mdt_a_unfused_maxabs_vs_reference', err)
    assert err <= TOL, err
    labels = _labels(model)
    assert labels.count('softmax_rows_bias') == 6 and not [s for s in labels if s.startswith('attn_flash')], labels


def test_mdt_null_label_scope_and_index_errors(cuda, golden):
    """As DiT: inside dmhip.null_label_scope() y[b] = -1 selects the null class row (the same as y=None); outside it a
    negative label is an IndexError, as is a label beyond the table; the null class index itself is a valid label."""
    import dmhip
    g, meta = golden('mdt')
    model = _model(meta, 'mdt_a', cuda)
    x, t, y = _inputs(g, 'mdt_a', cuda)
    out_n = model(x, t, None).cpu()
    with dmhip.null_label_scope():
        neg = model(x, t, torch.full_like(y, -1)).cpu()
    assert torch.equal(neg, out_n)
    with pytest.raises(IndexError):
        model(x, t, torch.full_like(y, -1))
    nc = meta['archs']['mdt_a']['num_classes']
    with pytest.raises(IndexError):
        model(x, t, torch.full_like(y, nc + 1))
    assert torch.equal(model(x, t, torch.full_like(y, nc)).cpu(), out_n)
    no_null = MDTv2(**dict(meta['archs']['mdt_c'], class_dropout_prob=0.0)).to(cuda)
    with pytest.raises(IndexError):
        no_null(torch.zeros((1, 4, 8, 8), device=cuda), torch.zeros((1, ), dtype=torch.long, device=cuda), None)
    with pytest.raises(NotImplementedError):
        model(x, t, y, enable_mask=True)


@pytest.mark.parametrize('name', ['mdt_a', 'mdt_b'])
def test_mdt_plan_replay_with_other_inputs(cuda, golden, name):
    """Two consecutive forwards with different inputs on one plan (graph replay over the skip workspace): the second
    equals what a fresh model computes for it, the first is reproduced afterwards, one plan was built."""
    import dmhip
    g, meta = golden('mdt')
    model = _model(meta, name, cuda)
    x, t, y = _inputs(g, name, cuda)
    gen = torch.Generator().manual_seed(11)
    x2 = torch.randn(x.shape, generator=gen).to(cuda)
    t2, y2 = torch.tensor([400, 801], device=cuda), torch.tensor([0, 9], device=cuda)
    a1 = model(x, t, y).cpu()
    a2 = model(x2, t2, y2).cpu()
    a3 = model(x, t, y).cpu()
    assert torch.equal(a1, a3) and not torch.equal(a1, a2)
    assert (a1 - torch.from_numpy(g[f'{name}_out_y'])).abs().max().item() <= TOL
    assert dmhip.plan_stats(model.native_handle(torch.device(cuda)), abi='dm_mdt') == (1, 1)
    fresh = _model(meta, name, cuda)
    assert torch.equal(fresh(x2, t2, y2).cpu(), a2)


@pytest.mark.parametrize('lin_sk', ['default', '0'])
@pytest.mark.parametrize('name', ['mdt_a', 'mdt_b'])
def test_mdt_batch_rows_vs_single(cuda, golden, report, monkeypatch, name, lin_sk):
    """B = 3 rows against three B = 1 forwards, the rule the README states for DiT: rows within 5e-7, and bit for bit
    with DM_LIN_SK=0. The split-K tail's reduction order is the one thing that depends on the batch; the README's
    figure is, as DESIGN.md's split-K section and test_dit_xl2_cfg_batch64 measure it, a fraction of the output's
    max (fp32 re-association), so it is applied to |difference| / max|out| here as well."""
    if lin_sk != 'default':
        monkeypatch.setenv('DM_LIN_SK', lin_sk)
    g, meta = golden('mdt')
    model = _model(meta, name, cuda)
    S = meta['archs'][name]['input_size']
    gen = torch.Generator().manual_seed(13)
    x = torch.randn((3, 4, S, S), generator=gen).to(cuda)
    t = torch.tensor([999, 500, 3], device=cuda)
    y = torch.tensor([1, 5, 9], device=cuda)
    full = model(x, t, y).cpu()
    worst = 0.0
    for b in range(3):
        one = model(x[b:b + 1].contiguous(), t[b:b + 1].contiguous(), y[b:b + 1].contiguous()).cpu()
        worst = max(worst, (one[0] - full[b]).abs().max().item())
    scale = full.abs().max().item()
    print(f'mdt_{name}_b3_rows_vs_b1 lin_sk={lin_sk}: {worst:.3e} abs, {worst / scale:.3e} of max |out| {scale:.3f}')
    report(f'mdt_{name}_b3_rows_vs_b1_lin_sk_{lin_sk}_rel', worst / scale)
    if lin_sk == '0':
        assert worst == 0.0, worst
    assert worst / scale <= 5e-7, (worst, scale)


def test_mdt_forward_with_cfg_vs_reference(cuda, golden, report):
    """forward_with_cfg (power-cosine scale) against the reference's own forward_with_cfg."""
    g, meta = golden('mdt')
    model = _model(meta, 'mdt_a', cuda)
    c = meta['cfg']
    x, t, y = (torch.from_numpy(g[f'cfg_{k}']).to(cuda) for k in ('x', 't', 'labels'))
    out = model.forward_with_cfg(x, t, y, cfg_scale=c['cfg_scale'], diffusion_steps=c['diffusion_steps'],
                                 scale_pow=c['scale_pow']).cpu()
    err = (out - torch.from_numpy(g['cfg_out'])).abs().max().item()
    report('mdt_forward_with_cfg_maxabs_vs_reference', err)
    assert err <= TOL, err
    assert torch.equal(out[:2, :3], out[2:, :3])
    plain = model.forward_with_cfg(torch.cat([x[:2], x[:2]]), t, y)   # cfg_scale None: the plain forward
    assert torch.equal(plain.cpu()[:, 3:], out[:, 3:])


@pytest.mark.parametrize('batched', [True, False])
def test_mdt_ddimcfg_trajectory_vs_reference(cuda, golden, report, batched):
    """DDIMCFG-5 (s = 4) on mdt_a against the reference model's trajectory: every step within 1e-4, the acceptance
    rule of test_dit_ddimcfg_trajectory_vs_oracle."""
    g, meta = golden('mdt')
    model = _model(meta, 'mdt_a', cuda)
    cfg = meta['cfg5']
    d = DDIMCFG(guidance_scale=cfg['guidance_scale'], respace_type=cfg['respace_type'],
                respace_steps=cfg['respace_steps'], eta=cfg['eta'], device=cuda)
    d.batch_cfg = batched
    labels = torch.from_numpy(g['cfg5_labels']).to(cuda)
    worst = 0.0
    for i, out in enumerate(d.sample_loop(model, torch.from_numpy(g['cfg5_init']).to(cuda),
                                          model_kwargs=dict(y=labels))):
        err = float(np.abs(out['sample'].cpu().numpy() - g[f'cfg5_step{i}_sample']).max())
        worst = max(worst, err)
        print(f'mdt cfg5 step {i}: {err:.3e}')
        assert err <= TOL, (i, err)
    report(f'mdt_ddimcfg5_{"batched" if batched else "two_calls"}_maxabs_vs_reference', worst)
