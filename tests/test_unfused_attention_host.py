"""CPU checks of the unfused attention chain tests' own inputs, layouts, margins and logic
(tests/unfused_attention_ref.py, tests/test_gpu_unfused_attention_ops.py), so that the GPU tests cannot hide a failure
behind a bad input or an unreachable bound:

* the row layouts: pack_rows and the device's addressing (unpack_rows, offsets) round-trip, the legacy rows are per
  head [q; k; v], the isolation mask covers exactly the other images and heads;
* the inputs are valid: `select` has distinct key rows and a winner ahead by >= 128 nats in every table case, every
  distribution appears on a shape with a tail, no in-range case trips the range predicate, the planted flag values
  sit on the intended side of 65504;
* the integer cases are exact in fp32 and in the fp16x2 split;
* every check of the GPU file runs on EmuBackend (the device arithmetic restated in fp32) and meets every bound, each
  err / e32 ratio printed; deliberately wrong backends (a wrong head stride, L for ld in softmax's row pointer, a
  dropped K tail, no max subtraction) make the checks fail.
"""
import pytest
import torch

from tests import attention_ref as ar
from tests import test_gpu_unfused_attention_ops as tg
from tests import unfused_attention_ref as ur

EMU = ur.EmuBackend()
RATIOS = {}


def _record(key, value):
    RATIOS[key] = value


def _noreport(*a):
    pass


# ------------------------------------------------------------------------------------------- layouts and inputs
@pytest.mark.parametrize('layout', ['blocks', 'legacy'])
def test_row_layouts(layout):
    shape = (2, 3, 5, 8)
    B, H, L, Dh = shape
    C = H * Dh
    q, k, v = (torch.arange(B * H * L * Dh, dtype=torch.float32).reshape(shape) + 1000.0 * i for i in range(3))
    rows = ur.pack_rows(q, k, v, layout)
    assert rows.shape == (B * L, 3 * C)
    for got, want in zip(ur.unpack_rows(rows, shape, layout), (q, k, v)):
        assert torch.equal(got, want)
    o = ur.offsets(shape, layout)
    if layout == 'legacy':
        assert (o['hs'], o['k0'], o['v0']) == (3 * Dh, Dh, 2 * Dh)
        assert torch.equal(rows[L + 2, 3 * Dh:4 * Dh], q[1, 1, 2]) and torch.equal(rows[L + 2, 5 * Dh:6 * Dh], v[1, 1, 2])
    else:
        assert (o['hs'], o['k0'], o['v0']) == (Dh, C, 2 * C)
        assert torch.equal(rows[L + 2, C + Dh:C + 2 * Dh], k[1, 1, 2])
    m = ur.outside_mask(shape, layout, 0, 0)
    assert int((~m).sum()) == 3 * L * Dh
    probe = rows.clone()
    probe[m] = float('nan')
    for got, want in zip(ur.unpack_rows(probe, shape, layout), (q, k, v)):
        assert torch.equal(got[0, 0], want[0, 0]) and torch.isnan(got[1]).all() and torch.isnan(got[0, 1:]).all()


def test_table_covers_every_distribution_on_a_tail():
    on_tail = {d for c in ur.CASES if c['shape'] in ur.TAIL_SHAPES for d in c['dists']}
    assert on_tail == set(ur.ALL_DISTS), set(ur.ALL_DISTS) - on_tail
    for c in ur.CASES:
        assert c['dists'][0] == 'select' and len(c['dists']) >= 3
    assert len(ur.TAIL_SHAPES) == 5


def test_scales_and_effective_operands():
    """alpha = Dh^-1/2 (a power of two only for Dh = 64) and ADM's Dh^-1/4; q_eff is the device's fp32 product of the
    row and alpha, within an ulp of the generated operand."""
    assert ur.scales((1, 1, 36, 64), 'blocks') == (0.125, 0.0)
    a, b = ur.scales((1, 2, 100, 32), 'legacy')
    assert a == b == ur.f32(32 ** -0.25)
    c = ur.case((2, 1, 40, 128), 'ramp40', 'blocks', *ur.scales((2, 1, 40, 128), 'blocks'))
    q, _, _, _ = ur.generate((2, 1, 40, 128), 'ramp40')
    assert not torch.equal(c['q_eff'], q)                       # 128^-1/2 rounds
    assert ((c['q_eff'] - q).abs() <= 2.0 ** -22 * q.abs()).all()
    q_rows, _, _ = ur.unpack_rows(c['rows'], c['shape'], c['layout'])
    assert torch.equal(c['q_eff'], q_rows * torch.tensor(c['alpha']))


@pytest.mark.parametrize('tc', ur.CASES, ids=ur.case_id)
def test_select_inputs(tc):
    c = ur.table_case(tc, 'select')
    _, kd, _ = c['ops'][2]
    B, H, L, Dh = tc['shape']
    for b in range(B):
        for h in range(H):
            assert torch.unique(kd[b, h], dim=0).shape[0] == L, 'select: the key rows must be distinct'
    margin = ur.select_margin(c)
    print(f'select {ur.case_id(tc)}: margin {margin:.1f} nats')
    assert margin >= 128.0, margin


def test_no_in_range_case_trips_the_range_predicate():
    worst = 0.0
    cases = [ur.table_case(tc, d) for tc, d in ur.CASE_DISTS]
    cases += [ur.case(s, d, 'blocks', ur.scales(s, 'blocks')[0], 0.0) for s in ur.FUSED_SHAPES for d in ur.FUSED_DISTS]
    cases += [ur.case(ur.ISOLATION_SHAPE, 'peaked', lay, *ur.scales(ur.ISOLATION_SHAPE, lay)) for lay in ('blocks', 'legacy')]
    for c in cases:
        m = ur.max_scaled(c)
        assert m <= ur.FP16_MAX, (c['shape'], m)
        worst = max(worst, m)
        assert EMU.s_gemm(tg.spec(c, 2))['flag'] == 0
    print(f'largest scaled operand {worst:.1f} of {ur.FP16_MAX}')
    assert worst >= 64000.0    # near_fp16 does reach the edge


@pytest.mark.parametrize('tc', ur.CASES, ids=ur.case_id)
def test_integer_cases_are_exact(tc):
    ic = ur.integer_case(tc['shape'], tc['layout'])
    q, k, v = ur.unpack_rows(ic['rows'], ic['shape'], ic['layout'])
    for x, e in ((q * ic['alpha'], 6), (k * ic['b_scale'], 6), (v, 6), (ic['P'], 14)):
        hi, lo = ar.split_planes(x, e)
        assert (lo == 0).all() and torch.equal(hi.double(), x.double() * 2.0 ** e)
    # the largest partial sum, in units of the smallest product, stays below 2^24
    assert ic['S'].abs().max().item() * 8 < 2 ** 24 and ic['O'].abs().max().item() * 4 < 2 ** 24
    assert ic['S'].abs().max().item() > 0 and len(torch.unique(ic['O'])) > 16


# ------------------------------------------------------------------------------------- dry runs of the checks
@pytest.mark.parametrize('stage', ['s', 'pv'])
@pytest.mark.parametrize('tc', ur.CASES, ids=ur.case_id)
def test_dry_integer_layout(tc, stage):
    tg.check_integer_layout(EMU, tc, stage)


@pytest.mark.parametrize('tc,dist', ur.CASE_DISTS, ids=lambda v: v if isinstance(v, str) else ur.case_id(v))
def test_dry_stage_accuracy_and_chain(tc, dist):
    """The emulation meets every bound of every stage and of the chain; the ratios are printed."""
    tg.check_stage_accuracy(EMU, _record, tc, dist)
    tg.check_chain(EMU, _record, tc, dist)


def test_emulation_ratios_stay_below_the_bounds_factor():
    """After the dry runs: the worst err / e32 per stage. The emulation needs less than the bound's factor 2 wherever
    e32 is not zero, so the 2^-21 term is the kernels' margin for their summation order."""
    if not RATIOS:
        for tc, dist in ur.CASE_DISTS:
            tg.check_stage_accuracy(EMU, _record, tc, dist)
            tg.check_chain(EMU, _record, tc, dist)
    for stage in ('s', 'p', 'pv', 'o', 's_fp32', 'o_fp32'):
        keys = [k for k in RATIOS if k.startswith(f'unfused_{stage}_') and k[len(f'unfused_{stage}_')].isdigit()]
        assert keys, stage
        worst = max(keys, key=RATIOS.get)
        print(f'{stage}: worst err / e32 {RATIOS[worst]:.3f} at {worst}')


@pytest.mark.parametrize('L', ur.SOFTMAX_L)
def test_dry_softmax_properties(L):
    x = ur.softmax_case(L)
    assert x.shape == (ur.SOFTMAX_ROWS, L) and ur.SOFTMAX_ROWS % 4 != 0 and (L + ur.PAD_SM) % 4 == 0
    assert x[3:].max() > 240 and x[3:].min() < -240
    tg.check_softmax_properties(EMU, _noreport, L)


@pytest.mark.parametrize('layout', ['blocks', 'legacy'])
def test_dry_isolation(layout):
    tg.check_isolation(EMU, layout)


def test_dry_range_flags():
    tg.check_range_flags(EMU)
    for part, eff, want in tg.FLAG_PLANTS:
        assert (eff * 64.0 > ur.FP16_MAX) == bool(want)


# ---------------------------------------------------------------------------- the checks catch a wrong backend
class _WrongHeadStride(ur.EmuBackend):
    """b_s2 taken from the other layout (as a swapped a_s2 / b_s2 would on the qkv rows)."""
    def s_gemm(self, s):
        q, _, _ = ur.unpack_rows(s['rows'], s['shape'], s['layout'])
        _, k, v = ur.unpack_rows(s['rows'], s['shape'], 'legacy' if s['layout'] == 'blocks' else 'blocks')
        return super().s_gemm(dict(s, rows=ur.pack_rows(q, k, v, s['layout'])))


class _DroppedKTail(ur.EmuBackend):
    """The PV GEMM stops at the last whole 32-deep K slice."""
    def pv_gemm(self, s):
        L = s['shape'][2]
        P = s['P'].clone()
        P[:, L // 32 * 32:L] = 0.0
        return super().pv_gemm(dict(s, P=P))


class _SoftmaxWrongPitch(ur.EmuBackend):
    def softmax(self, x, rows, L, ld, offset=0):
        out = x.clone()
        v = out.view(-1)[offset:offset + rows * L].view(rows, L)
        v[:] = ur.emu_softmax(torch.nan_to_num(v, nan=0.0))
        return out


class _SoftmaxNoMax(ur.EmuBackend):
    def softmax(self, x, rows, L, ld, offset=0):
        out = x.clone()
        v = out.view(-1)[offset:offset + rows * ld].view(rows, ld)
        e = torch.exp(v[:, :L])
        v[:, :L] = e / e.sum(dim=-1, keepdim=True)
        return out


def test_checks_catch_wrong_backends():
    multi_head = ur.CASES[2]     # (2, 3, 64, 72)
    with pytest.raises(AssertionError):
        tg.check_integer_layout(_WrongHeadStride(), multi_head, 's')
    k_tail = ur.CASES[0]         # L = 36
    with pytest.raises(AssertionError):
        tg.check_integer_layout(_DroppedKTail(), k_tail, 'pv')
    with pytest.raises(AssertionError):
        tg.check_chain(_DroppedKTail(), _noreport, k_tail, 'peaked')
    with pytest.raises(AssertionError):
        tg.check_softmax_properties(_SoftmaxWrongPitch(), _noreport, 36)
    with pytest.raises(AssertionError):
        tg.check_chain(_SoftmaxWrongPitch(), _noreport, k_tail, 'peaked')
    for L in (576, 1024):
        with pytest.raises(AssertionError):
            tg.check_softmax_properties(_SoftmaxNoMax(), _noreport, L)
    with pytest.raises(AssertionError):
        tg.check_chain(_SoftmaxNoMax(), _noreport, ur.CASES[5], 'offset')


def test_checked_rejects_stray_and_missing_writes():
    buf = ur.s_buffer((1, 1, 36, 64))
    buf[:36, :36] = 1.0
    tg.checked(buf, 36, 36, 'ok')
    for r, c, val in ((3, 37, 0.0), (36, 0, 0.0), (5, 5, float('nan'))):
        bad = buf.clone()
        bad[r, c] = val
        with pytest.raises(AssertionError):
            tg.checked(bad, 36, 36, 'bad')
    a = torch.tensor([float('nan'), 1.0])
    assert tg.same_bits(a, a.clone()) and not tg.same_bits(a, torch.tensor([float('nan'), 2.0]))
