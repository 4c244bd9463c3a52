"""Operator-level tests of the unfused attention chain: the batched split S GEMM, softmax_rows and the batched split
PV GEMM (csrc/gemm.hip, csrc/elementwise.hip), launched alone on the test's own buffers as the plans issue them.

The chain is the VAE's only attention, the fallback of every shape the fused kernels refuse and the oracle of every
bit-identity claim for them; whole-model tests with synthetic weights give it nearly flat scores and model-level
tolerances. Here every stage is compared with float64 on the operands it multiplies (tests/unfused_attention_ref.py)
within the project's bound 2 e32 + 2^-21 max|ref|, e32 being torch's float32 error on the same operands, at the
smallest shapes with M / N / K tails, head strides, the legacy [q; k; v] layout with b_scale, ld > L and the
128 x 128 batched split instances the plans run (hook dm_debug_gemm_pick: dm_gemm with a nominal pick_M / pick_Z).

Every output buffer is prefilled with NaN, has 8 pad columns (4 for softmax_rows' own tests) and sentinel rows past
the last row; all of those must still be NaN afterwards, and the range flag reads 0 after every in-range case. The
checks are functions of a backend: DeviceBackend here, the fp32 emulation in tests/test_unfused_attention_host.py,
which validates the inputs, the margins and the checks' own logic on the CPU. No shape of the table is refused by a
DM_REQUIRE (K, N and the leading dimensions are multiples of 4, the operands 16-byte aligned).
"""
import ctypes

import pytest
import torch

from tests import attention_ref as ar
from tests import unfused_attention_ref as ur

pytestmark = pytest.mark.gpu

LABEL_128 = ('gemm_kernel<128,128,64,64,false,true>', 'gemm_kernel<128,128,64,64,true,true>')
LABEL_64 = ('gemm_kernel<64,64,32,32,false,true>', 'gemm_kernel<64,64,32,32,true,true>')


class DeviceBackend:
    """dmhip.gemm / dmhip.softmax_rows / dm_debug_gemm_pick on NaN-prefilled device buffers; results on the CPU."""
    name = 'device'

    def __init__(self, dev):
        import dmhip
        from dmhip import _lib
        self.dev, self.dmhip, self._lib = dev, dmhip, _lib
        self.hook = _lib.load().dm_debug_gemm_pick
        self.hook.argtypes = [ctypes.POINTER(dmhip.GemmDesc), ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]

    def _launch(self, d, s):
        """dm_gemm, or the hook when the spec has a nominal pick or asks for the launch's label."""
        pick, log = s.get('pick'), s.get('log')
        if pick is None and not log:
            self.dmhip.gemm(d, self.dev)
            return None
        if log:
            self.dmhip.launch_log(True)
        pm, pz = pick or (0, 0)
        self._lib.check(self.hook(ctypes.byref(d), pm, pz, self._lib.stream_handle(self.dev)), 'dm_debug_gemm_pick')
        if not log:
            return None
        labels = self.dmhip.launch_log_read()
        self.dmhip.launch_log(False)
        return labels

    def _desc(self, s, flag):
        B, H, L, Dh = s['shape']
        d = self.dmhip.GemmDesc()
        d.Z1, d.Z2 = s.get('sub') or (B, H)
        d.split, d.range_flag = s['split'], flag.data_ptr()
        return d

    def s_gemm(self, s):
        B, H, L, Dh = s['shape']
        C, o, ldc = H * Dh, ur.offsets(s['shape'], s['layout']), L + ur.PAD_C
        rows = s['rows'].to(self.dev)
        out = ur.s_buffer(s['shape']).to(self.dev)
        flag = torch.zeros((1, ), dtype=torch.int32, device=self.dev)
        d = self._desc(s, flag)
        d.M, d.N, d.K = L, L, Dh
        d.A, d.a_s1, d.a_s2, d.lda = rows.data_ptr() + 4 * o['q0'], L * 3 * C, o['hs'], 3 * C
        d.B, d.b_s1, d.b_s2, d.ldb, d.b_kn = rows.data_ptr() + 4 * o['k0'], L * 3 * C, o['hs'], 3 * C, 0
        d.C, d.c_s1, d.c_s2, d.ldc = out.data_ptr(), H * L * ldc, L * ldc, ldc
        d.alpha, d.b_scale = s['alpha'], s['b_scale']
        if s['split']:
            d.split_ea, d.split_eb = ur.E_S
        labels = self._launch(d, s)
        torch.cuda.synchronize()
        return dict(C=out.cpu(), flag=int(flag.item()), labels=labels)

    def softmax(self, x, rows, L, ld, offset=0):
        buf = x.to(self.dev)
        self.dmhip.softmax_rows(buf.view(-1)[offset:], rows, L, ld)
        torch.cuda.synchronize()
        return buf.cpu()

    def pv_gemm(self, s):
        B, H, L, Dh = s['shape']
        C, o, lda = H * Dh, ur.offsets(s['shape'], s['layout']), L + ur.PAD_C
        rows, P = s['rows'].to(self.dev), s['P'].to(self.dev)
        out = ur.o_buffer(s['shape']).to(self.dev)
        flag = torch.zeros((1, ), dtype=torch.int32, device=self.dev)
        d = self._desc(s, flag)
        d.M, d.N, d.K = L, Dh, L
        d.A, d.a_s1, d.a_s2, d.lda = P.data_ptr(), H * L * lda, L * lda, lda
        d.B, d.b_s1, d.b_s2, d.ldb, d.b_kn = rows.data_ptr() + 4 * o['v0'], L * 3 * C, o['hs'], 3 * C, 1
        d.C, d.c_s1, d.c_s2, d.ldc = out.data_ptr(), L * (C + ur.PAD_C), Dh, C + ur.PAD_C
        d.alpha, d.b_scale = 1.0, 0.0
        if s['split']:
            d.split_ea, d.split_eb = ur.E_PV
        labels = self._launch(d, s)
        torch.cuda.synchronize()
        return dict(C=out.cpu(), flag=int(flag.item()), labels=labels)


@pytest.fixture(scope='module')
def device(cuda):
    return DeviceBackend(cuda)


# ------------------------------------------------------------------------------------------------------- helpers
def spec(c, split, pick=None, sub=None, log=False, **over):
    return dict(rows=c['rows'], shape=c['shape'], layout=c['layout'], alpha=c['alpha'], b_scale=c['b_scale'],
                split=split, pick=pick, sub=sub, log=log, **over)


def checked(buf, rows, cols, what):
    """The pad columns and the sentinel rows are still NaN, the block the kernel owns is finite -> that block."""
    assert buf.shape[0] > rows and buf.shape[1] > cols
    assert torch.isnan(buf[:, cols:]).all(), f'{what}: a pad column was written'
    assert torch.isnan(buf[rows:]).all(), f'{what}: a row past the last was written'
    assert torch.isfinite(buf[:rows, :cols]).all(), f'{what}: an element was not written, or is not finite'
    return buf[:rows, :cols]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def close(report, key, got, ref, e32, bound):
    err = (got.double() - ref).abs().max().item()
    ratio = err / e32 if e32 > 0 else 0.0
    print(f'{key}: err {err:.3e} e32 {e32:.3e} ratio {ratio:.3f} bound {bound:.3e}')
    report(f'{key}_err_over_e32', ratio)
    assert err <= bound, (key, err, e32, ratio, bound)
    return ratio


def run_chain(be, c, split, pick=None, log=False):
    """S GEMM, softmax_rows in place on its pitched output, PV GEMM -> S, P [B, heads, L, L], O [B, heads, L, Dh],
    the two range flags, the raw O buffer and the launch labels."""
    B, H, L, Dh = c['shape']
    sp = spec(c, split, pick, log=log)
    s = be.s_gemm(sp)
    S = checked(s['C'], B * H * L, L, 'S').reshape(B, H, L, L)
    pbuf = be.softmax(s['C'], B * H * L, L, L + ur.PAD_C)
    P = checked(pbuf, B * H * L, L, 'P').reshape(B, H, L, L)
    o = be.pv_gemm(dict(sp, P=pbuf))
    O = ar.out_rows(checked(o['C'], B * L, H * Dh, 'O').reshape(B, L, H * Dh), H, Dh)
    return dict(S=S, P=P, O=O, flags=(s['flag'], o['flag']), obuf=o['C'], labels=(s['labels'], o['labels']))


# -------------------------------------------------------------------------------------------------------- checks
def check_integer_layout(be, tc, stage):
    """Small-integer operands, power-of-two scales, both arithmetics: the pitched output equals float64 exactly, so
    any wrong image, head, row, column or k index fails outright."""
    shape = tc['shape']
    B, H, L, Dh = shape
    ic = ur.integer_case(shape, tc['layout'])
    for split in (0, 2):
        sp = spec(ic, split, ur.pick_of(tc))
        if stage == 's':
            r = be.s_gemm(sp)
            got = checked(r['C'], B * H * L, L, 'S').reshape(B, H, L, L)
            want = ic['S']
        else:
            pbuf = ur.s_buffer(shape)
            pbuf[:B * H * L].view(B, H, L, L + ur.PAD_C)[..., :L] = ic['P']
            r = be.pv_gemm(dict(sp, P=pbuf))
            got = ar.out_rows(checked(r['C'], B * L, H * Dh, 'O').reshape(B, L, H * Dh), H, Dh)
            want = ic['O']
        assert r['flag'] == 0, (stage, split)
        assert torch.equal(got.double(), want), (stage, split, (got.double() - want).abs().max().item())


def check_stage_accuracy(be, report, tc, dist):
    """With the plan's exponents: S against float64 of the decoded operands, softmax_rows on those device scores
    against float64 softmax of the same scores, PV on those probabilities against float64; then the range
    fallback's split = 0 chain (S and O) against float64 of the effective operands. Each within its bound."""
    c = ur.table_case(tc, dist)
    key = f'{ur.case_id(tc)}_{dist}'
    pick = ur.pick_of(tc)
    r = run_chain(be, c, 2, pick)
    assert r['flags'] == (0, 0), r['flags']
    ref = c['ref'][2]
    close(report, f'unfused_s_{key}', r['S'], ref['S'], ref['S_e32'], ref['S_bound'])
    sm = ur.softmax_refs(r['S'])
    close(report, f'unfused_p_{key}', r['P'], sm['ref'], sm['e32'], sm['bound'])
    pv = ur.pv_refs(r['P'], c['ops'][2][2], 2)
    close(report, f'unfused_pv_{key}', r['O'], pv['ref'], pv['e32'], pv['bound'])
    r0 = run_chain(be, c, 0, pick)
    assert r0['flags'] == (0, 0), r0['flags']
    ref0 = c['ref'][0]
    close(report, f'unfused_s_fp32_{key}', r0['S'], ref0['S'], ref0['S_e32'], ref0['S_bound'])
    close(report, f'unfused_o_fp32_{key}', r0['O'], ref0['O'], ref0['O_e32'], ref0['O_bound'])


def check_chain(be, report, tc, dist):
    """S, softmax, PV as the plans issue them against attention_f64 on the decoded operands; `select`: the output is
    v[pi] to 2^-20 max|v|; `equal` (all keys identical): the output is the mean of v within the bound."""
    c = ur.table_case(tc, dist)
    key = f'unfused_o_{ur.case_id(tc)}_{dist}'
    r = run_chain(be, c, 2, ur.pick_of(tc))
    assert r['flags'] == (0, 0), r['flags']
    ref = c['ref'][2]
    close(report, key, r['O'], ref['O'], ref['O_e32'], ref['O_bound'])
    if dist == 'select':
        want = ar.selected_rows(c['v'], c['pi']).double()
        err = (r['O'].double() - want).abs().max().item()
        print(f'{key}: |out - v[pi]| {err:.3e}')
        assert err <= 2.0 ** -20 * c['v'].abs().max().item(), (key, err)
    if dist == 'equal':
        mean = c['v'].double().mean(dim=2, keepdim=True).expand_as(r['O'])
        assert (r['O'].double() - mean).abs().max().item() <= ref['O_bound']


def check_softmax_properties(be, report, L):
    """softmax_rows alone, 37 rows (not a multiple of the 4 per block), ld = L + 4: all-equal rows give exactly
    fl32(1 / L); rows near +250 / -250 and peaked rows stay finite and within the bound of float64 softmax;
    permuting the rows permutes the outputs bit for bit; at L = 256 a base pointer one float further (the register
    arm instead of the vector arm) is within the same bound; pads and sentinel rows stay NaN."""
    R, ld = ur.SOFTMAX_ROWS, L + ur.PAD_SM
    x = ur.softmax_case(L)

    def run(rows_in, offset=0):
        buf = torch.full((R + ur.SENT_ROWS, ld), float('nan'))
        buf[:R, :L] = rows_in
        if offset:
            flat = torch.cat([torch.full((offset, ), float('nan')), buf.view(-1)])
            out = be.softmax(flat, R, L, ld, offset=offset)
            assert torch.isnan(out[:offset]).all(), 'the floats before the first row were written'
            out = out[offset:].view(R + ur.SENT_ROWS, ld)
        else:
            out = be.softmax(buf, R, L, ld)
        return checked(out, R, L, f'softmax L={L}')
    y = run(x)
    inv = torch.tensor(1.0) / torch.tensor(float(L))
    for r in range(3):
        assert (y[r] == inv).all(), (L, r, y[r, :4].tolist(), inv.item())
    refs = ur.softmax_refs(x)
    close(report, f'unfused_softmax_L{L}', y, refs['ref'], refs['e32'], refs['bound'])
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(L))
    assert same_bits(run(x[perm]), y[perm]), 'a row result depends on its position'
    if L == 256:
        close(report, f'unfused_softmax_L{L}_unaligned', run(x, offset=1), refs['ref'], refs['e32'], refs['bound'])


def check_isolation(be, layout):
    """Image 0, head 0 alone (Z1 = Z2 = 1) of a (2, 2, 100, 32) buffer: with every element outside that image and head
    at 1e6, then NaN (qkv rows and the other slices' P), both GEMMs' outputs and flags are bit-identical to the run
    on the clean buffer, the flag is 0 and nothing outside the slice's block is written."""
    shape = ur.ISOLATION_SHAPE
    B, H, L, Dh = shape
    c = ur.case(shape, 'peaked', layout, *ur.scales(shape, layout))
    mask = ur.outside_mask(shape, layout)
    for split in (2, 0):
        sp = spec(c, split, sub=(1, 1))
        s0 = be.s_gemm(sp)
        assert torch.isfinite(s0['C'][:L, :L]).all() and torch.isnan(s0['C'][L:]).all() and torch.isnan(s0['C'][:, L:]).all()
        ref = c['ref'][split]
        assert (s0['C'][:L, :L].double() - ref['S'][0, 0]).abs().max().item() <= ref['S_bound'], (layout, split)
        pb = be.softmax(s0['C'], L, L, L + ur.PAD_C)
        o0 = be.pv_gemm(dict(sp, P=pb))
        oc = o0['C']
        assert torch.isfinite(oc[:L, :Dh]).all() and torch.isnan(oc[L:]).all() and torch.isnan(oc[:, Dh:]).all()
        assert (s0['flag'], o0['flag']) == (0, 0)
        for fill in (1e6, float('nan')):
            rows = c['rows'].clone()
            rows[mask] = fill
            pb2 = pb.clone()
            pb2[L:B * H * L, :L] = fill
            s1 = be.s_gemm(dict(sp, rows=rows))
            o1 = be.pv_gemm(dict(sp, rows=rows, P=pb2))
            assert (s1['flag'], o1['flag']) == (0, 0), (layout, split, fill)
            assert same_bits(s1['C'], s0['C']), (layout, split, fill, 'S')
            assert same_bits(o1['C'], o0['C']), (layout, split, fill, 'O')


FLAG_PLANTS = [('q', 1023.0, 0), ('q', 1024.0, 1), ('k', 1023.0, 0), ('k', 1024.0, 1), ('v', 1000.0, 0), ('v', 1100.0, 1)]


def check_range_flags(be):
    """One element of the last image and last head at a value whose scaled form (q alpha 2^6, k b_scale 2^6, v 2^6) is
    just inside (65472 / 64000) or beyond (65536 / 70400) fp16: the flag of the GEMM that reads it follows, the other
    GEMM's flag stays clear, and the clear cases still meet the bound. Legacy layout, alpha = b_scale = Dh^-1/4."""
    shape, layout = ur.ISOLATION_SHAPE, 'legacy'
    B, H, L, Dh = shape
    alpha, bs = ur.scales(shape, layout)
    base = ur.case(shape, 'flat', layout, alpha, bs)
    o = ur.offsets(shape, layout)
    at = dict(q=(o['q0'], alpha, 17, 5), k=(o['k0'], bs, 63, 30), v=(o['v0'], 1.0, 99, 31))
    for part, eff, want in FLAG_PLANTS:
        p0, scale, l, d = at[part]
        rows = base['rows'].clone()
        rows[(B - 1) * L + l, p0 + (H - 1) * o['hs'] + d] = ur.f32(eff / scale)
        c = ur.case_from_rows(rows, shape, layout, alpha, bs)
        assert (ur.max_scaled(c) > ur.FP16_MAX) == bool(want), (part, eff, ur.max_scaled(c))
        sp = spec(c, 2)
        s = be.s_gemm(sp)
        assert s['flag'] == (want if part != 'v' else 0), (part, eff, s['flag'])
        if part != 'v':
            if not want:
                S = checked(s['C'], B * H * L, L, 'S').reshape(B, H, L, L)
                ref = c['ref'][2]
                assert (S.double() - ref['S']).abs().max().item() <= ref['S_bound'], (part, eff)
            continue
        pbuf = be.softmax(s['C'], B * H * L, L, L + ur.PAD_C)
        r = be.pv_gemm(dict(sp, P=pbuf))
        assert r['flag'] == want, (part, eff, r['flag'])
        if not want:
            O = ar.out_rows(checked(r['C'], B * L, H * Dh, 'O').reshape(B, L, H * Dh), H, Dh)
            ref = c['ref'][2]
            assert (O.double() - ref['O']).abs().max().item() <= ref['O_bound'], (part, eff)


# --------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize('stage', ['s', 'pv'])
@pytest.mark.parametrize('tc', ur.CASES, ids=ur.case_id)
def test_integer_layout(device, tc, stage):
    check_integer_layout(device, tc, stage)


@pytest.mark.parametrize('tc,dist', ur.CASE_DISTS, ids=lambda v: v if isinstance(v, str) else ur.case_id(v))
def test_stage_accuracy(device, report, tc, dist):
    check_stage_accuracy(device, report, tc, dist)


@pytest.mark.parametrize('tc,dist', ur.CASE_DISTS, ids=lambda v: v if isinstance(v, str) else ur.case_id(v))
def test_chain_vs_float64(device, report, tc, dist):
    check_chain(device, report, tc, dist)


@pytest.mark.parametrize('L', ur.SOFTMAX_L)
def test_softmax_properties(device, report, L):
    check_softmax_properties(device, report, L)


@pytest.mark.parametrize('layout', ['blocks', 'legacy'])
def test_subproblem_isolation(device, layout):
    check_isolation(device, layout)


def test_range_flags(device):
    check_range_flags(device)


@pytest.mark.parametrize('dist', ur.FUSED_DISTS)
@pytest.mark.parametrize('shape', ur.FUSED_SHAPES, ids=ur.sid)
def test_fused_equals_unfused(cuda, device, shape, dist):
    """dm_debug_attention on the fp32 q | k | v rows (attn_fused_kernel<64> / <256>) equals this chain bit for bit,
    with dm_gemm's own tile choice and with the plans' nominal pick (the 128 x 128 instances wherever N >= 128)."""
    from tests.test_gpu_attention_ops import _attention
    B, H, L, Dh = shape
    C = H * Dh
    alpha, _ = ur.scales(shape, 'blocks')
    c = ur.case(shape, dist, 'blocks', alpha, 0.0)
    fused, flag = _attention(cuda, shape, qkv=c['rows'], alpha=alpha, b_scale=1.0)
    assert flag == 0 and torch.isnan(fused[..., C:]).all() and torch.isfinite(fused[..., :C]).all()
    want_labels = {None: LABEL_64, (0, ur.PICK_BATCH * H): (LABEL_128[0], LABEL_128[1] if Dh >= 128 else LABEL_64[1])}
    for pick, labels in want_labels.items():
        r = run_chain(device, c, 2, pick, log=True)
        assert r['flags'] == (0, 0)
        assert (r['labels'][0], r['labels'][1]) == ([labels[0]], [labels[1]]), (pick, r['labels'])
        chain = r['obuf'][:B * L].view(B, L, C + ur.PAD_C)[..., :C]
        assert torch.equal(fused[..., :C], chain), (pick, (fused[..., :C] - chain).abs().max().item())


@pytest.mark.parametrize('tc', ur.CASES, ids=ur.case_id)
def test_launched_instances(device, tc):
    """The nominal-pick case launches gemm_kernel<128,128,64,64,false,true> (S) and <128,128,64,64,true,true> (PV),
    every small-Z case the 64-tile instances; the hook with no nominal pick is dm_gemm bit for bit."""
    c = ur.table_case(tc, tc['dists'][1])
    r = run_chain(device, c, 2, ur.pick_of(tc), log=True)
    want = LABEL_128 if tc['pick_Z'] else LABEL_64
    assert r['labels'] == ([want[0]], [want[1]]), r['labels']
    if not tc['pick_Z']:
        plain = run_chain(device, c, 2)
        assert plain['labels'] == (None, None)
        assert torch.equal(plain['S'], r['S']) and torch.equal(plain['O'], r['O'])
