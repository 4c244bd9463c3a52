"""Host checks of tests/split_operands_ref.py: every operand family splits into the intended pieces, which re-sum to
the value exactly; the exactness budget holds for every case tests/test_gpu_conv_split_pieces.py runs and its float64
reference is an fp32 value; the Winograd emulation equals the direct convolution; and the bit-for-bit comparison
detects a planted error (the low piece of one tap and channel zeroed in an fp32 emulation of the three- / six-product
contraction) in exactly the outputs that term reaches."""
import pytest
import torch
import torch.nn.functional as F

from tests import split_operands_ref as R


def test_g16_splits_into_two_nonzero_fp16_pieces():
    x = R.g16((4096, ), 1)
    h, l = R.split2(x)
    assert torch.equal(h.float(), x.round()) and (h != 0).all()
    assert torch.equal(l.double(), (x.double() - x.round().double())) and (l != 0).all()
    assert torch.equal(l.double() * 2 ** 14, (l.double() * 2 ** 14).round()) and (l.float().abs() <= 3 * 2.0 ** -14).all()
    assert torch.equal(h.double() + l.double(), x.double())


@pytest.mark.parametrize('npieces', [2, 3])
def test_g3_splits_into_the_intended_bf16_pieces(npieces):
    x = R.g3((4096, ), 2, npieces)
    p = R.split3(x)
    assert torch.equal(p[0].float(), x.round()) and (p[0] != 0).all() and (p[1] != 0).all()
    assert ((p[1].double() * 2 ** 11).abs() <= 3).all() and torch.equal(p[1].double() * 2 ** 11, (p[1].double() * 2 ** 11).round())
    assert ((p[2] != 0).all() if npieces == 3 else (p[2] == 0).all())
    assert torch.equal(sum(q.double() for q in p), x.double())


@pytest.mark.parametrize('lo,hi,subnormal', [(-2, 3, False), (-8, -3, True)])
def test_p16_pieces(lo, hi, subnormal):
    x = R.p16((8192, ), 3, lo, hi)
    h, l = R.split2(x)
    assert (l != 0).all() and torch.equal(h.double() + l.double(), x.double())
    ulp = torch.ldexp(torch.ones(8192, dtype=torch.float64), torch.frexp(h.double()).exponent - 11)
    assert (l.double().abs() <= 0.45 * ulp).all()
    if subnormal:
        assert (x.abs() < 2.0 ** -3).all() and (l.float().abs() < 2.0 ** -14).all()  # below fp16's smallest normal
    # an fp32 value in the normal range is exact under the three bf16 pieces
    y = torch.randn(8192, generator=torch.Generator().manual_seed(4)) * 37
    assert torch.equal(sum(q.double() for q in R.split3(y)), y.double())


def test_p16_rows_under_the_row_scale():
    w = R.p16_rows(64, 288, 5)
    sc = R.row_scale(w[None])
    ws = w * sc[:, None]
    m = ws.abs().amax(1)
    assert ((m >= 2.0 ** 13) & (m < 2.0 ** 14))[torch.arange(64) != 1].all() and m[1] == 0 and sc[1] == 1
    h, l = R.split2(ws)
    assert torch.equal(h.double() + l.double(), ws.double())
    nz = ws != 0
    assert (l != 0)[nz].all()
    assert ((l.float().abs() < 2.0 ** -14) & nz).sum() > 1000  # subnormal low pieces: > 2^16 below the row maximum
    assert sc[torch.arange(64) != 1].min() == 2.0 ** 4 and sc.max() == 2.0 ** 30  # the rows' own 2^k undone


@pytest.mark.parametrize('pro', [False, True])
def test_winograd_operands_split_exactly(pro):
    x = R.g16((2, 32, 6, 16), 6)
    V = R.wino_V(x * 2 - 1 if pro else x)  # fp32, as the loader forms it: no rounding on this grid
    assert torch.equal(V.double(), R.wino_V((x.double() * 2 - 1) if pro else x.double()))
    h, l = R.split2(V)
    assert torch.equal(h.double() + l.double(), V.double()) and (l != 0).float().mean() > 0.5
    w = R.g16((16, 32, 3, 3), 7)
    U = R.wino_U(w)
    assert torch.equal(U.float().double(), U)
    for k in (-20, 0, 9):  # any power-of-two row scale
        Us = U.float() * 2.0 ** k
        sc = R.row_scale(Us.reshape(4, 16, -1))
        h, l = R.split2(Us * sc[None, :, None, None])
        assert torch.equal((h.double() + l.double()) / sc.double()[None, :, None, None], Us.double())
        assert (l != 0).float().mean() > 0.5


def test_winograd_emulation_is_the_convolution():
    x, w = R.g16((2, 32, 6, 16), 8).double(), R.sparse_ints((8, 32, 3, 3), 9, 0.5).double()
    y = R.wino_out(R.wino_m(R.wino_V(x), R.wino_U(w)))
    assert torch.equal(y, F.conv2d(x, w, padding=1))
    x2, ws = R.g16((2, 64, 6, 16), 10).double(), R.sparse_ints((8, 64, 1, 1), 11, 0.5).double()
    Vs, Us = R.wino_shortcut_m(x2, ws)
    m = torch.stack([torch.einsum('bchw,oc->bohw', v, u) for v, u in zip(Vs, Us)])
    assert torch.equal(R.wino_out(m), F.conv2d(x2, ws))


@pytest.mark.parametrize('idx', range(len(R.CASES)), ids=R.CASE_IDS)
def test_case_is_admissible(idx):
    """The budget (a condition on the inputs): every accumulation's sum of |terms| is below 2^(24 - s) in the row's
    unit; then the float64 reference is a multiple of 2^-s below that bound, hence an fp32 value."""
    o = R.build(idx)
    assert o.budget < 0.95 * 2.0 ** 24, o.budget / 2.0 ** 24
    q = o.ref64 / o.unit[None, :, None, None] * 2.0 ** o.s
    assert torch.equal(q, q.round()) and q.abs().max() < 2.0 ** 24
    assert torch.equal(o.ref.double(), o.ref64)
    c, side = o.case, o.side
    low = o.x if side in ('act', 'both') else o.w
    if side == 'wgt':
        keep = torch.ones_like(o.w, dtype=torch.bool)
        keep[R.ZERO_ROW] = False
        if c['kind'] == 'fp16x2':
            keep[R.SUB_ROW, R.ZERO_CH] = False  # the subnormal row's one large weight
        low = (o.w / o.unit.float()[:, None, None, None])[keep]
    pl = R.pieces(low, c['kind'])[1]
    assert (pl != 0).all()  # the operand under test has a low piece everywhere
    if side == 'wgt' and c['kind'] == 'fp16x2':
        sub = o.w[R.SUB_ROW]
        sc = R.row_scale(o.w.reshape(1, c['Cout'], -1))[R.SUB_ROW]
        lo = R.split2(sub * sc)[1].float()
        assert ((lo != 0) & (lo.abs() < 2.0 ** -14)).sum() >= sub.numel() - sub[R.ZERO_CH].numel()  # subnormal pieces
        assert (o.w[R.ZERO_ROW] == 0).all() and (o.x[:, R.ZERO_CH] == (0.5 if c['pro'] else 0)).all()


def _planted_cases():
    B, C, Co, H = 1, 32, 8, 6
    yield 'G16-act', 'fp16x2', R.g16((B, C, H, H), 20), R.sparse_ints((Co, C, 3, 3), 21, 0.7), 'x'
    yield 'G16-wgt', 'fp16x2', R.sparse_ints((B, C, H, H), 22, 0.7), R.g16((Co, C, 3, 3), 23) * 2.0 ** -9, 'w'
    yield 'G3-act', 'bf16x3', R.g3((B, C, H, H), 24), R.sparse_ints((Co, C, 3, 3), 25, 0.7), 'x'
    yield 'G3-wgt', 'bf16x3', R.sparse_ints((B, C, H, H), 26, 0.7), R.g3((Co, C, 3, 3), 27) * 2.0 ** 5, 'w'
    oh = torch.zeros((9 * 4, C, 3, 3))  # one-hot weights over 4 channels: the P16 families
    for tap in range(9):
        oh[tap * 4 + torch.arange(4), torch.arange(4), tap // 3, tap % 3] = 1.0
    yield 'P16-act', 'fp16x2', R.p16((B, C, H, H), 28), oh, 'x'
    yield 'P16-small-act', 'fp16x2', R.p16((B, C, H, H), 29, -8, -3), oh, 'x'
    imp = torch.zeros((B, C, H, H))
    imp[0, 3, 2, 4] = 1.0
    yield 'P16-wgt', 'fp16x2', imp, R.p16_rows(Co, 9 * C, 30).view(Co, C, 3, 3), 'w'
    yield 'G3x3-wgt', 'bf16x3', imp, R.g3((Co, C, 3, 3), 31, 3), 'w'


@pytest.mark.parametrize('name,kind,x,w,which', list(_planted_cases()), ids=[c[0] for c in _planted_cases()])
@pytest.mark.parametrize('tap', [0, 4, 8])
def test_planted_low_piece_error_is_detected(name, kind, x, w, which, tap):
    ref = F.conv2d(x.double(), w.double(), padding=1)
    assert torch.equal(ref.float().double(), ref)
    good = R.emulate_conv(x, w, kind)
    assert torch.equal(good, ref.float())
    ch = 3
    bad = R.emulate_conv(x, w, kind, drop=(which, tap, ch))
    # the dropped products: (low piece of the operand) x (the other operand's pieces it is multiplied with)
    sc = R.row_scale(w.reshape(1, w.shape[0], -1))[:, None, None, None] if kind == 'fp16x2' else 1.0
    xs, ws = R.pieces(x, kind), [p.double() / sc for p in R.pieces(w * sc, kind)]  # fp16x2 splits the scaled rows
    dy, dx = divmod(tap, 3)
    H = x.shape[-1]
    if which == 'x':
        a = F.pad(xs[1].double(), (1, 1, 1, 1))[:, ch, dy:dy + H, dx:dx + H]
        b = sum(ws[ib].double() for ia, ib in R.PRODUCTS[kind] if ia == 1)[:, ch, dy, dx]
    else:
        a = sum(F.pad(xs[ia].double(), (1, 1, 1, 1)) for ia, ib in R.PRODUCTS[kind] if ib == 1)[:, ch, dy:dy + H, dx:dx + H]
        b = ws[1].double()[:, ch, dy, dx]
    delta = a[:, None] * b[None, :, None, None]
    assert (delta != 0).any()
    assert torch.equal(bad != ref.float(), delta != 0)  # the differing bits sit in the outputs the term reaches
    assert torch.equal(F.conv2d(x.double(), w.double(), padding=1), ref)  # the reference is untouched
