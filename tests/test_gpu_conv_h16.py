"""The conv-half 3x3 conv (csrc/conv_h16.hip) at the operator level, through dm_debug_conv_h16_image /
dm_debug_conv_h16 and float64 F.conv2d. Cases, references and bounds are tests/conv_h16_ref.py's (dry-run on a host
emulation in tests/test_conv_h16_host.py); the numbering follows that module's docstring:

(1) integer operands, bit for bit, per forced tile form and automatically   (2) both K segments, row vector, residual
and a pitched output in a NaN-filled buffer   (3) the image planes   (4) the conv on the device's own image   (5) the
distance to fp16x2   (6) the range flag   (7) refusals   (8) the emitted GroupNorm partials   (9) batch invariance.
"""
import ctypes

import pytest
import torch

import dmhip
from dmhip._lib import DM_ERR_UNSUPPORTED, DM_OK, load, stream_handle
from tests import conv_h16_ref as cr
from tests import norm_ref as nr
from tests.test_gpu_ops import _pack, _run_conv

pytestmark = pytest.mark.gpu
TAIL = 64          # sentinel fp16 elements past the planes
SENT16 = 0x7e2a    # an fp16 NaN pattern no kernel writes


class Dev:
    """conv_h16_ref.Emu's interface on the device."""
    name = 'device'

    def __init__(self, cuda):
        self.cuda = cuda
        self.L = load()

    def _build(self, s, tile):
        cuda = self.cuda
        x = s['x']
        B, C1, H, W = x.shape
        w = s['w']
        Cout, taps = w.shape[0], s.get('taps', 9)
        stride, up = s.get('stride', 1), s.get('upsample', 0)
        Ho, Wo = (2 * H, 2 * W) if up else ((H - 1) // stride + 1, (W - 1) // stride + 1)
        C2 = s['x2'].shape[1] if s.get('x2') is not None else 0
        K = taps * C1 + C2
        keep = []
        xp = s.get('x_pitch', C1)
        xb = torch.full((B, H, W, xp), float('nan'), device=cuda)
        xb[..., :C1] = cr.nhwc(x).to(cuda)
        wp = torch.zeros((Cout, K), device=cuda)
        if C1 % 32 == 0:
            _pack(w, cuda, K, 0, wp)
            if C2:
                _pack(s['ws'], cuda, K, taps * C1, wp)
            ws = dmhip.pack_conv_weight_split(wp, 1, C1, taps, dmhip.SPLIT_FP16X2)
        else:   # (the packers take Cin % 32 == 0 only: zero images of the right size; the gate refuses before they are read)
            ws = torch.zeros(self.L.dm_conv_weight_split_bytes(1, Cout, K, dmhip.SPLIT_FP16X2), dtype=torch.uint8,
                             device=cuda)
        pitch = s.get('y_pitch', Cout)
        y = torch.full((B, Ho, Wo, pitch), float('nan'), device=cuda)
        d = dmhip.ConvDesc()
        d.x, d.x_pitch, d.Cin, d.Hin, d.Win = xb.data_ptr(), xp, C1, H, W
        d.taps, d.stride, d.upsample = taps, stride, up
        if C2:
            x2 = cr.nhwc(s['x2']).to(cuda)
            d.x2, d.x2_pitch, d.Cin2 = x2.data_ptr(), C2, C2
            keep.append(x2)
        d.w, d.K = wp.data_ptr(), K
        d.y, d.y_pitch, d.Cout, d.B, d.Hout, d.Wout = y.data_ptr(), pitch, Cout, B, Ho, Wo
        for name in ('bias', 'rowvec'):
            if s.get(name) is not None:
                t = s[name].to(cuda).contiguous()
                setattr(d, name, t.data_ptr())
                keep.append(t)
        if s.get('rowvec') is not None:
            d.rowvec_pitch = Cout
        if s.get('res') is not None:
            res = cr.nhwc(s['res']).to(cuda)
            d.res, d.res_pitch = res.data_ptr(), Cout
            keep.append(res)
        if s.get('pro') is not None:
            sc, sh = (t.to(cuda).contiguous() for t in s['pro'])
            d.pro_scale, d.pro_shift, d.pro_nosilu = sc.data_ptr(), sh.data_ptr(), int(s.get('nosilu', 0))
            keep += [sc, sh]
        d.w_split, d.w_split_kind = ws.data_ptr(), dmhip.SPLIT_FP16X2
        flag = torch.zeros(1, dtype=torch.int32, device=cuda)
        d.range_flag = flag.data_ptr()
        n1 = B * H * W * C1
        n2 = B * Ho * Wo * C2
        n1a = (n1 + 7) // 8 * 8
        img = torch.full((n1a + n2 + TAIL + 8, ), SENT16, dtype=torch.int16, device=cuda)
        keep += [xb, wp, ws]
        return dict(d=d, y=y, img=img, flag=flag, n1=n1, n1a=n1a, n2=n2, keep=keep,
                    shape1=(B, H, W, C1), shape2=(B, Ho, Wo, C2), off=(1 if s.get('misalign') else 0))

    def _planes(self, r, ok):
        img = r['img'].cpu()[r['off']:]
        if not ok:
            assert (r['img'].cpu() == SENT16).all(), 'a refused call wrote to the image'
            return None, None
        n1, n1a, n2 = r['n1'], r['n1a'], r['n2']
        assert (img[n1:n1a] == SENT16).all() and (img[n1a + n2:] == SENT16).all(), 'a plane was written past its end'
        p1 = img[:n1].view(torch.float16).view(r['shape1'])
        p2 = img[n1a:n1a + n2].view(torch.float16).view(r['shape2']) if n2 else None
        return p1, p2

    def image(self, s):
        r = self._build(s, 0)
        rc = self.L.dm_debug_conv_h16_image(ctypes.byref(r['d']), r['img'].data_ptr() + 2 * r['off'],
                                            stream_handle(self.cuda))
        torch.cuda.synchronize(self.cuda)
        p1, p2 = self._planes(r, rc == DM_OK)
        assert torch.isnan(r['y']).all(), 'the image pass wrote to the output'
        return dict(rc=rc, plane1=p1, plane2=p2, flag=int(r['flag'].item()))

    def conv(self, s, tile=0, G=0):
        r = self._build(s, tile)
        st = stream_handle(self.cuda)
        ptr = r['img'].data_ptr() + 2 * r['off']
        part = None
        if G:
            B, Ho, Wo, _ = r['shape2']
            n = B * nr.nchunks(Ho * Wo) * G
            part = torch.full((n + nr.TAIL, 2), float('nan'), dtype=torch.float64, device=self.cuda)
            rc = self.L.dm_debug_conv_h16_gn(ctypes.byref(r['d']), ptr, tile, G, part.data_ptr(), st)
        else:
            rc = self.L.dm_debug_conv_h16(ctypes.byref(r['d']), ptr, tile, st)
        torch.cuda.synchronize(self.cuda)
        p1, p2 = self._planes(r, rc == DM_OK)
        return dict(rc=rc, y=r['y'].cpu(), plane1=p1, plane2=p2, flag=int(r['flag'].item()),
                    part=None if part is None else part.cpu())

    def fp16x2(self, s):
        """The same conv on the fp16x2 kernels (dm_conv2d_nhwc with split weights, no Winograd weights)."""
        cuda = self.cuda
        B, C1, H, W = s['x'].shape
        Cout = s['w'].shape[0]
        wp = _pack(s['w'], cuda)
        pro = None if s.get('pro') is None else tuple(t.to(cuda).contiguous() for t in s['pro'])
        y = _run_conv(cuda, cr.nhwc(s['x']).to(cuda), wp, Cout, H, W, 9, bias=s['bias'].to(cuda), pro=pro,
                      pro_nosilu=int(s.get('nosilu', 0)), split='fp16x2')
        return y.cpu()


@pytest.fixture(scope='module')
def be(cuda):
    return Dev(cuda)


@pytest.mark.parametrize('shape', cr.EXACT_SHAPES)
def test_integer_operands_exact(be, shape):
    """(1)"""
    s = cr.exact_case(*shape)
    want = cr.nhwc(cr.exact_ref(s))
    f = cr.form_of(shape[3], shape[3])
    for tile in (0, f):
        r = be.conv(s, tile)
        assert r['rc'] == DM_OK, (tile, load().dm_last_error())
        assert torch.equal(r['y'], want), f'tile {tile}: {(r["y"] - want).abs().max().item()}'
        assert r['flag'] == 0
    r = be.conv(s, 3 - f)        # the other form does not take the shape
    assert r['rc'] == DM_ERR_UNSUPPORTED and torch.isnan(r['y']).all()


@pytest.mark.parametrize('shape', cr.SEG_SHAPES)
def test_segments_rowvec_residual_pitch(be, shape):
    """(2)"""
    s = cr.segments_case(*shape)
    Cout = s['w'].shape[0]
    want = cr.nhwc(cr.exact_ref(s))
    for tile in (0, cr.form_of(shape[2], shape[2])):
        r = be.conv(s, tile)
        assert r['rc'] == DM_OK, load().dm_last_error()
        assert torch.equal(r['y'][..., :Cout], want)
        assert torch.isnan(r['y'][..., Cout:]).all(), 'the pad columns of the pitched output were written'
        assert torch.equal(r['plane2'].float(), cr.nhwc(s['x2']))


@pytest.mark.parametrize('kind', cr.IMAGE_KINDS)
def test_image_planes(be, report, kind):
    """(3)"""
    s = cr.image_case(kind)
    r = be.image(s)
    assert r['rc'] == DM_OK and r['flag'] == 0
    used = cr.image_check(s, r['plane1'].double(), None if r['plane2'] is None else r['plane2'].double())
    print(f'image {kind}: {used:.3f} of the bound')
    report(f'conv_h16_image_{kind}_err_over_bound', used)
    # bit for bit piece 0 of the split of the host's fp32 prologue wherever the fp32 prologue is exact (no prologue)
    if s.get('pro') is None:
        assert torch.equal(r['plane1'], cr.nhwc(s['x']).to(torch.float16))


@pytest.mark.parametrize('shape', cr.RAND_SHAPES)
def test_conv_on_own_image_and_distance(be, report, shape):
    """(4) and (5)"""
    s = cr.rand_case(*shape)
    r = be.conv(s)
    assert r['rc'] == DM_OK and r['flag'] == 0, load().dm_last_error()
    cr.image_check(s, r['plane1'].double())
    used4, bound4, e32 = cr.conv_on_image_check(s, r['y'], r['plane1'].double())
    yx2 = be.fp16x2(s)
    used5 = cr.distance_check(s, r['y'], yx2, bound4)
    tag = 'x'.join(map(str, shape))
    print(f'{tag}: check (4) {used4:.3f} of its bound (e32 {e32:.3e}), check (5) {used5:.3f} of its bound')
    report(f'conv_h16_on_image_{tag}_err_over_bound', used4)
    report(f'conv_h16_distance_{tag}_err_over_bound', used5)


@pytest.mark.parametrize('segment', [1, 2])
@pytest.mark.parametrize('peak,flagged', [(65504.0, 0), (1e5, 1)])
def test_range_flag(be, segment, peak, flagged):
    """(6)"""
    s = cr.flag_case(segment, peak)
    assert be.image(s)['flag'] == flagged
    assert be.conv(s)['flag'] == flagged


@pytest.mark.parametrize('kind', cr.REFUSALS)
def test_refusals(be, kind):
    """(7)"""
    s = cr.refusal_case(kind)
    for tile in (1, 2):
        r = be.conv(s, tile)
        assert r['rc'] == DM_ERR_UNSUPPORTED, (kind, tile, r['rc'])
        assert torch.isnan(r['y']).all(), 'a refused call wrote to the output'
    # ... and a w_split of another kind is an argument error
    r = be._build(cr.refusal_case('cin48'), 0)
    r['d'].w_split_kind = dmhip.SPLIT_BF16X3
    assert load().dm_debug_conv_h16(ctypes.byref(r['d']), r['img'].data_ptr(), 0, stream_handle(be.cuda)) not in (
        DM_OK, DM_ERR_UNSUPPORTED)


GN_CASES = [((3, 64, 64, 8), 16, 'chunk'),     # cpg 4 (the concat slices' 4-channel units), an odd image count
            ((2, 32, 64, 16), 8, 'chunk'),     # cpg 8
            ((2, 64, 128, 32), 8, 'chunk'),    # cpg 16
            ((1, 32, 64, 64), 2, 'cover'),     # cpg 32, 2-D tiles
            ((1, 64, 128, 64), 32, 'cover')]   # cpg 4, 2-D tiles


@pytest.mark.parametrize('shape,G,layout', GN_CASES)
def test_emitted_groupnorm_partials(be, report, shape, G, layout):
    """(8) tests/test_gpu_norm_ops.py's rule for the k32 epilogue: the output is bit-identical with and without the
    statistics, every slot of [B][nchunk][G] is written and the tail is not, each slot (64 consecutive pixels; for the
    2-D tiles, a disjoint cover of the image: each (image, group) total) within n 2^-52 sum|term| of the float64 sums
    of the stored output."""
    s = cr.rand_case(*shape)
    B, _, Cout, H = shape
    r0, r1 = be.conv(s), be.conv(s, 0, G)
    assert r0['rc'] == DM_OK and r1['rc'] == DM_OK, load().dm_last_error()
    assert torch.equal(r0['y'].view(torch.int32), r1['y'].view(torch.int32))
    nch = nr.nchunks(H * H)
    flat = r1['part']
    n = B * nch * G
    assert torch.isnan(flat[n:]).all() and not torch.isnan(flat[:n]).any()
    part = flat[:n].view(B, nch, G, 2)
    ref, bound = nr.partial_ref(r1['y'].view(B, H * H, Cout), G)
    if layout == 'cover':
        part, ref, bound = part.sum(dim=1), ref.sum(dim=1), bound.sum(dim=1) * nch
    rr = nr.ratio((part - ref).abs(), bound)
    report(f'conv_h16_gn_{"x".join(map(str, shape))}_G{G}', rr)
    assert rr <= 1.0, f'err / bound {rr:.3g}'


def test_groupnorm_partials_refused(be):
    """groups of 2 or 64 channels: the gate refuses, nothing is written"""
    s = cr.rand_case(3, 64, 64, 8)
    for G in (1, 32):   # cpg 64, cpg 2
        r = be.conv(s, 0, G)
        assert r['rc'] == DM_ERR_UNSUPPORTED and torch.isnan(r['y']).all() and torch.isnan(r['part']).all()


def test_batch_invariance(be):
    """(9)"""
    for shape in [(3, 64, 64, 8), (3, 32, 64, 16), (3, 32, 32, 64)]:
        s = cr.rand_case(*shape)
        y3 = be.conv(s)['y']
        for i in range(3):   # (8 x 8: image 1 is the second half of a tile, image 2 alone in the last one)
            one = dict(s, x=s['x'][i:i + 1], pro=tuple(t[i:i + 1] for t in s['pro']))
            y1 = be.conv(one)['y']
            assert torch.equal(y3[i:i + 1], y1), (shape, i)
            assert not torch.equal(y3[(i + 1) % 3:(i + 1) % 3 + 1], y1)
