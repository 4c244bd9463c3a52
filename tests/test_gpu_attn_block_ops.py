"""Operator-level tests of the folded UNet attention blocks (csrc/attn_block.hip): attn_block3_kernel,
attn_block4_kernel<8> and attn_small_kernel launched alone, and the fold helpers (attn_fold, attn_perm_cols,
attn_transpose), through dm_debug_attn_block: the product fold (attn_fold_all, the routine UNetModel::fold_for calls) of
the block's own parameters into the test's workspace, then one launch with the arguments the UNet plan gives it.

Inputs, references, yardsticks and the fp32 emulation are tests/attn_block_ref.py's; tests/test_attn_block_host.py
shows on the CPU that the emulation meets every bound used here on every family and that each of its mutants (no
rescale of O or l, a per-chunk maximum, a dropped split term, w or cb omitted, the bk term added back, a permutation
applied on one side only, swapped key chunks) breaks one, so no bound below is fitted to the kernels.

a. kernel accuracy: kinds 3, 4 (L = 256) and 16 (attn_small, L = 16) on every family at B = 1 and 3 (3: variant 3's
   grid is 6 blocks, the remainder branch of xcd_remap_p) against the folded form in float64 on the operands the kernel
   consumed (x, the tables, the hook's fp32 w / cb, At / Wg decoded from their fp16x2 split; attn_small: the fp32 At /
   Wg): err <= 2 e32f + 2^-21 max|ref|, e32f the same form's float32 error.
b. module accuracy: the same launches against the unfolded module in float64, err <= 2 e32 + 2^-21 max|ref| (the
   emulation meets it without a term for the fold's rounding). On `bigbk` this is the test of the dropped terms and w.
c. key selection: `select`'s exact answer x + g[winner] within 2^-20 max|g|.
d. bit identities on peaked / ramp40 / desc200: variant 3 = variant 4; the in-kernel GroupNorm finalize (gin_*) = the
   table form with dm_debug_gn_finalize's tables; replacing one image leaves the others' rows and statistics alone.
e. the emitted GroupNorm statistics, slot by slot against the float64 sums of the stored y (norm_ref's rule:
   n 2^-52 sum|term|), spare slots untouched, and the launchers' refusals, which write nothing.
f. the fold results read back from the workspace. g. the range flag: 0 everywhere but on gnwide's twin.

Every y is NaN-prefilled at pitch 256 + 8 with a tail: the pad columns and the tail must stay NaN, everything else be
finite; x has pitch 256 + 4 with NaN pad columns that must not be read.
"""
import ctypes
import functools

import pytest
import torch

from tests import attn_block_ref as ab
from tests import norm_ref as nr

pytestmark = pytest.mark.gpu

vp, ci, cf, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
F32, F64 = torch.float32, torch.float64
C = ab.C
XP, YP = C + 4, C + 8
SENT = 7.25e77                 # gn_part prefill
KINDS = [3, 4, 16]
ID_FAMS = ['peaked', 'ramp40', 'desc200']
_WORST = {}


def _L(kind):
    return 16 if kind == 16 else 256


class Device:
    def __init__(self, dev):
        from dmhip import _lib
        self.dev, self._lib, self.L = dev, _lib, _lib.load()
        self.L.dm_debug_attn_fold_bytes.argtypes = [ci]
        self.L.dm_debug_attn_fold_bytes.restype = ctypes.c_int64
        self.L.dm_debug_attn_block.argtypes = [vp, vp, vp, vp, cd, vp, ci, vp, vp, vp, ci, ci, vp, vp, cf, ci, ci, ci, vp,
                                               ci, vp, ci, vp, vp, vp]
        self.L.dm_debug_gn_finalize.argtypes = [vp, ci, ci, ci, ci, cf, vp, vp, vp, vp, ci, vp, vp, vp]
        self.nws = int(self.L.dm_debug_attn_fold_bytes(C))
        assert self.nws >= (5 * C * C + 2 * C) * 4

    @staticmethod
    def _p(t):
        return None if t is None else t.data_ptr()

    def _up(self, t):
        return None if t is None else t.contiguous().to(self.dev)

    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def finalize(self, part, B, HW, G, gamma, beta):
        """dm_debug_gn_finalize on float64 partials [B, nchunk, G, 2] -> (gsc, gsh) [B, C] CPU."""
        pd, ga, be = self._up(part), self._up(gamma), self._up(beta)
        sc = torch.full((B, C), nr.NAN, device=self.dev)
        sh = torch.full((B, C), nr.NAN, device=self.dev)
        self._lib.check(self.L.dm_debug_gn_finalize(self._p(pd), B, HW, C, G, nr.EPS, self._p(ga), self._p(be), None, None,
                                                    0, self._p(sc), self._p(sh), self._stream()), 'dm_debug_gn_finalize')
        return sc.cpu(), sh.cpu()

    def run(self, c, kind, gsc=None, gsh=None, gin=None, gn_G=0, x=None):
        """One dm_debug_attn_block launch of case c. gsc / gsh default to the case's tables; gin = dict(part, G,
        gamma, beta) selects the in-kernel finalize instead. -> dict(rc, y [B, L, C], ybuf, flag, part, fold)."""
        B, L = c['B'], c['L']
        x = c['x'] if x is None else x
        xb = torch.full((B, L, XP), nr.NAN)
        xb[..., :C] = x
        wq, bq = ab.wqkv(c)
        d = [self._up(t) for t in (wq, bq, c['Wp'], c['bp'], xb)]
        if gin is None:
            tabs = [self._up(c['gsc'] if gsc is None else gsc), self._up(c['gsh'] if gsh is None else gsh)]
            gargs = [None, 0, 0, None, None, 0.0]
        else:
            tabs = [None, None]
            gk = [self._up(gin['part']), self._up(gin['gamma']), self._up(gin['beta'])]
            gargs = [self._p(gk[0]), gin['G'], gin['part'].shape[1], self._p(gk[1]), self._p(gk[2]), nr.EPS]
        y = torch.full((B * L + nr.TAIL, YP), nr.NAN, device=self.dev)
        flag = torch.zeros(1, dtype=torch.int32, device=self.dev)
        ws = torch.zeros(self.nws, dtype=torch.uint8, device=self.dev)
        nslot = B * nr.nchunks(L) * gn_G
        part = torch.full((nslot + nr.TAIL, 2), SENT, dtype=F64, device=self.dev) if gn_G else None
        rc = self.L.dm_debug_attn_block(self._p(d[0]), self._p(d[1]), self._p(d[2]), self._p(d[3]), float(c['scale']),
                                        self._p(d[4]), XP, self._p(tabs[0]), self._p(tabs[1]), *gargs, kind, B, ab.EX,
                                        self._p(y), YP, self._p(part), gn_G, self._p(flag), self._p(ws), self._stream())
        torch.cuda.synchronize(self.dev)
        yb = y.cpu()
        f = ws[:(5 * C * C + 2 * C) * 4].view(F32).cpu()
        CC = C * C
        fold = dict(at=f[:CC].view(C, C), wg=f[CC:2 * CC].view(C, C), w=f[2 * CC:2 * CC + C], cb=f[2 * CC + C:2 * CC + 2 * C],
                    wgp=f[2 * CC + 2 * C:3 * CC + 2 * C].view(C, C), at_t=f[3 * CC + 2 * C:4 * CC + 2 * C].view(C, C),
                    wg_t=f[4 * CC + 2 * C:5 * CC + 2 * C].view(C, C))
        return dict(rc=rc, ybuf=yb, y=yb[:B * L, :C].reshape(B, L, C), flag=int(flag.item()),
                    part=None if part is None else part.cpu(), nslot=nslot, fold=fold)


@pytest.fixture(scope='module')
def dev(cuda):
    return Device(cuda)


_CACHE = {}


def launch(dev, fam, kind, B):
    """The (family, kind, B) launch shared by sections a, b, c, d, f and g: CPU tensors, not to be modified."""
    key = (fam, kind, B)
    if key not in _CACHE:
        _CACHE[key] = dev.run(ab.case(fam, _L(kind), B), kind)
    return _CACHE[key]


@functools.lru_cache(maxsize=None)
def _module_refs(fam, L, B):
    return ab.module_refs(ab.case(fam, L, B))


def check_buffers(r, B, L):
    """rc, the NaN pads and tail of y, a finite interior."""
    assert r['rc'] == 0
    yb = r['ybuf']
    assert torch.isnan(yb[:, C:]).all() and torch.isnan(yb[B * L:]).all(), 'y: pad columns or tail written'
    assert torch.isfinite(r['y']).all(), 'y: not finite (or a row not written)'


def _worst(report, key, val):
    _WORST[key] = max(_WORST.get(key, 0.0), val)
    report(key, _WORST[key])


def _over(err, e):
    return err / e if e > 0 else (0.0 if err == 0 else float('inf'))


CASES = [(k, f, B) for k in KINDS for f in ab.FAMILIES for B in (1, 3)]


@pytest.mark.parametrize('kind,fam,B', CASES)
def test_kernel_accuracy(dev, report, kind, fam, B):
    """a, g. -> err / e32f per case, the section's worst err / bound."""
    c = ab.case(fam, _L(kind), B)
    r = launch(dev, fam, kind, B)
    check_buffers(r, B, c['L'])
    kr = ab.kernel_refs(c, r['fold'], decoded=kind != 16)
    err = float((r['y'].double() - kr['ref']).abs().max())
    report(f'attn_block_fold_k{kind}_{fam}_b{B}_err_over_e32', _over(err, kr['e32f']))
    _worst(report, f'attn_block_a_k{kind}_worst_err_over_bound', err / kr['bound'])
    print(f'a k{kind} {fam} B{B}: err {err:.3e} e32f {kr["e32f"]:.3e} bound {kr["bound"]:.3e}')
    assert err <= kr['bound'], (err, kr['bound'], kr['e32f'], kr['scale'])
    assert r['flag'] == 0


@pytest.mark.parametrize('kind,fam,B', CASES)
def test_module_accuracy(dev, report, kind, fam, B):
    """b. -> err / e32 per case, the section's worst err / bound."""
    r = launch(dev, fam, kind, B)
    check_buffers(r, B, _L(kind))
    mr = _module_refs(fam, _L(kind), B)
    err = float((r['y'].double() - mr['ref']).abs().max())
    report(f'attn_block_module_k{kind}_{fam}_b{B}_err_over_e32', _over(err, mr['e32']))
    _worst(report, f'attn_block_b_k{kind}_worst_err_over_bound', err / mr['bound'])
    print(f'b k{kind} {fam} B{B}: err {err:.3e} e32 {mr["e32"]:.3e} bound {mr["bound"]:.3e}')
    assert err <= mr['bound'], (err, mr['bound'], mr['e32'], mr['scale'])


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('kind', KINDS)
def test_key_selection(dev, report, kind, B):
    """c."""
    c = ab.case('select', _L(kind), B)
    r = launch(dev, 'select', kind, B)
    check_buffers(r, B, c['L'])
    g, y = ab.select_answer(c)
    err = float((r['y'].double() - y).abs().max())
    bound = 2.0 ** -20 * float(g.abs().max())
    _worst(report, f'attn_block_c_k{kind}_worst_err_over_bound', err / bound)
    assert err <= bound, (err, bound)


@pytest.mark.parametrize('fam', ID_FAMS)
def test_variant3_equals_variant4(dev, fam):
    """d."""
    for B in (1, 3):
        a, b = launch(dev, fam, 3, B), launch(dev, fam, 4, B)
        check_buffers(a, B, 256)
        check_buffers(b, B, 256)
        assert torch.equal(a['y'], b['y'])


@pytest.mark.parametrize('kind', [4, 16])
@pytest.mark.parametrize('fam', ID_FAMS)
def test_in_kernel_finalize_equals_the_tables(dev, kind, fam):
    """d. GroupNorm(32) of x from float64 chunk partials made here (4 chunks of 64 pixels at L = 256, 1 at L = 16):
    gamma / beta chosen so that image 0 keeps the family's xn, hence its scores."""
    B, L, G = 3, _L(kind), 32
    c = ab.case(fam, L, B)
    part = ab.partials_of(c['x'], G)                           # [B, nchunk, G, 2]
    assert part.shape[1] == (4 if L == 256 else 1)
    mean, var = nr.group_moments(part, L * (C // G))
    rs = (var[0] + nr.EPS).rsqrt().repeat_interleave(C // G)
    mu = mean[0].repeat_interleave(C // G)
    gamma = (c['gsc'][0].double() / rs).to(F32)
    beta = (c['gsh'][0].double() + c['gsc'][0].double() * mu).to(F32)
    gsc, gsh = dev.finalize(part, B, L, G, gamma, beta)
    assert float((gsc[0] - c['gsc'][0]).abs().max()) <= 1e-5 * float(c['gsc'][0].abs().max())
    t = dev.run(c, kind, gsc=gsc, gsh=gsh, gn_G=G)
    k = dev.run(c, kind, gin=dict(part=part, G=G, gamma=gamma, beta=beta), gn_G=G)
    check_buffers(t, B, L)
    check_buffers(k, B, L)
    assert torch.equal(t['y'], k['y']) and torch.equal(t['part'], k['part'])
    assert t['flag'] == 0 and k['flag'] == 0


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('fam', ID_FAMS)
def test_images_are_independent(dev, kind, fam):
    """d. Image 1 of 3 replaced (by image 0's rows reversed): images 0 and 2 keep their rows and statistics slots,
    image 1 changes both."""
    B, L, G = 3, _L(kind), 32
    c = ab.case(fam, L, B)
    x2 = c['x'].clone()
    x2[1] = c['x'][0].flip(0)
    a, b = dev.run(c, kind, gn_G=G), dev.run(c, kind, gn_G=G, x=x2)
    check_buffers(a, B, L)
    check_buffers(b, B, L)
    assert torch.equal(a['y'], launch(dev, fam, kind, B)['y'])   # the statistics do not change y
    nch = nr.nchunks(L)
    pa, pb = a['part'][:a['nslot']].view(B, nch * G, 2), b['part'][:b['nslot']].view(B, nch * G, 2)
    for i in (0, 2):
        assert torch.equal(a['y'][i], b['y'][i]) and torch.equal(pa[i], pb[i])
    assert not torch.equal(a['y'][1], b['y'][1])
    assert (pa[1] != pb[1]).all()


STATS = [(k, G) for k in (3, 4) for G in (8, 16, 32, 64)] + [(16, G) for G in (4, 8, 16, 32, 64)]


@pytest.mark.parametrize('kind,G', STATS)
def test_emitted_groupnorm_statistics(dev, report, kind, G):
    """e. [B][4][G] (attn_block) / [B][G] (attn_small) slots against the float64 sums of the stored y."""
    B, L = 3, _L(kind)
    r = dev.run(ab.case('peaked', L, B), kind, gn_G=G)
    check_buffers(r, B, L)
    assert torch.equal(r['y'], launch(dev, 'peaked', kind, B)['y'])
    ref, bound = nr.partial_ref(r['y'], G)
    got = r['part'][:r['nslot']].view(B, nr.nchunks(L), G, 2)
    assert (r['part'][r['nslot']:] == SENT).all(), 'spare slots written'
    assert torch.isfinite(got).all() and (got != SENT).all()
    ratio = nr.ratio((got - ref).abs(), bound)
    _worst(report, f'attn_block_e_k{kind}_worst_err_over_bound', ratio)
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize('kind,G,gin', [(3, 128, False), (4, 128, False), (3, 4, False), (4, 4, False), (16, 128, False),
                                        (5, 32, False), (0, 0, False), (3, 32, True)])
def test_refusals_write_nothing(dev, kind, G, gin):
    """e. cpg 2 and cpg 64 (attn_block), cpg 2 (attn_small), a kind that is no kernel, and variant 3 with the in-kernel
    finalize: the launcher's error code, y and the statistics untouched."""
    L = 16 if kind == 16 else 256
    c = ab.case('flat', L, 1)
    g = None
    if gin:
        g = dict(part=ab.partials_of(c['x'], 32), G=32, gamma=torch.ones(C), beta=torch.zeros(C))
    r = dev.run(c, kind, gn_G=G, gin=g)
    assert r['rc'] == nr.ERR
    assert torch.isnan(r['ybuf']).all()
    assert r['part'] is None or (r['part'] == SENT).all()
    assert r['flag'] == 0


@pytest.mark.parametrize('kind', [4, 16])
@pytest.mark.parametrize('fam', ['flat', 'ramp200', 'bigbk', 'tiny', 'zeroq', 'select'])
def test_fold_helpers(dev, report, fam, kind):
    """f. at, w, wg, cb within 2^-24 |v| + C 2^-53 sum|term| of the float64 products; wgp, at_t, wg_t exact. (Kind 16
    is the same fold on the 16-token case's own weights.)"""
    c = ab.case(fam, _L(kind), 1)
    f = launch(dev, fam, kind, 1)['fold']
    ref, bound = ab.fold_f64(c)
    for k in ('at', 'w', 'wg', 'cb'):
        ratio = nr.ratio((f[k].double() - ref[k]).abs(), bound[k])
        _worst(report, 'attn_block_f_worst_err_over_bound', ratio)
        assert ratio <= 1.0, (k, ratio)
    assert torch.equal(f['wgp'], f['wg'][:, ab.PIPI])
    assert torch.equal(f['at_t'], f['at'].T) and torch.equal(f['wg_t'], f['wg'].T)
    if fam == 'select':
        assert torch.equal(f['at'], c['Wq'])
    if kind == 4:   # variant 3 folds alike
        g = launch(dev, fam, 3, 1)['fold']
        assert all(torch.equal(f[k], g[k]) for k in f)


@pytest.mark.parametrize('kind', KINDS)
def test_range_flag(dev, kind):
    """g. gnwide (max |xn| 2^6 = 57600) leaves the flag at 0, its twin (70400) raises it; attn_small is fp32 and has
    no flag. The twin's output is not checked."""
    B, L = 3, _L(kind)
    c = ab.case('gnwide', L, B)
    assert launch(dev, 'gnwide', kind, B)['flag'] == 0
    r = dev.run(ab.gnwide_twin(c), kind)
    assert r['rc'] == 0
    assert r['flag'] == (0 if kind == 16 else 1)
