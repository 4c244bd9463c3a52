"""Operator-level tests of the GroupNorm chain (csrc/gn.hip: gn_partial, gn_apply, gn_finalize and its wide form,
gn_concat_stats) and of the first / last convs and resample2x (csrc/elementwise.hip: conv3x3_small_in_kernel<1..4>
with its chunk-aware statistics flush, conv3x3_small_out2_kernel<1..8> with the table and the in-kernel (GnFin)
prologue, resample2x_kernel), each launched alone on the test's own buffers; and of the GroupNorm statistics the conv
epilogues emit (ConvArgs::gn_part through dm_debug_conv2d_gn: the fp32 halo-patch tile, conv_patch3 in both split
kinds and its 1x1 mode, every conv_k32 variant that emits, both split-K reductions, conv_wino, the sub-pixel forms),
slot by slot against the float64 sums of the stored output (the fp32 / fp16x2 GEMM's through dm_debug_gemm_gn); and of
the convs' in-kernel finalize of their GroupNorm prologue (ConvArgs::gin_* through dm_debug_conv2d_gin), bit for bit
against the table form.

dm_groupnorm_nhwc / dm_groupnorm_affine run with the test's scratch, so every chunk partial is read back; the hooks
dm_debug_gn_finalize, dm_debug_gn_concat_stats, dm_debug_conv3x3_small_in, dm_debug_conv3x3_small_out and
dm_debug_resample2x launch the rest. Inputs, float64 references and the derived bounds are tests/norm_ref.py's: a
partial slot within n 2^-52 sum|term| of the float64 sum of the stored values, the finalize tables within 2^-22 of the
float64 tables from the same partials, gn_apply's output within 2^-21 (|x sc| + |sc mu| + |beta|); integer operands
make the convs and the resampling exact, and the in-kernel finalize must equal the table form bit for bit. Image b of
every batch is scaled by 4^b and shifted by 10 b, pitched inputs carry NaN in their pad columns, every output is
NaN-prefilled with a tail that must survive, and every refusal must leave its outputs untouched.

The checks are functions of a backend: DeviceBackend here (ctypes on the library), norm_ref.EmuBackend in
tests/test_norm_host.py, which dry-runs them on the CPU and shows that each of its mutants (a wrong image index, a
dropped chunk, a late slot, fp32 sums, no clamp, an ignored pitch, a pad column, a wrong concat boundary) fails one.
Each check returns its worst err / bound, which goes to the parity report.
"""
import ctypes

import pytest
import torch

from tests import norm_ref as nr

pytestmark = pytest.mark.gpu

vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
F64 = torch.float64


class DeviceBackend:
    """The library on the GPU. Arguments and results are CPU tensors (norm_ref.EmuBackend has the same interface);
    every output buffer is allocated here with its NaN prefill and tail."""
    name = 'device'

    def __init__(self, dev):
        from dmhip import _lib
        self.dev, self._lib, self.L = dev, _lib, _lib.load()
        self.L.dm_debug_gn_finalize.argtypes = [vp, ci, ci, ci, ci, cf, vp, vp, vp, vp, ci, vp, vp, vp]
        self.L.dm_debug_gn_concat_stats.argtypes = [vp, ci, ci, vp, ci, ci, ci, ci, ci, vp, vp]
        self.L.dm_debug_conv3x3_small_in.argtypes = [vp, ci, ci, ci, ci, vp, vp, ci, vp, ci, vp, ci, vp]
        self.L.dm_debug_conv3x3_small_out.argtypes = [vp, ci, ci, ci, ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, cf,
                                                      vp, vp, vp]
        self.L.dm_debug_resample2x.argtypes = [vp, ci, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp]
        self.L.dm_debug_conv2d_gin.argtypes = [vp, ci, vp, ci, ci, cf, vp, vp, vp, vp, ci, vp]
        self.L.dm_debug_gemm_gn.argtypes = [vp, ci, ci, vp, vp]

    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def _up(self, t):
        return None if t is None else t.contiguous().to(self.dev)

    def _nan(self, shape, dtype=torch.float32):
        return torch.full(shape, nr.NAN, dtype=dtype, device=self.dev)

    @staticmethod
    def _p(t, off=0):
        return None if t is None else t.data_ptr() + 4 * off

    def _sync(self):
        torch.cuda.synchronize(self.dev)

    def gn_partial(self, xbuf, off, C, G):
        return self.gn_affine(xbuf, off, C, G, nr.EPS)['part']

    def gn_affine(self, xbuf, off, C, G, eps, gamma=None, beta=None):
        B, HW, pitch = xbuf.shape
        xd, ga, be = self._up(xbuf), self._up(gamma), self._up(beta)
        part = self._nan((B * nr.nchunks(HW) * G + nr.TAIL, 2), F64)
        sc, sh = self._nan((B + 1, C)), self._nan((B + 1, C))
        rc = self.L.dm_groupnorm_affine(self._p(xd, off), pitch, B, HW, C, G, eps, self._p(ga), self._p(be), self._p(sc),
                                        self._p(sh), self._p(part), self._stream())
        self._sync()
        return dict(part=part.cpu(), sc=sc.cpu(), sh=sh.cpu(), rc=rc)

    def gn_finalize(self, part, B, HW, C, G, eps, gamma=None, beta=None, modbuf=None, so=None, bo=None):
        pd, ga, be, mod = self._up(part), self._up(gamma), self._up(beta), self._up(modbuf)
        sc, sh = self._nan((B + 1, C)), self._nan((B + 1, C))
        rc = self.L.dm_debug_gn_finalize(self._p(pd), B, HW, C, G, eps, self._p(ga), self._p(be),
                                         None if so is None else self._p(mod, so), None if bo is None else self._p(mod, bo),
                                         0 if mod is None else mod.shape[1], self._p(sc), self._p(sh), self._stream())
        return dict(sc=sc.cpu(), sh=sh.cpu(), rc=rc)

    def groupnorm(self, xbuf, off, C, G, eps, gamma=None, beta=None, modbuf=None, so=None, bo=None, silu=False,
                  y_pitch=None):
        B, HW, pitch = xbuf.shape
        y_pitch = y_pitch or C
        xd, ga, be, mod = self._up(xbuf), self._up(gamma), self._up(beta), self._up(modbuf)
        part = self._nan((B * nr.nchunks(HW) * G + nr.TAIL, 2), F64)
        y = self._nan((B * HW + nr.TAIL, y_pitch))
        rc = self.L.dm_groupnorm_nhwc(self._p(xd, off), pitch, self._p(y), y_pitch, B, HW, C, G, eps, self._p(ga), self._p(be),
                                      None if so is None else self._p(mod, so), None if bo is None else self._p(mod, bo),
                                      0 if mod is None else mod.shape[1], int(silu), self._p(part), self._stream())
        self._sync()
        return dict(part=part.cpu(), y=y.cpu(), rc=rc)

    def gn_concat(self, ph, Ch, Gh, ps, Cs, Gs, B, HW, G):
        hd, sd = self._up(ph), self._up(ps)
        out = self._nan((B * nr.nchunks(HW) * max(G, 1) + nr.TAIL, 2), F64)
        rc = self.L.dm_debug_gn_concat_stats(self._p(hd), Ch, Gh, self._p(sd), Cs, Gs, B, HW, G, self._p(out), self._stream())
        return dict(out=out.cpu(), rc=rc)

    def small_in(self, x, w, bias, y_pitch, G=0):
        B, Cin, H, W = x.shape
        Cout = w.shape[0]
        xd, wd, bd = self._up(x), self._up(w), self._up(bias)
        y = self._nan((B * H * W + nr.TAIL, y_pitch))
        part = None if G == 0 else self._nan((B * nr.nchunks(H * W) * G + nr.TAIL, 2), F64)
        rc = self.L.dm_debug_conv3x3_small_in(self._p(xd), B, Cin, H, W, self._p(wd), self._p(bd), Cout, self._p(y), y_pitch,
                                              self._p(part), G, self._stream())
        return dict(y=y.cpu(), part=None if part is None else part.cpu(), rc=rc)

    def small_out(self, xbuf, Cin, w, bias, pro=None, fin=None):
        B, H, W, pitch = xbuf.shape
        Cout = w.shape[0]
        xd, wd, bd = self._up(xbuf), self._up(w), self._up(bias)
        nwp = 9 * Cin * ((Cout + 1) & ~1)
        wp = self._nan((nwp + nr.TAIL, ))
        y = self._nan((B + 1, Cout, H, W))
        sc = sh = fp = ga = be = None
        fG = fn = 0
        feps = nr.EPS
        if pro is not None:
            sc, sh = self._up(pro[0]), self._up(pro[1])
        if fin is not None:
            fp, ga, be = self._up(fin['part']), self._up(fin['gamma']), self._up(fin['beta'])
            fG, fn, feps = fin['G'], fin['nchunk'], fin['eps']
        rc = self.L.dm_debug_conv3x3_small_out(self._p(xd), B, H, W, Cin, pitch, self._p(wd), self._p(wp), self._p(bd), Cout,
                                               self._p(y), self._p(sc), self._p(sh), self._p(fp), fG, fn, feps, self._p(ga),
                                               self._p(be), self._stream())
        return dict(y=y.cpu(), wp_tail_ok=bool(torch.isnan(wp[nwp:]).all()), rc=rc)

    def resample(self, xbuf, C, y_pitch, down, pro=None):
        B, H, W, xp = xbuf.shape
        Ho, Wo = (H // 2, W // 2) if down else (2 * H, 2 * W)
        xd = self._up(xbuf)
        sc, sh = (None, None) if pro is None else (self._up(pro[0]), self._up(pro[1]))
        y = self._nan((B * Ho * Wo + nr.TAIL, y_pitch))
        rc = self.L.dm_debug_resample2x(self._p(xd), xp, self._p(y), y_pitch, B, C, H, W, int(down), self._p(sc), self._p(sh),
                                        self._stream())
        return dict(y=y.cpu(), Ho=Ho, Wo=Wo, rc=rc)


    def _conv_desc(self, s, c, pro=None, nosilu=0):
        """(dm_conv_desc without y, keep-alive tensors, rows) of a conv case (bias, rowvec, residual, pitched output)."""
        import dmhip
        from tests.test_gpu_ops import _nhwc, _pack, _pack_subpix
        B, Cin, Cout, H, W, Ho, Wo = s['B'], s['Cin'], s['Cout'], s['H'], s['W'], c['Ho'], c['Wo']
        taps, up = s.get('taps', 9), s.get('up', 0)
        rows = B * Ho * Wo
        xd = _nhwc(c['x']).to(self.dev)
        wp = _pack_subpix(c['w'], self.dev) if up == 2 else _pack(c['w'], self.dev)
        bd, rv, res = self._up(c['bias']), self._up(c['rowvec']), self._up(c['res'])
        keep = [xd, wp, bd, rv, res]
        d = dmhip.ConvDesc()
        d.x, d.x_pitch, d.Cin, d.Hin, d.Win = xd.data_ptr(), Cin, Cin, H, W
        d.taps, d.stride, d.upsample = taps, s.get('stride', 1), up
        d.w, d.K = wp.data_ptr(), wp.shape[1]
        d.y_pitch, d.Cout, d.B, d.Hout, d.Wout = c['y_pitch'], Cout, B, Ho, Wo
        d.bias, d.rowvec, d.rowvec_pitch, d.res, d.res_pitch = bd.data_ptr(), rv.data_ptr(), Cout, res.data_ptr(), Cout
        d.tile, d.pro_nosilu = s['tile'], nosilu
        if pro is not None:
            keep += [self._up(pro[0]), self._up(pro[1])]
            d.pro_scale, d.pro_shift = keep[-2].data_ptr(), keep[-1].data_ptr()
        if s['split']:
            kind = dmhip.SPLIT_FP16X2 if s['split'] == 'fp16x2' else dmhip.SPLIT_BF16X3
            nmat, ntap = (4, 4) if up == 2 else (1, taps)
            ws = dmhip.pack_conv_weight_split(wp, nmat, Cin, ntap, kind)
            d.w_split, d.w_split_kind = ws.data_ptr(), kind
            keep.append(ws)
        if s.get('wino'):
            ww = dmhip.pack_conv_weight_wino(wp, Cin, 0, False)
            d.w_wino, d.w_wino_fold = ww.data_ptr(), 0
            keep.append(ww)
        if s.get('ksplit', 0) > 1:
            kpart = torch.empty((s['ksplit'], rows, Cout), device=self.dev)
            d.ksplit, d.kpart = s['ksplit'], kpart.data_ptr()
            keep.append(kpart)
        return d, keep, rows

    def conv_gn(self, s, G):
        import dmhip
        c = nr.conv_case(s)
        d, keep, rows = self._conv_desc(s, c)
        nch = nr.nchunks(c['Ho'] * c['Wo'])
        pad0 = int(bool(s.get('s2_pad0')))
        y0, y1 = self._nan((rows + nr.TAIL, c['y_pitch'])), self._nan((rows + nr.TAIL, c['y_pitch']))
        part = self._nan((s['B'] * nch * G + nr.TAIL, 2), F64)
        d.y = y0.data_ptr()
        rc0 = (self.L.dm_conv2d_nhwc_s2pad0 if pad0 else self.L.dm_conv2d_nhwc)(ctypes.byref(d), self._stream())
        self._sync()
        assert rc0 == 0, (rc0, self.L.dm_last_error())
        d.y = y1.data_ptr()
        dmhip.launch_log(True)
        rc = self.L.dm_debug_conv2d_gn(ctypes.byref(d), pad0, G, self._p(part), self._stream())
        self._sync()
        log = dmhip.launch_log_read()
        dmhip.launch_log(False)
        del keep
        return dict(y0=y0.cpu(), y1=y1.cpu(), part=part.cpu(), log=log, rc=rc)

    def conv_gin(self, s, mod, nosilu):
        c = nr.gin_case(s, mod)
        B, Cin, HW, G = s['B'], s['Cin'], s['H'] * s['W'], c['G']
        t = self.gn_finalize(c['part'], B, HW, Cin, G, c['eps'], c['gamma'], c['beta'], c['modbuf'], c['so'], c['bo'])
        assert t['rc'] == 0, t['rc']
        d, keep, rows = self._conv_desc(s, c, pro=(t['sc'][:B], t['sh'][:B]), nosilu=nosilu)
        y_tab, y_gin = self._nan((rows + nr.TAIL, c['y_pitch'])), self._nan((rows + nr.TAIL, c['y_pitch']))
        d.y = y_tab.data_ptr()
        rc0 = self.L.dm_conv2d_nhwc(ctypes.byref(d), self._stream())
        self._sync()
        assert rc0 == 0, (rc0, self.L.dm_last_error())
        d.y, d.pro_scale, d.pro_shift = y_gin.data_ptr(), None, None
        pd, ga, be, mb = self._up(c['part']), self._up(c['gamma']), self._up(c['beta']), self._up(c['modbuf'])
        import dmhip
        dmhip.launch_log(True)
        rc = self.L.dm_debug_conv2d_gin(ctypes.byref(d), 0, self._p(pd), G, nr.nchunks(HW), c['eps'], self._p(ga), self._p(be),
                                        None if mb is None else self._p(mb, c['so']),
                                        None if mb is None else self._p(mb, c['bo']),
                                        0 if mb is None else mb.shape[1], self._stream())
        self._sync()
        log = dmhip.launch_log_read()
        dmhip.launch_log(False)
        del keep
        return dict(y_tab=y_tab.cpu(), y_gin=y_gin.cpu(), log=log, rc=rc)

    def gemm_gn(self, s, G):
        import dmhip
        c = nr.gemm_case(s)
        (M, K), N, hw = c['A'].shape, c['W'].shape[0], s['hw']
        A, W, bias, res = self._up(c['A']), self._up(c['W']), self._up(c['bias']), self._up(c['res'])
        flag = torch.zeros((1, ), dtype=torch.int32, device=self.dev)
        y0, y1 = self._nan((M + nr.TAIL, c['ldc'])), self._nan((M + nr.TAIL, c['ldc']))
        part = self._nan(((M // hw) * nr.nchunks(hw) * G + nr.TAIL, 2), F64)
        d = dmhip.GemmDesc()
        d.M, d.N, d.K, d.Z1, d.Z2, d.alpha = M, N, K, 1, 1, 1.0
        d.A, d.lda, d.B, d.ldb, d.ldc = A.data_ptr(), K, W.data_ptr(), K, c['ldc']
        d.bias, d.res, d.ld_res = bias.data_ptr(), res.data_ptr(), N
        d.split, d.split_ea, d.split_eb, d.range_flag = s['split'], 6, 6, flag.data_ptr()
        d.C = y0.data_ptr()
        rc0 = self.L.dm_gemm(ctypes.byref(d), self._stream())
        self._sync()
        assert rc0 == 0, (rc0, self.L.dm_last_error())
        d.C = y1.data_ptr()
        rc = self.L.dm_debug_gemm_gn(ctypes.byref(d), G, hw, self._p(part), self._stream())
        self._sync()
        assert int(flag.item()) == 0, 'an operand beyond the fp16 range'
        return dict(y0=y0.cpu(), y1=y1.cpu(), part=part.cpu(), rc=rc)

@pytest.fixture(scope='module')
def be(cuda):
    return DeviceBackend(cuda)


# ----------------------------------------------------------------------------------------------- the checks
def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == F64 else torch.int32)


def checked_part(flat, n):
    """A partial buffer [n + TAIL, 2]: every slot written, the tail untouched -> [n, 2]."""
    assert flat.shape[0] == n + nr.TAIL
    assert torch.isnan(flat[n:]).all(), 'a partial was written past the buffer'
    assert not torch.isnan(flat[:n]).any(), 'a partial slot was left unwritten (or is NaN)'
    return flat[:n]


def checked_rows(y, rows, C):
    """An NHWC output [rows + TAIL, pitch]: the pad columns and the tail rows still NaN, [rows][C] finite."""
    assert y.shape[0] == rows + nr.TAIL
    assert torch.isnan(y[:, C:]).all(), 'the kernel wrote the pad columns'
    assert torch.isnan(y[rows:]).all(), 'the kernel wrote rows past the output'
    assert torch.isfinite(y[:rows, :C]).all(), 'a NaN / inf inside the output'
    return y[:rows, :C]


def checked_tables(r, B):
    assert r['rc'] == 0, r['rc']
    for t in (r['sc'], r['sh']):
        assert torch.isnan(t[B:]).all(), 'a table was written past image B'
        assert torch.isfinite(t[:B]).all(), 'a NaN / inf inside a table'
    return r['sc'][:B], r['sh'][:B]


def untouched(*ts):
    return all(t is None or bool(torch.isnan(t).all()) for t in ts)


def _mod(c):
    C = c['C']
    ms = None if c['so'] is None else c['modbuf'][:, c['so']:c['so'] + C]
    mb = None if c['bo'] is None else c['modbuf'][:, c['bo']:c['bo'] + C]
    return ms, mb


def check_groupnorm(be, shape, fam, variant='default'):
    """a. dm_groupnorm_nhwc: every partial slot against the float64 sums of the input, every output element against
    the float64 apply from those partials. -> (worst partial ratio, worst output ratio)."""
    c = nr.gn_case(shape, fam, variant)
    B, C, HW, G = shape
    r = be.groupnorm(c['xbuf'], c['off'], C, G, c['eps'], c['gamma'], c['beta'], c['modbuf'], c['so'], c['bo'], c['silu'],
                     c['y_pitch'])
    assert r['rc'] == 0, r['rc']
    nch = nr.nchunks(HW)
    part = checked_part(r['part'], B * nch * G).view(B, nch, G, 2)
    ref, bound = nr.partial_ref(c['x'], G)
    rp = nr.ratio((part - ref).abs(), bound)
    assert rp <= 1.0, f'partials: err / bound {rp:.3g}'
    y = checked_rows(r['y'], B * HW, C).view(B, HW, C)
    ms, mb = _mod(c)
    yref, yb = nr.apply_ref(c['x'], part, G, c['eps'], c['gamma'], c['beta'], ms, mb, c['silu'])
    ry = nr.ratio((y.to(F64) - yref).abs(), yb)
    assert ry <= 1.0, f'output: err / bound {ry:.3g}'
    return rp, ry


def _flat(part):
    return torch.cat([part.reshape(-1, 2), torch.full((nr.TAIL, 2), nr.NAN, dtype=F64)])


def check_finalize(be, HW, C, G, mode, flavour):
    """b. dm_debug_gn_finalize on CPU-built partials. -> worst table ratio."""
    c = nr.fin_case(HW, C, G, mode, flavour)
    B = c['B']
    r = be.gn_finalize(_flat(c['part']), B, HW, C, G, c['eps'], c['gamma'], c['beta'], c['modbuf'], c['so'], c['bo'])
    sc, sh = checked_tables(r, B)
    ms, mb = _mod(c)
    fr = nr.finalize_ref(c['part'], HW, C, c['eps'], c['gamma'], c['beta'], ms, mb)
    rs = nr.ratio((sc.to(F64) - fr['sc']).abs(), fr['sc_bound'])
    rh = nr.ratio((sh.to(F64) - fr['sh']).abs(), fr['sh_bound'])
    assert rs <= 1.0 and rh <= 1.0, f'{flavour}: scale err / bound {rs:.3g}, shift {rh:.3g}'
    return max(rs, rh)


def check_finalize_rechunk(be):
    """b. One tensor's partials as 65 chunks (wide kernel) and as 64 (narrow): each form's group tables within the
    bound of the other's reference."""
    c = nr.rechunk_case()
    B, G = c['B'], c['G']
    got, ref = {}, {}
    for k in ('wide', 'narrow'):
        f = c[k]
        cpg = f['C'] // G
        sc, sh = checked_tables(be.gn_finalize(_flat(f['part']), B, f['HW'], f['C'], G, nr.EPS), B)
        assert torch.equal(sc.view(B, G, cpg), sc.view(B, G, cpg)[:, :, :1].expand(B, G, cpg))
        fr = nr.finalize_ref(f['part'], f['HW'], f['C'], nr.EPS)
        got[k] = (sc[:, ::cpg].to(F64), sh[:, ::cpg].to(F64))
        ref[k] = tuple(fr[n][:, ::cpg] for n in ('sc', 'sh', 'sc_bound', 'sh_bound'))
    worst = 0.0
    for a in ('wide', 'narrow'):
        for b in ('wide', 'narrow'):
            rs = nr.ratio((got[a][0] - ref[b][0]).abs(), ref[b][2])
            rh = nr.ratio((got[a][1] - ref[b][1]).abs(), ref[b][3])
            assert rs <= 1.0 and rh <= 1.0, f'{a} tables against the {b} reference: {rs:.3g}, {rh:.3g}'
            worst = max(worst, rs, rh)
    return worst


def check_affine_equals_hook(be, shape, fam='benign'):
    """b. dm_groupnorm_affine's tables equal dm_debug_gn_finalize's on the scratch it leaves, bit for bit."""
    c = nr.gn_case(shape, fam)
    B, C, HW, G = shape
    a = be.gn_affine(c['xbuf'], c['off'], C, G, c['eps'], c['gamma'], c['beta'])
    sc, sh = checked_tables(a, B)
    checked_part(a['part'], B * nr.nchunks(HW) * G)
    sc2, sh2 = checked_tables(be.gn_finalize(a['part'], B, HW, C, G, c['eps'], c['gamma'], c['beta']), B)
    assert torch.equal(bits(sc), bits(sc2)) and torch.equal(bits(sh), bits(sh2))
    fr = nr.finalize_ref(a['part'][:B * nr.nchunks(HW) * G].view(B, -1, G, 2), HW, C, c['eps'], c['gamma'], c['beta'])
    r = max(nr.ratio((sc.to(F64) - fr['sc']).abs(), fr['sc_bound']), nr.ratio((sh.to(F64) - fr['sh']).abs(), fr['sh_bound']))
    assert r <= 1.0, r
    return r


def check_concat(be, case, HW):
    """c. gn_concat_stats on the slices' own partials (gn_partial on channel slices of the concat buffer): bit-identical
    to the ordered float64 restatement, and within the partial bound of the float64 sums of the materialised concat,
    as gn_partial on the whole concat is. -> worst ratio."""
    Ch, Gh, Cs, Gs, G = case
    x = nr.concat_case(Ch, Cs, HW)
    B, nch = x.shape[0], nr.nchunks(HW)
    ph, ps = be.gn_partial(x, 0, Ch, Gh), be.gn_partial(x, Ch, Cs, Gs)
    h = checked_part(ph, B * nch * Gh).view(B, nch, Gh, 2)
    s = checked_part(ps, B * nch * Gs).view(B, nch, Gs, 2)
    worst = 0.0
    for got, xs, g in ((h, x[:, :, :Ch], Gh), (s, x[:, :, Ch:], Gs)):   # a channel slice of a wider tensor
        ref, bound = nr.partial_ref(xs, g)
        worst = max(worst, nr.ratio((got - ref).abs(), bound))
    assert worst <= 1.0, f'slice partials: err / bound {worst:.3g}'
    r = be.gn_concat(ph, Ch, Gh, ps, Cs, Gs, B, HW, G)
    assert r['rc'] == 0, r['rc']
    out = checked_part(r['out'], B * nch * G).view(B, nch, G, 2)
    assert torch.equal(bits(out), bits(nr.concat_ordered(h, s, Ch, Cs, G))), 'not the documented summation order'
    ref, bound = nr.partial_ref(x, G)
    full = checked_part(be.gn_partial(x, 0, Ch + Cs, G), B * nch * G).view(B, nch, G, 2)
    rc_, rf = nr.ratio((out - ref).abs(), bound), nr.ratio((full - ref).abs(), bound)
    assert rc_ <= 1.0 and rf <= 1.0, f'concat {rc_:.3g}, gn_partial on the concat {rf:.3g}'
    return max(worst, rc_, rf)


def check_concat_refused(be, case):
    Ch, Gh, Cs, Gs, G = case
    assert not nr.concat_ok(*case)
    B, HW = 2, 64
    ph = torch.ones((B * max(Gh, 1) + nr.TAIL, 2), dtype=F64)
    ps = torch.ones((B * max(Gs, 1) + nr.TAIL, 2), dtype=F64)
    r = be.gn_concat(ph, Ch, Gh, ps, Cs, Gs, B, HW, G)
    assert r['rc'] != 0 and untouched(r['out']), (r['rc'], 'out was written by a refused call')


def check_conv_gn(be, s, G):
    """d. Statistics emitted by a conv's epilogue: the intended kernel ran, y is bit-identical to the same call
    without statistics, every slot of [B][nchunk][G] is written and the tail is not, and each slot (64 consecutive
    pixels) -- or, where the kernel documents any disjoint cover, each (image, group) total -- is within the
    partial bound of the float64 sums of the stored output. -> worst ratio."""
    r = be.conv_gn(s, G)
    assert r['rc'] == 0, (s['name'], G, r['rc'])
    assert any(s['kernel'] in ln for ln in r['log']), (s['kernel'], r['log'])
    B, Cout = s['B'], s['Cout']
    rows = r['y0'].shape[0] - nr.TAIL
    HW = rows // B
    y0, y1 = checked_rows(r['y0'], rows, Cout), checked_rows(r['y1'], rows, Cout)
    assert torch.equal(bits(y0), bits(y1)), 'the output changes with the statistics'
    assert float(y1.view(B, HW, Cout)[B - 1].mean()) > 50.0 * B, 'the per-image rowvec is not in the stored value'
    nch = nr.nchunks(HW)
    part = checked_part(r['part'], B * nch * G).view(B, nch, G, 2)
    ref, bound = nr.partial_ref(y1.view(B, HW, Cout), G)
    if s['layout'] == 'cover':   # n = HW cpg values per total: the slots' bounds (n_slot 2^-52 sum|term|) times nchunk
        part, ref, bound = part.sum(dim=1), ref.sum(dim=1), bound.sum(dim=1) * nch
    rr = nr.ratio((part - ref).abs(), bound)
    assert rr <= 1.0, f'{s["name"]} G = {G}: err / bound {rr:.3g}'
    return rr


def check_conv_gn_refused(be, s, G):
    """d. A shape conv_can_emit_gn refuses: an error, nothing launched (y and part stay NaN)."""
    r = be.conv_gn(s, G)
    assert r['rc'] != 0 and untouched(r['y1'], r['part']) and not r['log'], (s['name'], r['rc'], r['log'])


def check_gemm_gn(be, s):
    """d. The GEMM epilogue's statistics (gemm.hip gn_emit_group): C bit-identical to dm_gemm's, every slot within
    the partial bound of the float64 sums of the stored rows. -> worst ratio."""
    c = nr.gemm_case(s)
    M, N, hw, G = s['M'], s['N'], s['hw'], s['G']
    r = be.gemm_gn(s, G)
    assert r['rc'] == 0, (s['name'], r['rc'])
    y0, y1 = checked_rows(r['y0'], M, N), checked_rows(r['y1'], M, N)
    assert torch.equal(bits(y0), bits(y1)), 'the output changes with the statistics'
    ref = c['A'].double() @ c['W'].double().T + c['bias'].double() + c['res'].double()
    assert float((y1.double() - ref).abs().max()) < 5e-3, 'not the GEMM of the case'
    B, nch = M // hw, nr.nchunks(hw)
    part = checked_part(r['part'], B * nch * G).view(B, nch, G, 2)
    pref, bound = nr.partial_ref(y1.view(B, hw, N), G)
    rr = nr.ratio((part - pref).abs(), bound)
    assert rr <= 1.0, f'{s["name"]}: err / bound {rr:.3g}'
    return rr


def check_gemm_gn_refused(be, s):
    """d. A GEMM that runs 64-row tiles: an error, nothing launched."""
    r = be.gemm_gn(s, s['G'])
    assert r['rc'] != 0 and untouched(r['y1'], r['part']), (s['name'], r['rc'])


def check_conv_gin(be, s, mod, nosilu):
    """e. The conv's in-kernel GroupNorm finalize against the table form (tables from dm_debug_gn_finalize on the same
    partials, the same dispatch): bit-identical outputs."""
    r = be.conv_gin(s, mod, nosilu)
    assert r['rc'] == 0, (s['name'], r['rc'])
    assert any(s['kernel'] in ln for ln in r['log']), (s['kernel'], r['log'])
    rows = r['y_tab'].shape[0] - nr.TAIL
    yt, yg = checked_rows(r['y_tab'], rows, s['Cout']), checked_rows(r['y_gin'], rows, s['Cout'])
    assert torch.equal(bits(yt), bits(yg)), f'{s["name"]}: the in-kernel finalize differs from the table form'
    # the prologue is in the output: the same conv of the raw input is far away
    assert float(yt.view(s['B'], -1, s['Cout'])[0].std()) > 0.0


def check_conv_gin_refused(be, s):
    """e. Where ConvChoice::lds_tables is false the hook returns DM_ERR_UNSUPPORTED and launches nothing."""
    r = be.conv_gin(s, 0, 0)
    assert r['rc'] == nr.UNSUPPORTED and untouched(r['y_gin']) and not r['log'], (s['name'], r['rc'], r['log'])


def check_small_in(be, case, G):
    """f. The first conv on integer operands: bit-exact against float64 F.conv2d, without (G = 0) and with the
    GroupNorm(G) statistics; every partial slot within the bound; a shape conv3x3_small_in_can_emit (or the LDS
    budget) refuses is an error that writes nothing. -> partial ratio (0 where nothing is emitted)."""
    Cin, H, W, Cout = case
    c = nr.small_in_case(*case)
    B, HW = c['x'].shape[0], H * W
    want = c['ref'].view(B * HW, Cout)
    r = be.small_in(c['x'], c['w'], c['bias'], c['y_pitch'], G)
    if G and not (nr.small_in_can_emit(H, W, Cout, G) and nr.small_in_fits(Cin, H, W, Cout, True)):
        assert r['rc'] != 0 and untouched(r['y'], r['part']), f'a refused call returned {r["rc"]} or wrote'
        return 0.0
    assert r['rc'] == 0, r['rc']
    assert torch.equal(checked_rows(r['y'], B * HW, Cout).to(F64), want), 'the conv is not exact'
    if not G:
        return 0.0
    nch = nr.nchunks(HW)
    part = checked_part(r['part'], B * nch * G).view(B, nch, G, 2)
    ref, bound = nr.partial_ref(want.view(B, HW, Cout).float(), G)
    rp = nr.ratio((part - ref).abs(), bound)
    assert rp <= 1.0, f'partials err / bound {rp:.3g}'
    return rp


def check_small_out_int(be, case):
    """g. The last conv on integer operands (pitch > Cin, NaN pad columns): bit-exact against float64."""
    Cout, H, W, Cin = case
    c = nr.small_out_case(Cout, H, W, Cin, 'int')
    B = c['x'].shape[0]
    r = be.small_out(c['xbuf'], Cin, c['w'], c['bias'])
    assert r['rc'] == 0 and r['wp_tail_ok'], r['rc']
    assert torch.isnan(r['y'][B:]).all(), 'written past the output'
    ref, _ = nr.small_out_ref(c['x'], c['w'], c['bias'])
    assert torch.equal(r['y'][:B].to(F64), ref), 'the conv is not exact'


def check_small_out_gn(be, case):
    """g. GroupNorm(32) + SiLU prologue: the in-kernel finalize (GnFin) bit-identical to the table form (tables from
    dm_debug_gn_finalize on the same partials), and within the carried apply bound of float64. -> worst ratio."""
    Cout, H, W, Cin = case
    c = nr.small_out_case(Cout, H, W, Cin, 'gn')
    B, HW, G = c['x'].shape[0], H * W, c['G']
    xf = c['x'].view(B, HW, Cin)
    part, _ = nr.partial_ref(xf, G)
    flat = _flat(part)
    sc, sh = checked_tables(be.gn_finalize(flat, B, HW, Cin, G, c['eps'], c['gamma'], c['beta']), B)
    ra = be.small_out(c['xbuf'], Cin, c['w'], c['bias'], pro=(sc, sh))
    rb = be.small_out(c['xbuf'], Cin, c['w'], c['bias'],
                      fin=dict(part=flat, G=G, nchunk=nr.nchunks(HW), eps=c['eps'], gamma=c['gamma'], beta=c['beta']))
    for r in (ra, rb):
        assert r['rc'] == 0 and r['wp_tail_ok'], r['rc']
        assert torch.isnan(r['y'][B:]).all() and torch.isfinite(r['y'][:B]).all()
    assert torch.equal(bits(ra['y'][:B]), bits(rb['y'][:B])), 'the in-kernel finalize differs from the table form'
    fr = nr.finalize_ref(part, HW, Cin, c['eps'], c['gamma'], c['beta'])
    _, pb = nr.apply_ref(xf, part, G, c['eps'], c['gamma'], c['beta'])
    ref, bound = nr.small_out_ref(c['x'], c['w'], c['bias'], fr['sc'], fr['sh'], pb.view(B, H, W, Cin))
    rr = nr.ratio((ra['y'][:B].to(F64) - ref).abs(), bound)
    assert rr <= 1.0, f'err / bound {rr:.3g}'
    return rr


def check_small_out_refused(be):
    """g. Cin = 544 (> 512 LDS table entries) with the in-kernel finalize: an error, nothing written."""
    B, H, W, Cin, G = 1, 3, 5, 544, 32
    xbuf = torch.ones((B, H, W, Cin))
    w, bias = torch.ones((3, Cin, 3, 3)), torch.zeros((3, ))
    flat = torch.ones((B * G + nr.TAIL, 2), dtype=F64)
    r = be.small_out(xbuf, Cin, w, bias, fin=dict(part=flat, G=G, nchunk=1, eps=nr.EPS, gamma=None, beta=None))
    assert r['rc'] != 0 and untouched(r['y']), r['rc']


def check_resample(be, shape, down, kind):
    """h. resample2x with x_pitch != y_pitch != C: integer data exact against avg_pool2d / nearest-2x, the prologue
    form within the activation bound. -> ratio (0 for the exact form)."""
    c = nr.resample_case(shape, kind)
    B, C, H, W = shape
    pro = None if c['sc'] is None else (c['sc'], c['sh'])
    r = be.resample(c['xbuf'], C, c['y_pitch'], down, pro)
    assert r['rc'] == 0, r['rc']
    rows = B * r['Ho'] * r['Wo']
    y = checked_rows(r['y'], rows, C).to(F64)
    ref, bound = nr.resample_ref(c['x'], down, c['sc'], c['sh'])
    if bound is None:
        assert torch.equal(y, ref.view(rows, C)), 'not exact'
        return 0.0
    rr = nr.ratio((y - ref.view(rows, C)).abs(), bound.reshape(rows, C))
    assert rr <= 1.0, f'err / bound {rr:.3g}'
    return rr


def check_resample_refused(be):
    """h. An odd Hin with `down` set: an error, nothing written."""
    r = be.resample(torch.ones((2, 5, 10, 16)), 8, 12, True)
    assert r['rc'] != 0 and untouched(r['y']), r['rc']


# --------------------------------------------------------------------------------------------------- the cases
GN_FAMILY_CASES = [(s, f) for s in nr.GN_SHAPES
                   for f in (nr.FAMILIES if s in nr.GN_ALL_FAMILIES else ('benign', 'offset'))]
GN_VARIANT_CASES = [(s, v) for s in nr.GN_VARIANT_SHAPES for v in nr.GN_VARIANTS]
FIN_CASES = [(hw, c, g, m) for hw in nr.FIN_HW for c, g in nr.FIN_CG for m in nr.FIN_MODES]
AFFINE_SHAPES = [(3, 64, 64, 32), (1, 32, 4160, 8)]     # the narrow and the wide finalize
SO_CASES = nr.small_out_cases()
RS_CASES = [(s, d, k) for s in nr.RS_SHAPES for d in (True, False) for k in ('int', 'pro')]


def _id(v):
    return '-'.join(str(e) for e in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize('shape,fam', GN_FAMILY_CASES, ids=_id)
def test_groupnorm_statistics_and_apply(be, report, shape, fam):
    rp, ry = check_groupnorm(be, shape, fam)
    report(f'norm_a_partial_{_id(shape)}_{fam}', rp)
    report(f'norm_a_apply_{_id(shape)}_{fam}', ry)


@pytest.mark.parametrize('fam', ['benign', 'offset'])
@pytest.mark.parametrize('shape,variant', GN_VARIANT_CASES, ids=_id)
def test_groupnorm_variants(be, report, shape, variant, fam):
    rp, ry = check_groupnorm(be, shape, fam, variant)
    report(f'norm_a_partial_{_id(shape)}_{fam}_{variant}', rp)
    report(f'norm_a_apply_{_id(shape)}_{fam}_{variant}', ry)


@pytest.mark.parametrize('flavour', nr.FIN_FLAVOURS)
@pytest.mark.parametrize('HW,C,G,mode', FIN_CASES, ids=_id)
def test_finalize_forms(be, report, HW, C, G, mode, flavour):
    report(f'norm_b_finalize_{HW}_{C}_{G}_{mode}_{flavour}', check_finalize(be, HW, C, G, mode, flavour))


def test_finalize_rechunked(be, report):
    report('norm_b_rechunk_64_vs_65', check_finalize_rechunk(be))


@pytest.mark.parametrize('shape', AFFINE_SHAPES, ids=_id)
def test_groupnorm_affine_equals_finalize_hook(be, report, shape):
    report(f'norm_b_affine_{_id(shape)}', check_affine_equals_hook(be, shape))


@pytest.mark.parametrize('HW', nr.CONCAT_HW)
@pytest.mark.parametrize('case', nr.CONCAT_CASES, ids=_id)
def test_concat_stats(be, report, case, HW):
    report(f'norm_c_concat_{_id(case)}_{HW}', check_concat(be, case, HW))


@pytest.mark.parametrize('case', nr.CONCAT_REFUSED, ids=_id)
def test_concat_stats_refusals(be, case):
    check_concat_refused(be, case)


@pytest.mark.parametrize('s,G', [(s, G) for s in nr.CONV_GN_CASES for G in s['G']],
                         ids=lambda v: v['name'] if isinstance(v, dict) else str(v))
def test_conv_emitted_statistics(be, report, s, G):
    report(f'norm_d_emit_{s["name"]}_G{G}', check_conv_gn(be, s, G))


@pytest.mark.parametrize('s', nr.CONV_GN_REFUSED, ids=lambda v: v['name'])
def test_conv_emitted_statistics_refusals(be, s):
    check_conv_gn_refused(be, s, s['G'][0])


@pytest.mark.parametrize('s', nr.GEMM_GN_CASES, ids=lambda v: v['name'])
def test_gemm_emitted_statistics(be, report, s):
    report(f'norm_d_emit_gemm_{s["name"]}_G{s["G"]}', check_gemm_gn(be, s))


@pytest.mark.parametrize('s', nr.GEMM_GN_REFUSED, ids=lambda v: v['name'])
def test_gemm_emitted_statistics_refusals(be, s):
    check_gemm_gn_refused(be, s)


@pytest.mark.parametrize('nosilu', [0, 1], ids=['silu', 'nosilu'])
@pytest.mark.parametrize('mod', [0, 1], ids=['plain', 'adagn'])
@pytest.mark.parametrize('s', nr.CONV_GIN_CASES, ids=lambda v: v['name'])
def test_conv_in_kernel_finalize(be, s, mod, nosilu):
    check_conv_gin(be, s, mod, nosilu)


@pytest.mark.parametrize('s', nr.CONV_GIN_REFUSED, ids=lambda v: v['name'])
def test_conv_in_kernel_finalize_refusals(be, s):
    check_conv_gin_refused(be, s)


@pytest.mark.parametrize('G', [0] + nr.SI_G)
@pytest.mark.parametrize('case', nr.small_in_cases(), ids=_id)
def test_first_conv(be, report, case, G):
    report(f'norm_f_small_in_{_id(case)}_G{G}', check_small_in(be, case, G))


@pytest.mark.parametrize('case', SO_CASES, ids=_id)
def test_last_conv_exact(be, case):
    check_small_out_int(be, case)


@pytest.mark.parametrize('case', SO_CASES[::2], ids=_id)
def test_last_conv_groupnorm_prologue(be, report, case):
    report(f'norm_g_small_out_{_id(case)}', check_small_out_gn(be, case))


def test_last_conv_refuses_wide_in_kernel_finalize(be):
    check_small_out_refused(be)


@pytest.mark.parametrize('shape,down,kind', RS_CASES, ids=_id)
def test_resample2x(be, report, shape, down, kind):
    report(f'norm_h_resample_{_id(shape)}_{"down" if down else "up"}_{kind}', check_resample(be, shape, down, kind))


def test_resample2x_refuses_odd_down(be):
    check_resample_refused(be)
