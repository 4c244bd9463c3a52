"""Host-side inputs, float64 references, derived bounds and an fp32 / fp64 emulation for the GroupNorm chain
(csrc/gn.hip: gn_partial, gn_apply, gn_finalize and its wide form, gn_concat_stats) and the first / last convs and
resample2x (csrc/elementwise.hip).

Plain torch on the CPU, shared by tests/test_norm_host.py (no GPU) and tests/test_gpu_norm_ops.py.

Data (family): six seeded families, fp32 tensors [B, HW, C]; image b is scaled by 4^b and shifted by 10 b, so a
statistic or table taken from the wrong image is off by far more than any bound. Pitched views (pitched) carry NaN in
every pad column; output, partial and table buffers are NaN-prefilled with a tail that must survive (the backends
allocate them; checked_* below verify them).

Bounds (derived, not measured; u = 2^-24, the fp32 unit roundoff):

* A partial slot {sum v, sum v^2} over n stored fp32 values (partial_ref): reference = the float64 sum of the stored
  values; bound = n 2^-52 sum|term|. (double)v and (double)v * v are exact, so every error is fp64 summation error,
  at most (n - 1) 2^-53 sum|term| in any order: the bound is twice that.
* The finalize tables (finalize_ref): from the SAME partials, the group mean and variance evaluated exactly (rational
  arithmetic on the fp64 partials, the variance clamped at 0 as the kernels document), then in float64
  sc64 = rstd64 gamma, sh64 = -sc64 mu64 + beta. |sc - sc64| <= 2^-22 |sc64| (two roundings: float(rstd), the
  product; four allowed). sh = fl(fl(-sc mu) + beta) carries FIVE roundings on its product term (float(rstd), the
  gamma product, float(mean), the product, the sum) and one on beta, so its worst case is 5 u |sc mu| + u |beta|:
  the flat 2^-22 (|sc64 mu64| + |beta|) = 4 u (...) first proposed for it counted three and lies BELOW that worst
  case when beta is small (the emulation reached 0.52 of it). The bound is one rounding above the count on each term:
  |sh - sh64| <= u (6 |sc64 mu64| + 2 |beta|)  -- wider on the product term, tighter on beta.
  (The library is built without contraction, so all five roundings occur and 5 u |sc mu| is attainable: a bound
  equal to the worst case would leave nothing for the first-order analysis' dropped u^2 terms, and the other bounds
  here allow one rounding beyond their count (four for three). With contraction the count is four and 6 u is slack.)
  With modulation f = 1 + ms: sc' = sc f, sh' = sh f + mb; f, the products and the sum add at most three roundings
  of the value they produce to the propagated error, so  |sc' - sc'64| <= 2 * 2^-22 |sc64 f64|  and
  |sh' - sh'64| <= u (6 |sc64 mu64| + 2 |beta|) |f64| + 2^-22 (|sh64 f64| + |mb|).
* gn_apply's output (apply_ref): |y - ref64| <= 2^-21 (|x sc64| + |sc64 mu64| + |beta|) per element; with
  modulation the bound is carried through (times |f64|) and 2^-22 |value| is added per extra operation, the value
  being that operation's float64 result (two operations for the scale: f and the product; one for the shift);
  behind SiLU tests/token_ref.py's activation widening (times 1.13, + 4 ulp of the output).
* The last conv behind a GroupNorm + SiLU prologue (small_out_ref): the prologue's bound (activation form) carried
  through sum |w| ., plus the fp32 chain's (9 Cin + 1) u (sum |w a| + |bias|).

EmuBackend evaluates every operation with the kernels' expressions in fp32 / fp64 torch (fma=True: the multiply-add
pairs contracted) behind the interface of the device backend; its mutants are the subtly wrong kernels the checks must
notice (tests/test_norm_host.py).
"""
import functools
import math
import zlib
from fractions import Fraction

import torch
import torch.nn.functional as Fn

F32, F64 = torch.float32, torch.float64
CHUNK = 64                    # kGnPixPerChunk
WIDE = 64                     # kGnWideChunks: more chunks per image run gn_finalize_wide_kernel
EPS = float(torch.tensor(1e-5, dtype=F32))
NAN = float('nan')
TAIL = 64                     # sentinel slots / rows past every output buffer
ERR = -1                      # DM_ERR_ARG: what a refusing DM_REQUIRE returns
UNSUPPORTED = -4              # DM_ERR_UNSUPPORTED


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def nchunks(HW):
    return (HW + CHUNK - 1) // CHUNK


# ------------------------------------------------------------------------------------------------------ data
FAMILIES = ('benign', 'offset', 'neg', 'const', 'outlier', 'tiny')


def family(name, B, HW, C, G, g):
    """fp32 [B, HW, C] of one family, image b times 4^b plus 10 b."""
    z = torch.randn((B, HW, C), generator=g)
    if name == 'benign':
        x = 3.0 * z + 0.5
    elif name == 'offset':
        x = 1024.0 + z                      # mean / sigma = 2^10
    elif name == 'neg':
        x = -1e4 + 0.5 * z
    elif name == 'const':
        x = torch.full((B, HW, C), 0.1)     # E[x^2] - E[x]^2 cancels completely
    elif name == 'outlier':
        x = z.clone()
        cpg = C // G
        v = x.view(B, HW, G, cpg)
        for b in range(B):
            for gi in range(G):
                v[b, int(torch.randint(0, HW, (1, ), generator=g)), gi, int(torch.randint(0, cpg, (1, ), generator=g))] = 3e4
    elif name == 'tiny':
        x = 1e-4 * z
    else:
        raise ValueError(name)
    img = torch.arange(B, dtype=F32)[:, None, None]
    return (x * torch.pow(torch.tensor(4.0), img) + 10.0 * img).to(F32).contiguous()


def pitched(x, pitch, off):
    """x [B, HW, C] inside a NaN-filled [B, HW, pitch] buffer at column off -> the buffer."""
    B, HW, C = x.shape
    assert off + C <= pitch
    buf = torch.full((B, HW, pitch), NAN)
    buf[:, :, off:off + C] = x
    return buf


def affine(C, g):
    """gamma ~ U(0.5, 1.5) (a few negative), beta ~ N(0, 1)."""
    gamma = 0.5 + torch.rand((C, ), generator=g)
    gamma[::7] = -gamma[::7]
    return gamma, torch.randn((C, ), generator=g)


def mod_tables(B, C, g, scale=True, shift=True):
    """Modulation tables inside a wider NaN-filled [B, pitch] buffer (pitch > C, column offsets multiples of 4);
    the images' tables differ by O(1). -> (buf, scale offset | None, shift offset | None)."""
    pitch = 2 * C + 16
    buf = torch.full((B, pitch), NAN)
    img = torch.arange(B, dtype=F32)[:, None]
    so = bo = None
    if scale:
        so = 4
        buf[:, so:so + C] = -0.5 + 2.0 * torch.rand((B, C), generator=g) + 0.25 * img
    if shift:
        bo = C + 12
        buf[:, bo:bo + C] = -2.0 + 4.0 * torch.rand((B, C), generator=g) + img
    return buf, so, bo


def ints(shape, g, lo=-3, hi=4):
    return torch.randint(lo, hi, shape, generator=g).float()


# ------------------------------------------------------------------------------------------------ references
def ratio(err, bound):
    """max err / bound; a zero bound admits a zero error only."""
    err, bound = torch.as_tensor(err, dtype=F64), torch.as_tensor(bound, dtype=F64)
    if torch.isnan(err).any():
        return math.inf
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf))
    return float(r.max()) if r.numel() else 0.0


def partial_ref(y, G):
    """Stored values y [B, HW, C] (fp32) -> (ref, bound) float64 [B, nchunk, G, 2]: the float64 sums per (image,
    64-pixel chunk, group) and n 2^-52 sum|term|."""
    B, HW, C = y.shape
    nch, cpg = nchunks(HW), C // G
    v = torch.zeros((B, nch * CHUNK, C), dtype=F64)
    v[:, :HW] = y.to(F64)
    v = v.view(B, nch, CHUNK, G, cpg)
    s, q, sa = v.sum(dim=(2, 4)), (v * v).sum(dim=(2, 4)), v.abs().sum(dim=(2, 4))
    n = torch.tensor([min(CHUNK, HW - k * CHUNK) * cpg for k in range(nch)], dtype=F64)[None, :, None]
    return torch.stack([s, q], dim=-1), torch.stack([n * 2.0 ** -52 * sa, n * 2.0 ** -52 * q], dim=-1)


def _exact_sum(vals):
    """The exact sum of finite doubles as a Fraction (every value is an integer multiple of 2^E)."""
    nz = [v for v in vals if v != 0.0]
    if not nz:
        return Fraction(0)
    E = min(math.frexp(v)[1] for v in nz) - 53
    return Fraction(sum(int(math.ldexp(v, -E)) for v in nz)) * Fraction(2) ** E


def group_moments(part, n):
    """part float64 [B, nchunk, G, 2] -> (mean64, var64) [B, G]: exact rational evaluation of a / n and
    q / n - (a / n)^2 from the fp64 partials, the variance clamped at 0, rounded once to float64."""
    B, nch, G, _ = part.shape
    mean, var = torch.zeros((B, G), dtype=F64), torch.zeros((B, G), dtype=F64)
    p = part.permute(0, 2, 3, 1).tolist()   # [B][G][2][nchunk]
    for b in range(B):
        for gi in range(G):
            a, q = _exact_sum(p[b][gi][0]), _exact_sum(p[b][gi][1])
            m = a / n
            mean[b, gi] = float(m)
            var[b, gi] = max(float(q / n - m * m), 0.0)
    return mean, var


def finalize_ref(part, HW, C, eps, gamma=None, beta=None, ms=None, mb=None):
    """-> dict(sc, sh, sc_bound, sh_bound, mu, base_sc, base_sh, f) float64 [B, C] (module docstring)."""
    B, _, G, _ = part.shape
    cpg = C // G
    mean, var = group_moments(part, HW * cpg)
    rstd = 1.0 / torch.sqrt(var + eps)
    mu = mean.repeat_interleave(cpg, dim=1)
    ga = torch.ones((C, ), dtype=F64) if gamma is None else gamma.to(F64)
    be = torch.zeros((C, ), dtype=F64) if beta is None else beta.to(F64)
    sc = rstd.repeat_interleave(cpg, dim=1) * ga
    sh = -sc * mu + be
    scb = 2.0 ** -22 * sc.abs()
    shb = 2.0 ** -24 * (6.0 * (sc * mu).abs() + 2.0 * be.abs())
    out = dict(mu=mu, base_sc=sc, base_sh=sh, beta=be.expand(B, C), f=None)
    if ms is not None:
        f = 1.0 + ms.to(F64)
        m = torch.zeros((B, C), dtype=F64) if mb is None else mb.to(F64)
        sc2, sh2 = sc * f, sh * f + m
        scb = 2.0 * 2.0 ** -22 * sc2.abs()
        shb = shb * f.abs() + 2.0 ** -22 * ((sh * f).abs() + m.abs())
        sc, sh = sc2, sh2
        out['f'] = f
    out.update(sc=sc, sh=sh, sc_bound=scb, sh_bound=shb)
    return out


def silu_widen(bound, ref_act):
    """tests/token_ref.py's activation widening: times 1.13, + 4 ulp of the output."""
    return 1.13 * bound + 4.0 * 2.0 ** -23 * ref_act.abs()


def apply_ref(x, part, G, eps, gamma=None, beta=None, ms=None, mb=None, silu=False):
    """gn_apply's float64 reference and elementwise bound from the partials: ((x sc64 + sh64) (1 + ms) + mb, SiLU)."""
    B, HW, C = x.shape
    fr = finalize_ref(part, HW, C, eps, gamma, beta)
    sc, sh, mu, be = fr['sc'][:, None, :], fr['sh'][:, None, :], fr['mu'][:, None, :], fr['beta'][:, None, :]
    x64 = x.to(F64)
    y = x64 * sc + sh
    bound = 2.0 ** -21 * ((x64 * sc).abs() + (sc * mu).abs() + be.abs())
    if ms is not None:
        f = (1.0 + ms.to(F64))[:, None, :]
        y = y * f
        bound = bound * f.abs() + 2.0 * 2.0 ** -22 * y.abs()
    if mb is not None:
        y = y + mb.to(F64)[:, None, :]
        bound = bound + 2.0 ** -22 * y.abs()
    if silu:
        y = Fn.silu(y)
        bound = silu_widen(bound, y)
    return y, bound


def concat_ordered(ph, ps, Ch, Cs, G, edge=None):
    """gn_concat_stats restated in float64 in the order its comment documents: concat group j sums h's slice
    groups inside its channel range, then skip's, in channel order. ph [B, nchunk, Gh, 2], ps [B, nchunk, Gs, 2].
    edge (EmuBackend's mutant only): where the loops believe the slice boundary to be."""
    B, nch, Gh, _ = ph.shape
    Gs = ps.shape[2]
    cpg, cph, cps = (Ch + Cs) // G, Ch // Gh, Cs // Gs
    h, s = ph.tolist(), ps.tolist()
    out = torch.zeros((B, nch, G, 2), dtype=F64)
    edge = Ch if edge is None else edge
    for b in range(B):
        for k in range(nch):
            for j in range(G):
                lo, hi = j * cpg, (j + 1) * cpg
                s1 = s2 = 0.0
                for c in range(lo, min(hi, edge), cph):
                    s1 += h[b][k][c // cph][0]
                    s2 += h[b][k][c // cph][1]
                for c in range(max(lo, edge), hi, cps):
                    s1 += s[b][k][max((c - Ch) // cps, 0)][0]
                    s2 += s[b][k][max((c - Ch) // cps, 0)][1]
                out[b, k, j, 0], out[b, k, j, 1] = s1, s2
    return out


def concat_ok(Ch, Gh, Cs, Gs, G):
    """gn_concat_ok restated: every count positive and dividing its channels, no slice group straddling a concat
    group's edge."""
    C = Ch + Cs
    if G <= 0 or Gh <= 0 or Gs <= 0 or C % G or Ch % Gh or Cs % Gs:
        return False
    cpg, cph, cps = C // G, Ch // Gh, Cs // Gs
    edges = {j * cpg for j in range(G + 1)}
    return all(e % cph == 0 for e in edges if e < Ch) and all((e - Ch) % cps == 0 for e in edges if e > Ch)


# the first conv's geometry (csrc/elementwise.hip small_in_rows, conv3x3_small_in_can_emit, the launcher's LDS check)
def small_in_rows(H, W):
    if not (W < CHUNK and CHUNK % W == 0 and H % (CHUNK // W) == 0):
        return 1
    R = CHUNK // W
    if H % (2 * R) == 0 and (2 * R * W) // CHUNK <= 8:
        R *= 2
    return R


def small_in_can_emit(H, W, Cout, G):
    R = small_in_rows(H, W)
    lpp = min(Cout // 2, 256)
    if G <= 0 or G > 32 or Cout % G:
        return False
    cpg = Cout // G
    return (cpg % 2 == 0 and cpg <= 64 and cpg & (cpg - 1) == 0 and lpp >= 64 and 256 % lpp == 0 and (Cout // 2) % lpp == 0
            and (R * W) % CHUNK == 0 and (R * W) // CHUNK <= 8 and 256 // lpp <= 4)


def small_in_fits(Cin, H, W, Cout, stats):
    R = small_in_rows(H, W)
    nf = Cin * 3 * (W + 2) + Cin * (R - 1) * (W + 2) + Cout * Cin * 9
    return ((nf + 3) & ~3) * 4 + (4 * 8 * 32 * 16 if stats else 0) <= 64 * 1024


def conv3x3_f64(x, w, bias):
    """NCHW float64 3x3 conv, padding 1 -> NHWC [B, H, W, Cout]."""
    return Fn.conv2d(x.to(F64), w.to(F64), bias.to(F64), padding=1).permute(0, 2, 3, 1).contiguous()


def small_out_ref(x, w, bias, sc64=None, sh64=None, pro_bound=None):
    """Last conv: x [B, H, W, Cin] NHWC, w [Cout, Cin, 3, 3] -> (ref64 NCHW [B, Cout, H, W], bound | None); the
    prologue a = silu(x sc64 + sh64) with its elementwise bound pro_bound (before the activation) when given."""
    a = x.to(F64)
    if sc64 is None:
        return Fn.conv2d(a.permute(0, 3, 1, 2), w.to(F64), bias.to(F64), padding=1), None
    pre = a * sc64[:, None, None, :] + sh64[:, None, None, :]
    act = Fn.silu(pre)
    ab = silu_widen(pro_bound, act)
    w64 = w.to(F64)
    ref = Fn.conv2d(act.permute(0, 3, 1, 2), w64, bias.to(F64), padding=1)
    mag = Fn.conv2d(act.abs().permute(0, 3, 1, 2), w64.abs(), bias.to(F64).abs(), padding=1)
    n = 9 * x.shape[3] + 1
    return ref, Fn.conv2d(ab.permute(0, 3, 1, 2), w64.abs(), None, padding=1) + n * 2.0 ** -24 * mag


def resample_ref(x, down, sc=None, sh=None):
    """x [B, H, W, C] NHWC -> (float64 avg_pool2d / nearest-2x of the optional silu(x sc + sh), bound | None)."""
    a = x.to(F64)
    bound = None
    if sc is not None:
        s, h = sc.to(F64)[:, None, None, :], sh.to(F64)[:, None, None, :]
        pre = a * s + h
        # the tables are the kernel's inputs: x s + h is two fp32 roundings, 2^-23 (|x s| + |h|) allows four
        bound = 2.0 ** -23 * ((a * s).abs() + h.abs())
        a = Fn.silu(pre)
        bound = silu_widen(bound, a)
    t = a.permute(0, 3, 1, 2)
    if down:
        y = Fn.avg_pool2d(t, 2)
        if bound is not None:   # the mean of four carries their bounds' mean, + three adds and the division
            bound = Fn.avg_pool2d(bound.permute(0, 3, 1, 2), 2) + 4.0 * 2.0 ** -24 * Fn.avg_pool2d(t.abs(), 2)
            bound = bound.permute(0, 2, 3, 1)
    else:
        y = Fn.interpolate(t, scale_factor=2, mode='nearest')
        if bound is not None:
            bound = Fn.interpolate(bound.permute(0, 3, 1, 2), scale_factor=2, mode='nearest').permute(0, 2, 3, 1)
    return y.permute(0, 2, 3, 1).contiguous(), bound


# ------------------------------------------------------------------------------------------------- emulation
def _silu32(v):
    return v / (1.0 + torch.exp(-v))


MUTANTS = ('image_index', 'drop_last_chunk', 'slot_late', 'fp32_sums', 'no_clamp', 'mod_pitch', 'pad_in_stats',
           'concat_boundary')


class EmuBackend:
    """The device backend's interface on the CPU: each operation in the kernels' own expressions (fp64 sums, fp32
    tables and outputs), with the same NaN-prefilled outputs and tails. mutant: one of MUTANTS (a subtly wrong
    kernel); fma: the fp32 multiply-add pairs contracted."""

    def __init__(self, mutant=None, fma=False):
        assert mutant is None or mutant in MUTANTS
        self.mutant, self.fma = mutant, fma
        self.name = 'emulation' + (f'[{mutant}]' if mutant else '') + ('[fma]' if fma else '')

    def _madd(self, a, b, c):
        """a b + c in fp32: separately rounded, or one rounding (fma; exact product in float64, then the sum --
        float64's 53 bits make the double rounding immaterial here)."""
        if self.fma:
            return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)
        return a * b + c

    # ---- statistics
    def gn_partial(self, xbuf, off, C, G):
        """xbuf [B, HW, pitch], the view at column off -> flat float64 [B nchunk G + TAIL, 2]."""
        B, HW, _ = xbuf.shape
        if self.mutant == 'pad_in_stats' and off > 0:
            off -= 1
        x = xbuf[:, :, off:off + C]
        nch, cpg = nchunks(HW), C // G
        acc = F32 if self.mutant == 'fp32_sums' else F64
        v = torch.zeros((B, nch * CHUNK, C), dtype=acc)
        v[:, :HW] = x.to(acc)
        v = v.view(B, nch, CHUNK, G, cpg)
        # (double)v * v is exact; the fp32 mutant rounds the squares and both sums
        p = torch.stack([v.sum(dim=(2, 4)), (v * v).sum(dim=(2, 4))], dim=-1).to(F64)
        out = torch.full((B * nch * G + TAIL, 2), NAN, dtype=F64)
        flat = p.reshape(-1, 2)
        if self.mutant == 'slot_late':
            out[G:G + flat.shape[0]] = flat   # every (chunk, group) slot one chunk late (G <= TAIL)
        else:
            out[:flat.shape[0]] = flat
        return out

    def _tables(self, part, HW, C, eps, gamma, beta, modbuf=None, so=None, bo=None):
        """gn_finalize's expressions: part float64 [B, nchunk, G, 2] -> (sc, sh) fp32 [B, C]."""
        B, nch, G, _ = part.shape
        cpg = C // G
        if self.mutant == 'drop_last_chunk' and nch > 1:
            part = part[:, :-1]
        tot = torch.zeros((B, G, 2), dtype=F64)
        for k in range(part.shape[1]):
            tot = tot + part[:, k]
        n = float(HW * cpg)
        m = tot[..., 0] / n
        var = tot[..., 1] / n - m * m
        if self.mutant != 'no_clamp':
            var = var.clamp_min(0.0)
        mu = m.to(F32)
        rs = (1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=F32)))).to(F32)
        if self.mutant == 'image_index' and B > 1:
            mu, rs = mu.roll(1, 0), rs.roll(1, 0)
        mu, rs = mu.repeat_interleave(cpg, dim=1), rs.repeat_interleave(cpg, dim=1)
        ga = torch.ones((C, )) if gamma is None else gamma
        be = torch.zeros((C, )) if beta is None else beta
        sc = rs * ga
        sh = self._madd(-sc, mu, be.expand(B, C))
        if so is not None:
            ms, mb = self._mod(modbuf, so, C), (None if bo is None else self._mod(modbuf, bo, C))
            f = 1.0 + ms
            sc = sc * f
            sh = self._madd(sh, f, torch.zeros((B, C)) if mb is None else mb)
        return sc, sh

    def _mod(self, buf, off, C):
        """Rows b of a [B, pitch] table buffer at column off; the mutant strides by C instead of the pitch."""
        if self.mutant != 'mod_pitch':
            return buf[:, off:off + C]
        flat = torch.cat([buf.reshape(-1), torch.full((C, ), NAN)])
        return torch.stack([flat[off + b * C:off + b * C + C] for b in range(buf.shape[0])])

    def gn_finalize(self, part, B, HW, C, G, eps, gamma=None, beta=None, modbuf=None, so=None, bo=None):
        """part flat float64 [>= B nchunk G, 2] -> dict(sc, sh fp32 [B + 1, C] with a NaN tail row, rc)."""
        nch = nchunks(HW)
        p = part[:B * nch * G].view(B, nch, G, 2)
        out = dict(sc=torch.full((B + 1, C), NAN), sh=torch.full((B + 1, C), NAN), rc=0)
        if C % G:
            out['rc'] = ERR
            return out
        out['sc'][:B], out['sh'][:B] = self._tables(p, HW, C, eps, gamma, beta, modbuf, so, bo)
        return out

    def groupnorm(self, xbuf, off, C, G, eps, gamma=None, beta=None, modbuf=None, so=None, bo=None, silu=False,
                  y_pitch=None):
        """dm_groupnorm_nhwc: -> dict(part flat, y [B HW + TAIL, y_pitch] fp32 (NaN prefill), rc)."""
        B, HW, _ = xbuf.shape
        y_pitch = y_pitch or C
        part = self.gn_partial(xbuf, off, C, G)
        nch = nchunks(HW)
        # gn_apply's own finalize (no modulation folded into the tables: it is applied to the normalized value)
        sc, sh = self._tables(part[:B * nch * G].view(B, nch, G, 2), HW, C, eps, gamma, beta)
        x = xbuf[:, :, off:off + C]
        o = self._madd(x, sc[:, None, :].expand_as(x), sh[:, None, :].expand_as(x))
        if so is not None:
            o = o * (1.0 + self._mod(modbuf, so, C))[:, None, :]
        if bo is not None:
            o = o + self._mod(modbuf, bo, C)[:, None, :]
        if silu:
            o = _silu32(o)
        y = torch.full((B * HW + TAIL, y_pitch), NAN)
        y[:B * HW, :C] = o.reshape(B * HW, C)
        return dict(part=part, y=y, rc=0)

    def gn_affine(self, xbuf, off, C, G, eps, gamma=None, beta=None):
        """dm_groupnorm_affine: -> dict(part, sc, sh, rc) as gn_partial + gn_finalize."""
        B, HW, _ = xbuf.shape
        part = self.gn_partial(xbuf, off, C, G)
        out = self.gn_finalize(part, B, HW, C, G, eps, gamma, beta)
        out['part'] = part
        return out

    def gn_concat(self, ph, Ch, Gh, ps, Cs, Gs, B, HW, G):
        """ph / ps flat float64 partials -> dict(out flat [B nchunk max(G, 1) + TAIL, 2], rc)."""
        nch = nchunks(HW)
        out = torch.full((B * nch * max(G, 1) + TAIL, 2), NAN, dtype=F64)
        if not concat_ok(Ch, Gh, Cs, Gs, G):
            return dict(out=out, rc=ERR)
        h, s = ph[:B * nch * Gh].view(B, nch, Gh, 2), ps[:B * nch * Gs].view(B, nch, Gs, 2)
        edge = None
        if self.mutant == 'concat_boundary':   # the slice boundary taken at a concat group's edge (no straddling group)
            edge = Ch // ((Ch + Cs) // G) * ((Ch + Cs) // G)
        out[:B * nch * G] = concat_ordered(h, s, Ch, Cs, G, edge).view(-1, 2)
        return dict(out=out, rc=0)

    def conv_gn(self, s, G):
        """d. A conv with bias, per-image rowvec, residual and a pitched output, run without and with the epilogue's
        GroupNorm(G) statistics -> dict(y0, y1 [rows + TAIL, y_pitch], part flat, log, rc)."""
        c = conv_case(s)
        B, Cout, Ho, Wo = s['B'], s['Cout'], c['Ho'], c['Wo']
        rows, nch = B * Ho * Wo, nchunks(Ho * Wo)
        y0 = torch.full((rows + TAIL, c['y_pitch']), NAN)
        y1, part = y0.clone(), torch.full((B * nch * G + TAIL, 2), NAN, dtype=F64)
        a = c['x']
        if s.get('up'):
            a = Fn.interpolate(a, scale_factor=2, mode='nearest')
        if s.get('s2_pad0'):
            y = Fn.conv2d(Fn.pad(a, (0, 1, 0, 1)), c['w'], c['bias'], stride=2)
        else:
            y = Fn.conv2d(a, c['w'], c['bias'], stride=s.get('stride', 1), padding=c['w'].shape[-1] // 2)
        y = (y + c['rowvec'][:, :, None, None]).permute(0, 2, 3, 1) + c['res']
        y0[:rows, :Cout] = y.reshape(rows, Cout)
        if s.get('refuse') or Cout % G:
            return dict(y0=y0, y1=y1, part=part, log=[], rc=ERR)
        y1[:rows, :Cout] = y0[:rows, :Cout]
        part[:] = self.gn_partial(y.reshape(B, Ho * Wo, Cout), 0, Cout, G)
        return dict(y0=y0, y1=y1, part=part, log=[s['kernel']], rc=0)

    def gemm_gn(self, s, G):
        """d. C = A W^T + bias + res with and without the epilogue's GroupNorm(G) statistics over images of hw rows
        -> dict(y0, y1 [M + TAIL, ldc], part flat, rc)."""
        c = gemm_case(s)
        M, N, hw = c['A'].shape[0], c['W'].shape[0], s['hw']
        B = M // hw
        y0 = torch.full((M + TAIL, c['ldc']), NAN)
        y1, part = y0.clone(), torch.full((B * nchunks(hw) * G + TAIL, 2), NAN, dtype=F64)
        y = c['A'] @ c['W'].T + c['bias'] + c['res']
        y0[:M, :N] = y
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        if not (M >= 128 and N >= 128 and tiles >= 512) or hw % 64 or N % G or 32 % (N // G):
            return dict(y0=y0, y1=y1, part=part, rc=ERR)
        y1[:M, :N] = y
        part[:] = self.gn_partial(y.view(B, hw, N), 0, N, G)
        return dict(y0=y0, y1=y1, part=part, rc=0)

    def conv_gin(self, s, mod, nosilu):
        """e. A conv behind a GroupNorm (+ AdaGN modulation) (+ SiLU) prologue, the tables from gn_finalize (y_tab) and
        finalized in the kernel from the same partials (y_gin) -> dict(y_tab, y_gin [rows + TAIL, y_pitch], log, rc)."""
        c = gin_case(s, mod)
        B, Cin, Cout, H, W = s['B'], s['Cin'], s['Cout'], s['H'], s['W']
        rows = B * H * W
        y_tab = torch.full((rows + TAIL, c['y_pitch']), NAN)
        y_gin = y_tab.clone()
        p = c['part'][:B * nchunks(H * W) * c['G']].view(B, -1, c['G'], 2)
        sc, sh = self._tables(p, H * W, Cin, c['eps'], c['gamma'], c['beta'], c['modbuf'], c['so'], c['bo'])
        x = c['x'].permute(0, 2, 3, 1)
        a = self._madd(x, sc[:, None, None, :].expand_as(x), sh[:, None, None, :].expand_as(x))
        if not nosilu:
            a = _silu32(a)
        y = Fn.conv2d(a.permute(0, 3, 1, 2), c['w'], c['bias'], padding=c['w'].shape[-1] // 2)
        y = (y + c['rowvec'][:, :, None, None]).permute(0, 2, 3, 1) + c['res']
        y_tab[:rows, :Cout] = y.reshape(rows, Cout)
        if s.get('refuse'):
            return dict(y_tab=y_tab, y_gin=y_gin, log=[], rc=UNSUPPORTED)
        y_gin[:rows, :Cout] = y_tab[:rows, :Cout]
        return dict(y_tab=y_tab, y_gin=y_gin, log=[s['kernel']], rc=0)

    # ---- first / last conv, resample
    def small_in(self, x, w, bias, y_pitch, G=0):
        """x NCHW [B, Cin, H, W] -> dict(y [B H W + TAIL, y_pitch], part flat | None, rc)."""
        B, Cin, H, W = x.shape
        Cout = w.shape[0]
        y = torch.full((B * H * W + TAIL, y_pitch), NAN)
        part = None if G == 0 else torch.full((B * nchunks(H * W) * G + TAIL, 2), NAN, dtype=F64)
        ok = 1 <= Cin <= 4 and Cout % 2 == 0 and y_pitch % 2 == 0 and small_in_fits(Cin, H, W, Cout, G > 0)
        if not ok or (G and not small_in_can_emit(H, W, Cout, G)):
            return dict(y=y, part=part, rc=ERR)
        # acc from 0, acc + w x over (ci, ky, kx), products separately rounded, then + bias
        xp = Fn.pad(x, (1, 1, 1, 1))
        acc = torch.zeros((B, H, W, Cout))
        for ci in range(Cin):
            for ky in range(3):
                for kx in range(3):
                    acc = acc + xp[:, ci, ky:ky + H, kx:kx + W, None] * w[:, ci, ky, kx]
        v = (acc + bias).reshape(B, H * W, Cout)
        y[:B * H * W, :Cout] = v.reshape(B * H * W, Cout)
        if G:
            part[:] = self.gn_partial(v, 0, Cout, G)
        return dict(y=y, part=part, rc=0)

    def small_out(self, xbuf, Cin, w, bias, pro=None, fin=None):
        """xbuf [B, H, W, pitch] (the view's channels first) -> dict(y NCHW [B + 1, Cout, H, W], wp_tail_ok, rc).
        pro: (sc, sh) fp32 [B, Cin]; fin: dict(part flat, G, nchunk, eps, gamma, beta)."""
        B, H, W, pitch = xbuf.shape
        Cout = w.shape[0]
        y = torch.full((B + 1, Cout, H, W), NAN)
        if not (1 <= Cout <= 8 and Cin % 32 == 0 and pitch % 4 == 0) or \
                (fin is not None and (pro is not None or fin['G'] <= 0 or Cin % fin['G'] or Cin > 512 or fin['nchunk'] <= 0)):
            return dict(y=y, wp_tail_ok=True, rc=ERR)
        a = xbuf[..., :Cin]
        if fin is not None:
            p = fin['part'][:B * fin['nchunk'] * fin['G']].view(B, fin['nchunk'], fin['G'], 2)
            pro = self._tables(p, H * W, Cin, fin['eps'], fin['gamma'], fin['beta'])
        if pro is not None:
            a = _silu32(self._madd(a, pro[0][:, None, None, :].expand_as(a), pro[1][:, None, None, :].expand_as(a)))
        # (the device's fused chain over (16-channel chunk, tap, channel) is not restated: fp32 conv + bias)
        y[:B] = Fn.conv2d(a.permute(0, 3, 1, 2), w, None, padding=1) + bias[None, :, None, None]
        return dict(y=y, wp_tail_ok=True, rc=0)

    def resample(self, xbuf, C, y_pitch, down, pro=None):
        """xbuf [B, H, W, x_pitch] -> dict(y [B Ho Wo + TAIL, y_pitch], Ho, Wo, rc)."""
        B, H, W, xp = xbuf.shape
        Ho, Wo = (H // 2, W // 2) if down else (2 * H, 2 * W)
        y = torch.full((B * Ho * Wo + TAIL, y_pitch), NAN)
        if C % 4 or xp % 4 or y_pitch % 4 or (down and (H % 2 or W % 2)):
            return dict(y=y, Ho=Ho, Wo=Wo, rc=ERR)
        a = xbuf[..., :C]
        if pro is not None:
            a = _silu32(self._madd(a, pro[0][:, None, None, :].expand_as(a), pro[1][:, None, None, :].expand_as(a)))
        if down:   # torch avg_pool2d: the row-major window sum, then / 4
            o = (((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + a[:, 1::2, 0::2]) + a[:, 1::2, 1::2]) / 4.0
        else:
            o = a.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        y[:B * Ho * Wo, :C] = o.reshape(B * Ho * Wo, C)
        return dict(y=y, Ho=Ho, Wo=Wo, rc=0)


# ------------------------------------------------------------------------------------------------------ cases
# a. (B, C, HW, G)
GN_SHAPES = [
    (3, 64, 64, 32),
    (3, 32, 100, 32),      # one channel per group, last chunk 36 pixels
    (2, 192, 36, 32),      # C / 4 = 48 does not divide 256
    (1, 1280, 16, 32),     # 320-thread blocks
    (1, 4096, 4, 32),      # the LDS limit
    (2, 8, 200, 2),        # PY = 128 exceeds the chunk's 64 pixels
    (1, 32, 4160, 8),      # 65 chunks
]
GN_ALL_FAMILIES = [(3, 64, 64, 32), (3, 32, 100, 32)]
GN_VARIANT_SHAPES = [(3, 64, 64, 32), (2, 192, 36, 32)]
GN_VARIANTS = {
    'pitched': dict(pitched=True),
    'plain': dict(affine=False),
    'silu': dict(silu=True),
    'mod': dict(mod='both'),
    'mod_scale_silu': dict(mod='scale', silu=True),
    'mod_shift': dict(mod='shift'),
    'pitched_mod_silu': dict(pitched=True, mod='both', silu=True),
}


@functools.lru_cache(maxsize=None)
def gn_case(shape, fam, variant='default'):
    """One dm_groupnorm_nhwc case (shared; callers must not modify the tensors)."""
    B, C, HW, G = shape
    v = dict(pitched=False, affine=True, mod=None, silu=False)
    v.update(GN_VARIANTS.get(variant, {}))
    g = torch.Generator().manual_seed(_seed('gn', shape, fam, variant))
    x = family(fam, B, HW, C, G, g)
    xp, off, yp = (C + 8, 8, C + 4) if v['pitched'] else (C, 0, C)
    gamma, beta = affine(C, g) if v['affine'] else (None, None)
    modbuf = so = bo = None
    if v['mod']:
        modbuf, so, bo = mod_tables(B, C, g, scale=v['mod'] in ('both', 'scale'), shift=v['mod'] in ('both', 'shift'))
    return dict(B=B, C=C, HW=HW, G=G, x=x, xbuf=pitched(x, xp, off), off=off, y_pitch=yp, gamma=gamma, beta=beta,
                modbuf=modbuf, so=so, bo=bo, silu=v['silu'], eps=EPS)


# b. finalize on CPU-built partials
FIN_HW = [4096, 4097, 4160, 16384]     # 64 chunks (narrow), 65, 65, 256 (wide)
FIN_CG = [(256, 4), (32, 32), (12, 3)]  # cpg 64: two passes of the wide kernel's lane loop; B G = 9: a partial block
FIN_MODES = ['plain', 'mod', 'mod_scale']
FIN_FLAVOURS = ['spread', 'offset', 'clamp']


@functools.lru_cache(maxsize=None)
def fin_case(HW, C, G, mode, flavour, B=3):
    """Chunk partials of a plausible tensor built on the CPU: chunk k of (image, group) holds cnt_k cpg values of
    mean mu_k and variance s_k^2 (sum = n mu_k, sum of squares = n (s_k^2 + mu_k^2)). 'spread': O(1) statistics far
    apart across images; 'offset': mean 1024 4^b, sigma 4^b (mean / sigma = 2^10, as the data family); 'clamp': a
    constant 3e4 4^b map whose sum of squares came
    out 2^-40 low (fp64 accumulation over ~10^6 values reaches that), so q / n - m^2 < -eps and the clamp decides."""
    g = torch.Generator().manual_seed(_seed('fin', HW, C, G, mode, flavour))
    nch, cpg = nchunks(HW), C // G
    cnt = torch.tensor([min(CHUNK, HW - k * CHUNK) * cpg for k in range(nch)], dtype=F64)[None, :, None]
    img = torch.arange(B, dtype=F64)[:, None, None]
    z = torch.randn((B, nch, G), generator=g, dtype=F64)
    s = 0.5 + torch.rand((B, nch, G), generator=g, dtype=F64)
    if flavour == 'spread':
        mu, s = (0.5 + 10.0 * img) + 3.0 * 4.0 ** img * z, s * 4.0 ** img
    elif flavour == 'offset':
        mu, s = (1024.0 + 0.1 * z) * 4.0 ** img, s * 4.0 ** img
    else:
        mu, s = (3e4 * 4.0 ** img).expand(B, nch, G), torch.zeros((B, nch, G), dtype=F64)
    part = torch.stack([cnt * mu, cnt * (s * s + mu * mu)], dim=-1)
    if flavour == 'clamp':
        part[..., 1] *= 1.0 - 2.0 ** -40
    gamma = beta = modbuf = so = bo = None
    if mode != 'plain':
        gamma, beta = affine(C, g)
        modbuf, so, bo = mod_tables(B, C, g, scale=True, shift=mode == 'mod')
    return dict(B=B, HW=HW, C=C, G=G, part=part.contiguous(), gamma=gamma, beta=beta, modbuf=modbuf, so=so, bo=bo, eps=EPS)


@functools.lru_cache(maxsize=None)
def rechunk_case():
    """One tensor's statistics chunked two ways: per (image, group) 266240 values, as 4160 pixels of 64 channels
    (65 chunks: the wide kernel) and as 4096 pixels of 65 channels (64 chunks: the narrow one). G = 4, B = 3."""
    B, G, n = 3, 4, 4160 * 64
    g = torch.Generator().manual_seed(_seed('rechunk'))
    img = torch.arange(B, dtype=F32)[:, None, None]
    v = ((1024.0 + torch.randn((B, G, n), generator=g)) * torch.pow(torch.tensor(4.0), img) + 10.0 * img).to(F64)

    def chunks(nch):
        c = v.view(B, G, nch, n // nch)
        return torch.stack([c.sum(dim=3), (c * c).sum(dim=3)], dim=-1).permute(0, 2, 1, 3).contiguous()
    return dict(B=B, G=G, wide=dict(HW=4160, C=256, part=chunks(65)), narrow=dict(HW=4096, C=260, part=chunks(64)))


# c. (Ch, Gh, Cs, Gs, G)
CONCAT_CASES = [(256, 64, 128, 32, 32), (128, 16, 128, 16, 32), (64, 8, 192, 24, 32)]
CONCAT_HW = [64, 100]
CONCAT_REFUSED = [(256, 32, 128, 32, 32), (128, 16, 128, 16, 48), (128, 16, 128, 16, 0)]


@functools.lru_cache(maxsize=None)
def concat_case(Ch, Cs, HW, B=3):
    g = torch.Generator().manual_seed(_seed('concat', Ch, Cs, HW))
    return family('offset', B, HW, Ch + Cs, 1, g)


# d. convs whose epilogue emits the consumer's GroupNorm statistics (ConvArgs::gn_part through dm_debug_conv2d_gn).
# One entry per emitter: the forced tile, the smallest shape of the existing exact tests that the tile takes with
# HW % 64 == 0, the kernel the launch log must name, the group counts tried (cpg = Cout / G out of 1 .. 32, as the
# emitter admits: the K = 32 and Winograd epilogues store 4-channel quads, cpg 4 .. 32) and whether its chunks are
# 64 consecutive pixels ('slots') or any disjoint cover of the image
# ('cover': the 2-D tiles and the sub-pixel parities; the per-(image, group) totals are checked).
def _cv(name, kernel, G, B, Cin, Cout, H, W, tile, split='fp16x2', layout='slots', **kw):
    d = dict(name=name, kernel=kernel, G=G, B=B, Cin=Cin, Cout=Cout, H=H, W=W, tile=tile, split=split, layout=layout)
    d.update(kw)
    return d


CONV_GN_CASES = [
    _cv('patch128_fp32', 'conv_patch_kernel<128,128,64,64,0,288,false,false>', (64, 32), 3, 32, 64, 8, 8, 4, split=False),
    _cv('patch3_bf16x3', 'conv_patch3_kernel<128,128,64,64,0,208,false,false,3>',
        (32, 4), 3, 32, 64, 8, 8, 4, split='bf16x3'),
    _cv('patch3_fp16x2', 'conv_patch3_kernel<128,128,64,64,0,208,false,false,2>', (16, 2), 3, 32, 64, 8, 8, 4),
    _cv('patch3_128x64', 'conv_patch3_kernel<128,64,64,32,0,208,false,false,2>',
        (64, 8), 3, 32, 64, 8, 8, 5),
    _cv('patch3_256', 'conv_patch3_kernel<256,256,128,128,0,352,false,false,2>',
        (32, 4), 3, 64, 64, 16, 16, 7),
    _cv('patch3_512', 'conv_patch3_kernel<512,128,128,128,0,656,false,false,2>',
        (16, 2), 3, 64, 64, 16, 16, 8),
    _cv('patch3_segments', 'conv_patch3_kernel<128,128,64,64,0,392,false,false,2>',
        (32, 8), 2, 32, 64, 4, 256, 9),
    _cv('pw_1x1', 'conv_patch3_kernel<128,64,64,32,3,128,false,false,2>', (24, 96), 3, 64, 96, 8, 8, 0, taps=1),
    _cv('k32_v1', 'conv_k32_kernel<128,128,64,64,false,false,false>', (8, 2), 3, 64, 64, 8, 8, 10),
    _cv('k32_v2', 'conv_k32_kernel<128,64,64,32,false,false,false>', (4, 16), 3, 64, 64, 8, 8, 11),
    _cv('k32_v5_rows', 'conv_k32_kernel<64,128,32,64,false,false,false>', (32, 8), 2, 64, 128, 64, 64, 14),
    _cv('k32_v6_small', 'conv_k32s_kernel<false,8>', (16, 2), 3, 128, 64, 4, 4, 15, ksplit=2),
    _cv('k32_v7_wide', 'conv_k32_kernel<128,128,64,32,false,false,false,512>', (32, 4), 2, 64, 128, 64, 64, 16),
    _cv('k32_v8_bigtab', 'conv_k32_kernel<128,128,64,64,false,false,false,256,208,8192>',
        (16, 2), 3, 128, 64, 16, 16, 17),
    _cv('k32_v9_s2', 'conv_k32_kernel<64,128,32,32,false,false,false,512,392,2048,true>',
        (16, 8), 2, 64, 64, 32, 32, 18, stride=2),
    _cv('k32_v13_s2seg', 'conv_k32_kernel<64,128,32,32,false,false,false,512,392,2048,true>',
        (8, ), 1, 32, 64, 4, 256, 22,
        stride=2, s2_pad0=True),
    _cv('k32_v10_t2d', 'conv_k32_kernel<128,128,64,64,false,false,false,256,208,2048,false,true>',
        (24, 3), 2, 64, 96, 8, 64, 19, layout='cover'),
    _cv('k32_v11_8x8', 'conv_k32_kernel<64,128,32,64,false,false,false>', (16, 2), 3, 64, 64, 8, 8, 20),
    _cv('splitk_64', 'conv_k32_kernel<64,64,32,32,false,true,false>', (32, 8), 3, 128, 64, 4, 4, 12, ksplit=2),
    _cv('splitk_128_cout96', 'conv_k32_kernel<64,128,32,64,false,true,false>', (24, 3), 3, 128, 96, 4, 4, 13, ksplit=4),
    _cv('wino', 'conv_wino_kernel<16,0,false>', (32, 8, 4), 3, 64, 128, 16, 16, 21, wino=True),
    _cv('subpixel_v1', 'conv_k32_kernel<128,128,64,64,false,false,true>',
        (16, 2), 3, 64, 64, 16, 16, 10, up=2, layout='cover'),
    _cv('subpixel_v2', 'conv_k32_kernel<128,64,64,32,false,false,true>',
        (8, ), 3, 64, 64, 16, 16, 11, up=2, layout='cover'),
    _cv('subpixel_t2d', 'conv_k32_kernel<128,128,64,64,false,false,true,256,208,2048,false,true>',
        (8, ), 2, 64, 32, 8, 128, 19, up=2, layout='cover'),
    # the automatic pick: narrow maps take 128-row tiles only from 512 blocks on (a 64-row tile, which emits nothing,
    # at any batch a test can afford); a 64-pixel-wide map goes to the 2-D tiles at every batch
    _cv('auto_wide', 'conv_k32_kernel<128,128,64,64,false,false,false,256,208,2048,false,true>',
        (16, ), 2, 64, 64, 8, 64, 0,
        layout='cover'),
]
# refused before any launch (conv2d_igemm's check of conv_can_emit_gn): HW % 64 != 0, a 64-row tile, groups of 64
# columns on the K = 32 kernel, groups of 3, the automatic pick of a small batch (a 64-row tile)
CONV_GN_REFUSED = [
    _cv('hw_36', '', (32, ), 3, 64, 64, 6, 6, 10, refuse=True),
    _cv('tile_64_rows', '', (32, ), 3, 64, 64, 8, 8, 6, refuse=True),
    _cv('k32_cpg_64', '', (2, ), 3, 64, 128, 8, 8, 10, refuse=True),
    _cv('cpg_3', '', (32, ), 3, 64, 96, 8, 8, 10, refuse=True),
    _cv('auto_64_row_tile', '', (16, ), 3, 64, 64, 8, 8, 0, refuse=True),
]


def _freeze(s):
    return tuple(sorted((k, v) for k, v in s.items() if k not in ('G', 'name', 'kernel', 'layout', 'refuse')))


@functools.lru_cache(maxsize=None)
def _conv_case(key):
    s = dict(key)
    B, Cin, Cout, H, W = s['B'], s['Cin'], s['Cout'], s['H'], s['W']
    taps = s.get('taps', 9)
    g = torch.Generator().manual_seed(_seed('conv', key))
    if s.get('up'):
        Ho, Wo = 2 * H, 2 * W
    elif s.get('stride', 1) == 2:
        Ho, Wo = ((H - 2) // 2 + 1, (W - 2) // 2 + 1) if s.get('s2_pad0') else ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    else:
        Ho, Wo = H, W
    k = 3 if taps == 9 else 1
    x = torch.randn((B, Cin, H, W), generator=g) * torch.pow(torch.tensor(2.0), torch.arange(B, dtype=F32))[:, None, None, None]
    w = torch.randn((Cout, Cin, k, k), generator=g) / (taps * Cin) ** 0.5
    return dict(x=x, w=w, bias=torch.randn((Cout, ), generator=g), Ho=Ho, Wo=Wo, y_pitch=Cout + 32,
                rowvec=(100.0 * torch.arange(1, B + 1, dtype=F32))[:, None].expand(B, Cout).contiguous(),
                res=torch.randn((B, Ho, Wo, Cout), generator=g))


def conv_case(s):
    """Operands of one conv case: x NCHW (image b times 2^b), w torch layout, bias, rowvec 100 (b + 1), residual NHWC."""
    return _conv_case(_freeze(s))


# d. the GEMM epilogue's statistics (GemmArgs::gn_part through dm_debug_gemm_gn): gemm.hip emits them from its 128-row
# tiles only, which gemm_pick takes from 512 tiles and N >= 128 on -- M = 65536, N = 128 is the smallest such GEMM.
GEMM_GN_CASES = [
    dict(name='fp32', split=0, G=128, M=65536, N=128, K=32, hw=8192),       # cpg 1
    dict(name='fp16x2', split=2, G=4, M=65536, N=128, K=32, hw=8192),       # cpg 32
]
GEMM_GN_REFUSED = [dict(name='64_row_tiles', split=0, G=32, M=256, N=128, K=32, hw=64)]


@functools.lru_cache(maxsize=None)
def _gemm_case(key):
    s = dict(key)
    M, N, K, hw = s['M'], s['N'], s['K'], s['hw']
    g = torch.Generator().manual_seed(_seed('gemm', key))
    img = (torch.arange(M) // hw).to(F32)[:, None]
    return dict(A=torch.randn((M, K), generator=g) * (1.0 + img), W=torch.randn((N, K), generator=g) / K ** 0.5,
                bias=torch.randn((N, ), generator=g), res=100.0 * (img + 1.0) + torch.randn((M, N), generator=g),
                ldc=N + 32)


def gemm_case(s):
    """Operands of one GEMM case: A rows of image b times (1 + b), a residual of 100 (b + 1) + N(0, 1)."""
    return _gemm_case(tuple(sorted((k, v) for k, v in s.items() if k in ('M', 'N', 'K', 'hw'))))


# e. the convs' in-kernel GroupNorm finalize (ConvArgs::gin_* through dm_debug_conv2d_gin), one case per kernel
# family for which ConvChoice::lds_tables holds; B = 3, GroupNorm(32) of the input.
CONV_GIN_CASES = [
    # the 8^2 map on the two-image 128 x 128 tile, the 16^2 map on a two-images-per-block (512-row) tile, the 1x1
    _cv('patch3_8x8_two_images', 'conv_patch3_kernel<128,128,64,64,0,208,true', (), 3, 64, 64, 8, 8, 4),
    _cv('patch3_512_16x16_two_images', 'conv_patch3_kernel<512,128,128,128,0,656,true', (), 3, 64, 64, 16, 16, 8),
    _cv('pw_1x1', 'conv_patch3_kernel<128,64,64,32,3,128,true', (), 3, 64, 96, 8, 8, 0, taps=1),
    # ConvChoice::lds_tables is a statement about the automatic pick (tile 0), so the K = 32 and Winograd kernels are
    # reached the way the plans reach them: a 64-pixel-wide map (2-D tiles), a split-K 4 x 4 map, Winograd weights
    _cv('k32_t2d_wide', 'conv_k32_kernel<128,128,64,64,true', (), 3, 64, 64, 8, 64, 0),
    _cv('k32s_4x4', 'conv_k32s_kernel<true', (), 3, 128, 64, 4, 4, 0, ksplit=2),
    _cv('wino_16x16', 'conv_wino_kernel<16,', (), 3, 64, 128, 16, 16, 0, wino=True),
]
CONV_GIN_REFUSED = [
    _cv('fp32_weights', '', (), 3, 64, 64, 8, 8, 4, split=False, refuse=True),
    _cv('bf16x3_weights', '', (), 3, 64, 64, 8, 8, 4, split='bf16x3', refuse=True),
    _cv('forced_k32_tile', '', (), 3, 64, 64, 8, 8, 10, refuse=True),   # (lds_tables knows the patch tiles only)
]


@functools.lru_cache(maxsize=None)
def _gin_case(key, mod):
    s = dict(key)
    c = dict(_conv_case(key))
    B, Cin, H, W = s['B'], s['Cin'], s['H'], s['W']
    g = torch.Generator().manual_seed(_seed('gin', key, mod))
    x = (c['x'] + 3.0 * torch.arange(B, dtype=F32)[:, None, None, None]).contiguous()   # statistics far apart
    part, _ = partial_ref(x.permute(0, 2, 3, 1).reshape(B, H * W, Cin), 32)
    gamma, beta = affine(Cin, g)
    modbuf, so, bo = mod_tables(B, Cin, g) if mod else (None, None, None)
    c.update(x=x, G=32, eps=EPS, gamma=gamma, beta=beta, modbuf=modbuf, so=so, bo=bo,
             part=torch.cat([part.reshape(-1, 2), torch.full((TAIL, 2), NAN, dtype=F64)]))
    return c


def gin_case(s, mod):
    """conv_case's operands with image b shifted by 3 b, the float64 chunk partials of x for GroupNorm(32), gamma /
    beta and (mod) AdaGN tables inside a wider NaN-filled buffer (gin_mp > Cin)."""
    return _gin_case(_freeze(s), bool(mod))


# f. the first conv: (Cin, H, W, Cout), every (H, W) x Cout with Cin cycling through what fits the LDS
SI_HW = [(32, 32), (28, 28), (16, 16), (8, 8), (4, 4), (2, 128), (3, 192)]
SI_COUT = [96, 128, 192, 256, 320, 512, 1024]
SI_G = [8, 16, 32]


def small_in_cases():
    out, i = [], 0
    for H, W in SI_HW:
        for Cout in SI_COUT:
            i += 1
            if Cout == 1024:
                cin = 1
            else:
                cin = next(c for c in ((i + d) % 4 + 1 for d in range(4)) if small_in_fits(c, H, W, Cout, False))
            out.append((cin, H, W, Cout))
    return out


@functools.lru_cache(maxsize=None)
def small_in_case(Cin, H, W, Cout, B=3):
    """Integer operands (exact in fp32); image b is scaled by b + 1."""
    g = torch.Generator().manual_seed(_seed('si', Cin, H, W, Cout))
    x = ints((B, Cin, H, W), g) * torch.arange(1, B + 1, dtype=F32)[:, None, None, None]
    w, bias = ints((Cout, Cin, 3, 3), g), ints((Cout, ), g, -8, 9)
    return dict(x=x, w=w, bias=bias, ref=conv3x3_f64(x, w, bias), y_pitch=Cout + 4)


# g. the last conv
SO_HW = [(8, 32), (9, 33), (28, 28), (3, 5)]
SO_CIN = [32, 96, 512]


def small_out_cases():
    """(Cout, H, W, Cin): every Cout 1..8, every (H, W), every Cin, each pair of them at least once."""
    out = []
    for i, Cout in enumerate(range(1, 9)):
        for j in range(2):
            H, W = SO_HW[(i + 2 * j) % 4]
            out.append((Cout, H, W, SO_CIN[(i + j) % 3]))
    return out


@functools.lru_cache(maxsize=None)
def small_out_case(Cout, H, W, Cin, kind, B=3):
    """kind 'int': integer operands; 'gn': the benign family with a GroupNorm(32) + SiLU prologue."""
    g = torch.Generator().manual_seed(_seed('so', Cout, H, W, Cin, kind))
    if kind == 'int':
        x = ints((B, H, W, Cin), g) * torch.arange(1, B + 1, dtype=F32)[:, None, None, None]
        w, bias = ints((Cout, Cin, 3, 3), g), ints((Cout, ), g, -8, 9)
        gamma = beta = None
    else:
        x = family('benign', B, H * W, Cin, 32, g).view(B, H, W, Cin)
        w, bias = torch.randn((Cout, Cin, 3, 3), generator=g) / (3.0 * Cin ** 0.5), torch.randn((Cout, ), generator=g)
        gamma, beta = affine(Cin, g)
    xbuf = torch.full((B, H, W, Cin + 4), NAN)
    xbuf[..., :Cin] = x
    return dict(x=x, xbuf=xbuf, w=w, bias=bias, gamma=gamma, beta=beta, G=32, eps=EPS)


# h. (B, C, Hin, Win)
RS_SHAPES = [(2, 8, 6, 10), (3, 64, 4, 4)]


@functools.lru_cache(maxsize=None)
def resample_case(shape, kind):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(_seed('rs', shape, kind))
    if kind == 'int':
        x = ints((B, H, W, C), g, -8, 9) * torch.arange(1, B + 1, dtype=F32)[:, None, None, None]
        sc = sh = None
    else:
        x = family('benign', B, H * W, C, 1, g).view(B, H, W, C)
        sc = (0.2 + torch.rand((B, C), generator=g)) * torch.pow(torch.tensor(0.25), torch.arange(B, dtype=F32))[:, None]
        sh = torch.randn((B, C), generator=g) - torch.arange(B, dtype=F32)[:, None]
    xbuf = torch.full((B, H, W, C + 8), NAN)
    xbuf[..., :C] = x
    return dict(x=x, xbuf=xbuf, sc=sc, sh=sh, y_pitch=C + 4)
