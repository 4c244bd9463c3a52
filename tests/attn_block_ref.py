"""Host-side inputs, references and emulation for the folded UNet attention blocks (csrc/attn_block.hip:
attn_block3_kernel, attn_block4_kernel<8>, attn_small_kernel and the fold helpers).

Plain torch on the CPU, shared by tests/test_attn_block_host.py (no GPU) and tests/test_gpu_attn_block_ops.py.

The block is y = x + proj(softmax(s q k^T) v) on xn = x gsc + gsh (the GroupNorm tables of the image), q / k / v / proj
1x1 convs with biases. The kernels run its folded form: T = xn At^T + w, S = T xn^T, P = softmax(S),
y = x + (P xn) Wg^T + cb with At = s Wk^T Wq, w = s Wk^T bq, Wg = Wp Wv, cb = Wp bv + bp; the terms s xn_i^T Wq^T bk and
s bq . bk are constant along the key and dropped.

* unfolded(c, dtype): the module as the reference model writes it. Its float32 error against float64 is e32.
* fold_f64 / fold_f32: the fold products; split_decode: a matrix as its fp16x2 image holds it (row scale 2^e with
  max |row| 2^e in [2^13, 2^14), hi = fp16, lo = fp16(rest); token_ref.weight_row_exponents / split_exact).
* folded(c, fw, dtype): the folded form on given fold operands. On the decoded At / Wg it is the reference of variants
  3 / 4 (kernel_refs(c, fw, True)); on the fp32 ones that of attn_small, which is fp32 throughout
  (kernel_refs(c, fw, False)). Its float32 error is the yardstick e32f.
* emulation(c, fw, mutant): variants 3 / 4 restated in fp32 (module docstring of test_attn_block_host.py has the
  steps), with the channel permutation pi of the staged key image, of T's accumulators and of Wg' carried explicitly,
  and MUTANTS of it that the host test must see fail.
* case(family, L, B): the seeded input families, cached.

The smallest |T| the kernel scales correctly: the per-query scale is ldexpf(1, 14 - E) with max |T| in [2^(E-1), 2^E),
finite for 14 - E <= 127, i.e. max |T| >= 2^-114 (about 2^-113 with margin); below that it is inf and inf 0 = NaN for
the row's zero elements. The `tiny` family stays at 2^-100.
"""
import functools
import math
import zlib

import torch

from tests import norm_ref as nr
from tests import token_ref as tr

F32, F64 = torch.float32, torch.float64
C = 256
EX = 6                         # the plan's activation exponent (unet_exec.hip: ab.ex = 6)
EP = 14                        # P x 2^14
LOG2E32 = torch.tensor(1.4426950408889634, dtype=F32)
FP16_MAX = 65504.0
REL = 2.0 ** -21
FAMILIES = ['flat', 'peaked', 'ramp8', 'ramp40', 'ramp200', 'desc8', 'desc40', 'desc200', 'bigbk', 'gnwide', 'zeroq',
            'tiny', 'select']
MUTANTS = ['no_o_rescale', 'no_l_rescale', 'chunk_max', 'drop_a1b0_s', 'drop_a1b0_pv', 'no_w', 'no_cb', 'bk_back',
           'pi_keys_only', 'wg_pi_once', 'swap_chunks_p']


def pi32(m):
    """Storage position m of a 32-channel group holds channel pi32(m) (attn_block.hip pi32)."""
    return 4 * (m >> 3) + (m & 3) + 16 * ((m >> 2) & 1)


PI = torch.tensor([(p & ~31) + pi32(p & 31) for p in range(C)])   # storage position -> channel
PIPI = PI[PI]                                                     # Wg' column -> Wg column


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def hadamard(n):
    h = torch.ones((1, 1), dtype=F64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def _derangement(n, g):
    while True:
        p = torch.randperm(n, generator=g)
        if not (p == torch.arange(n)).any():
            return p


# ------------------------------------------------------------------------------------------------------ families
def _select_case(L, B, g):
    H = hadamard(C)
    # pi permutes within blocks of 16 rows, without fixed points, so a 16-token image (one block) is closed under it
    pi = torch.cat([16 * a + _derangement(16, g) for a in range(C // 16)])
    Wq = (H[pi].T @ H) / C                      # Wq h_m = h_pi(m); entries multiples of 1 / 256
    eye = torch.eye(C, dtype=F64)
    Wp = torch.randint(-2, 3, (C, C), generator=g).to(F64)
    bp = torch.randint(-3, 4, (C, ), generator=g).to(F64)
    rows, win = [], []
    for b in range(B):
        if L == C:
            rho = torch.randperm(C, generator=g)
        else:
            rho = 16 * int(torch.randint(0, C // 16, (1, ), generator=g)) + torch.randperm(16, generator=g)
        inv = {int(r): i for i, r in enumerate(rho)}
        rows.append(H[rho])
        win.append(torch.tensor([inv[int(pi[r])] for r in rho]))
    x = torch.stack(rows)
    z = torch.zeros(C, dtype=F64)
    return dict(x=x, gsc=torch.ones((B, C), dtype=F64), gsh=torch.zeros((B, C), dtype=F64), Wq=Wq, Wk=eye, Wv=eye,
                bq=z, bk=z, bv=z, Wp=Wp, bp=bp, scale=1.0, win=torch.stack(win))


def generate(fam, L, B):
    """One family at L tokens and B images, all float32 (select's are exact): x [B, L, C], gsc / gsh [B, C], Wq, Wk, Wv,
    Wp [C, C], bq, bk, bv, bp [C], scale; `win` [B, L] the winning key of each query (select)."""
    g = torch.Generator().manual_seed(_seed('attn_block', fam, L, B))
    if fam == 'select':
        c = _select_case(L, B, g)
    else:
        rn = lambda *s: torch.randn(s, generator=g, dtype=F64)  # noqa: E731
        Wq, Wk, Wv, Wp = (rn(C, C) / C ** 0.5 for _ in range(4))
        bq, bk, bv, bp = (0.3 * rn(C) for _ in range(4))
        scale = 1.0 / 16
        xn = rn(B, L, C)
        gsc = 1.0 + 0.5 * torch.rand((B, C), generator=g, dtype=F64)
        gsh = 0.5 * rn(B, C)
        if fam == 'peaked':
            Wq = Wq * 8
        elif fam.startswith('ramp') or fam.startswith('desc'):
            gap = float(fam[4:])
            u = rn(C)
            u = u / u.norm()
            proj = torch.eye(C, dtype=F64) - torch.outer(u, u)
            Wk = proj @ Wk @ proj + torch.outer(u, u)     # Wk preserves u and maps nothing else onto it
            Wq = Wq * 0.25                                # the random part of the scores: about 0.25 nats
            r = torch.arange(L, dtype=F64) / (L - 1)
            if fam.startswith('desc'):
                r = 1.0 - r
            a = (gap / scale) ** 0.5
            xn = xn @ proj + a * r[None, :, None] * u
            bq = bq @ proj + a * u
        elif fam == 'bigbk':
            bk = 50.0 * rn(C)
            bq = bq + 2.0 * bk / bk.norm()
        elif fam == 'gnwide':
            gsc = gsc * (4.0 ** torch.arange(B, dtype=F64))[:, None]
            gsh = 8.0 * rn(B, C)
            for b in range(B):   # one element per image at max |xn| = 900 (x 2^6 = 57600 < 65504)
                xn[b, (37 + 11 * b) % L, (101 + 64 * b) % C] = 900.0 * (-1) ** b
        elif fam == 'zeroq':
            Wq, bq = Wq * 0, bq * 0
        elif fam == 'tiny':
            Wq, bq = Wq * 2.0 ** -98, bq * 2.0 ** -98   # max |T| about 2^-100
        elif fam != 'flat':
            raise ValueError(fam)
        c = dict(x=(xn - gsh[:, None]) / gsc[:, None], gsc=gsc, gsh=gsh, Wq=Wq, Wk=Wk, Wv=Wv, bq=bq, bk=bk, bv=bv,
                 Wp=Wp, bp=bp, scale=scale, win=None)
    for k, v in c.items():
        if torch.is_tensor(v) and v.dtype == F64:
            c[k] = v.to(F32)
    c.update(fam=fam, L=L, B=B)
    return c


@functools.lru_cache(maxsize=None)
def case(fam, L, B):
    """generate(), cached and shared: callers must not modify the tensors."""
    return generate(fam, L, B)


def gnwide_twin(c):
    """gnwide with image B - 1's planted element at |xn| = 1100: x 2^6 is beyond fp16, the range flag must rise."""
    t = dict(c)
    b = c['B'] - 1
    i, ch = (37 + 11 * b) % c['L'], (101 + 64 * b) % C
    x = c['x'].clone()
    x[b, i, ch] = ((1100.0 * (-1) ** b - c['gsh'][b, ch].double()) / c['gsc'][b, ch].double()).to(F32)
    t['x'] = x
    return t


def wqkv(c):
    """The parameters as the engine holds them: wqkv [3 C][C], bqkv [3 C]."""
    return torch.cat([c['Wq'], c['Wk'], c['Wv']]).contiguous(), torch.cat([c['bq'], c['bk'], c['bv']]).contiguous()


# ---------------------------------------------------------------------------------------------------- references
def xn_of(c, dtype):
    return c['x'].to(dtype) * c['gsc'].to(dtype)[:, None] + c['gsh'].to(dtype)[:, None]


def scores_f64(c):
    """The module's float64 scores s q k^T, [B, L, L]."""
    d = F64
    xn = xn_of(c, d)
    q = xn @ c['Wq'].to(d).T + c['bq'].to(d)
    k = xn @ c['Wk'].to(d).T + c['bk'].to(d)
    return c['scale'] * (q @ k.transpose(1, 2))


def unfolded(c, dtype):
    d = dtype
    xn = xn_of(c, d)
    q = xn @ c['Wq'].to(d).T + c['bq'].to(d)
    k = xn @ c['Wk'].to(d).T + c['bk'].to(d)
    v = xn @ c['Wv'].to(d).T + c['bv'].to(d)
    s = torch.tensor(c['scale'], dtype=d)
    p = torch.softmax((q @ k.transpose(1, 2)) * s, dim=-1)
    return c['x'].to(d) + ((p @ v) @ c['Wp'].to(d).T + c['bp'].to(d))


def fold_f64(c):
    """The fold in float64 with the error each fp32 result may carry: 2^-24 |v| + C 2^-53 sum|term| (one rounding to
    fp32 of a C-term float64 sum). -> dict(at, w, wg, cb) and dict of bounds."""
    d = F64
    Wq, Wk, Wv, Wp = (c[k].to(d) for k in ('Wq', 'Wk', 'Wv', 'Wp'))
    bq, bv, bp, s = c['bq'].to(d), c['bv'].to(d), c['bp'].to(d), c['scale']
    v = dict(at=s * (Wk.T @ Wq), w=s * (Wk.T @ bq), wg=Wp @ Wv, cb=Wp @ bv + bp)
    a = dict(at=abs(s) * (Wk.abs().T @ Wq.abs()), w=abs(s) * (Wk.abs().T @ bq.abs()), wg=Wp.abs() @ Wv.abs(),
             cb=Wp.abs() @ bv.abs() + bp.abs())
    return v, {k: 2.0 ** -24 * v[k].abs() + C * 2.0 ** -53 * a[k] for k in v}


def fold_f32(c):
    """The fold as the engine stores it: float64 products rounded once to fp32."""
    return {k: v.to(F32) for k, v in fold_f64(c)[0].items()}


def split_decode(W):
    """W [rows, K] fp32 as its fp16x2 image holds it, fp32 (exact)."""
    e = tr.weight_row_exponents(W)
    return torch.ldexp(tr.split_exact(torch.ldexp(W, e[:, None]), 0), -e[:, None])


def folded(c, fw, dtype, bk_terms=False):
    """The folded form on the fold operands fw (at, w, wg, cb). bk_terms: the dropped key-constant terms added back
    (they must cancel: the proof of the fold algebra)."""
    d = dtype
    xn = xn_of(c, d)
    t = xn @ fw['at'].to(d).T + fw['w'].to(d)
    s = t @ xn.transpose(1, 2)
    if bk_terms:
        q = xn @ c['Wq'].to(d).T + c['bq'].to(d)
        s = s + c['scale'] * (q @ c['bk'].to(d))[..., None]
    p = torch.softmax(s, dim=-1)
    return c['x'].to(d) + ((p @ xn) @ fw['wg'].to(d).T + fw['cb'].to(d))


def kernel_refs(c, fw, decoded):
    """The kernel's float64 reference on the fold results fw it really consumed (the hook's, or fold_f32's), the
    yardstick e32f and the bound 2 e32f + 2^-21 max|ref|. decoded: variants 3 / 4 (At, Wg through the fp16x2 split)."""
    ops = dict(fw)
    if decoded:
        ops['at'], ops['wg'] = split_decode(fw['at']), split_decode(fw['wg'])
    ref = folded(c, ops, F64)
    e32f = float((folded(c, ops, F32).double() - ref).abs().max())
    scale = float(ref.abs().max())
    return dict(ref=ref, e32f=e32f, scale=scale, bound=2.0 * e32f + REL * scale)


def module_refs(c):
    ref = unfolded(c, F64)
    e32 = float((unfolded(c, F32).double() - ref).abs().max())
    scale = float(ref.abs().max())
    return dict(ref=ref, e32=e32, scale=scale, bound=2.0 * e32 + REL * scale)


def chunk_maxima(c, chunk=32):
    """Per query the maximum float64 score of every key chunk, [B, L, L / chunk]."""
    s = scores_f64(c)
    return s.view(c['B'], c['L'], c['L'] // chunk, chunk).amax(dim=-1)


def select_answer(c):
    """select's exact rows: g [B, L, C] (integers) and y = x + g[win]."""
    g = c['x'].double() @ c['Wp'].double().T + c['bp'].double()
    gw = torch.gather(g, 1, c['win'][..., None].expand(-1, -1, C))
    return g, c['x'].double() + gw


def partials_of(x, G):
    """GroupNorm(G) chunk partials of the rows x [B, L, C] as float64 [B, nchunk, G, 2] (norm_ref.partial_ref)."""
    return nr.partial_ref(x, G)[0]


# ----------------------------------------------------------------------------------------------------- emulation
def _split(v):
    hi = v.to(torch.float16).to(F32)
    return hi, (v - hi).to(torch.float16).to(F32)


def _mm3(a, b, drop=False):
    """a1 b0 + a0 b1 + a0 b0 with fp32 sums; a, b = (hi, lo) piece pairs, contraction a[..., m, k] b[..., n, k]."""
    bt0, bt1 = b[0].transpose(-1, -2), b[1].transpose(-1, -2)
    if drop:
        return a[0] @ bt1 + a[0] @ bt0
    return (a[1] @ bt0 + a[0] @ bt1) + a[0] @ bt0


def emulation(c, fw, mutant=None):
    """attn_block3_kernel / attn_block4_kernel in fp32 on the fp32 fold results fw. -> dict(y [B, L, C] fp32, flag)."""
    assert c['L'] == 256 and mutant in (None, *MUTANTS)
    B, L = c['B'], c['L']
    x = c['x']
    xs = torch.ldexp(xn_of(c, F32), torch.tensor(EX))
    flag = int((xs.abs() > FP16_MAX).any())
    xp = _split(xs)                                               # natural channel order [B, L, C]
    kimg = (xp[0][..., PI], xp[1][..., PI])                       # the staged key image: storage order
    # 1. T = xn At^T + w
    ea = tr.weight_row_exponents(fw['at'])
    ap = _split(torch.ldexp(fw['at'], ea[:, None]))
    w = torch.zeros_like(fw['w']) if mutant == 'no_w' else fw['w']
    T = _mm3(xp, ap) * torch.ldexp(torch.ones(C), -ea - EX) + w   # [B, L, C'] natural order
    m = T.abs().amax(dim=-1)
    _, E = torch.frexp(m)
    eT = torch.where(m > 0, 14 - E, torch.zeros_like(E))
    tp_nat = _split(T * torch.ldexp(torch.ones_like(m), eT)[..., None])
    # T's accumulators as S's B operand: position p holds channel PI[p]
    tp = tp_nat if mutant == 'pi_keys_only' else (tp_nat[0][..., PI], tp_nat[1][..., PI])
    tun = torch.ldexp(torch.ones_like(m), -(EX + eT))
    sl2 = tun * LOG2E32                                           # [B, L]
    back = None
    if mutant == 'bk_back':   # the dropped key-constant terms, with the wrong sign, in accumulator units
        q = xn_of(c, F32) @ c['Wq'].T + c['bq']
        back = -(c['scale'] * (q @ c['bk'])) / tun
    # 2. the key pass
    m_run = torch.full((B, L), -math.inf, dtype=F32)
    l_run = torch.zeros((B, L), dtype=F32)
    O = torch.zeros((B, L, C), dtype=F32)                         # storage order
    for kc in range(8):
        ks = slice(32 * kc, 32 * kc + 32)
        kk = (kimg[0][:, ks], kimg[1][:, ks])
        S = _mm3(kk, tp, drop=mutant == 'drop_a1b0_s').transpose(1, 2)   # [B, L queries, 32 keys]
        if back is not None:
            S = S + back[..., None]
        cm = S.amax(dim=-1) * sl2
        m_new = cm if mutant == 'chunk_max' else torch.maximum(m_run, cm)
        corr = torch.exp2(m_run - m_new)
        arg = (S.double() * sl2.double()[..., None] - m_new.double()[..., None]).to(F32)   # the FMA: one rounding
        v = torch.exp2(arg)
        l_run = (l_run if mutant == 'no_l_rescale' else l_run * corr) + v.sum(dim=-1)
        pp = _split(v * 16384.0)
        if kc > 0 and mutant != 'no_o_rescale':
            O = O * corr[..., None]
        if mutant == 'swap_chunks_p' and kc in (2, 5):
            o = 5 if kc == 2 else 2
            kk = (kimg[0][:, 32 * o:32 * o + 32], kimg[1][:, 32 * o:32 * o + 32])
        kt = (kk[0].transpose(1, 2), kk[1].transpose(1, 2))        # [B, C storage, 32]
        O = O + _mm3(kt, pp, drop=mutant == 'drop_a1b0_pv').transpose(1, 2)
        m_run = m_new
    op_st = _split(O * (1.0 / (16384.0 * l_run))[..., None])
    # O's accumulators as the projection's B operand: position p' holds storage row PI[p'], channel PI[PI[p']]
    op = (op_st[0][..., PI], op_st[1][..., PI])
    # 3. Y = Wg' O, y = x + (Y + cb)
    wgp = fw['wg'][:, PI if mutant == 'wg_pi_once' else PIPI]
    eg = tr.weight_row_exponents(wgp)
    gp = _split(torch.ldexp(wgp, eg[:, None]))
    Y = _mm3(op, gp) * torch.ldexp(torch.ones(C), -eg - EX)
    cb = torch.zeros_like(fw['cb']) if mutant == 'no_cb' else fw['cb']
    return dict(y=x + (Y + cb), flag=flag)
