"""Host-side references, case builders and an fp32 emulation for the unfused attention chain: the batched split S GEMM
(csrc/gemm.hip, B read [n][k]), softmax_rows (csrc/elementwise.hip) and the batched split PV GEMM (B read [k][n]),
as the plans issue them (unet_exec.hip, dit_exec.hip, vae_blocks.h attn_block).

Plain torch on the CPU, shared by tests/test_unfused_attention_host.py (no GPU) and
tests/test_gpu_unfused_attention_ops.py. The score distributions, the fp16x2 packers and the attention references are
tests/attention_ref.py's; `equal` and `near_fp16` are tests/test_gpu_pesser.py's.

* CASES: the (B, heads, L, Dh) shapes, each the smallest at which a mechanism of the chain exists, with the qkv row
  layout ('blocks': q | k | v column blocks, hs = Dh; 'legacy': per head [q; k; v], hs = 3 Dh), the plans' scales
  (blocks: alpha = Dh^-1/2 on q; legacy: alpha = b_scale = Dh^-1/4 on q and k, ADM's form) and the nominal pick_Z.
* case / case_from_rows: the fp32 rows [B L][3 C] the device reads (q / alpha, k / b_scale, v), the effective operands
  as the device forms them (q_eff = fl32(q_rows alpha), k_eff = fl32(k_rows b_scale)), the operands decoded after
  the 2^6 split, and per arithmetic (split 2: decoded operands; split 0: the effective ones) the float64 S and O with
  the float32 yardstick's error of each. P's and the PV stage's references depend on the scores / probabilities the
  backend produced, so softmax_refs / pv_refs compute them from those.
* bound: the project's own, 2 e32 + 2^-21 max|ref64|; e32 is torch's float32 evaluation of the same stage on the same
  operands, never a measurement of the code under test.
* EmuBackend: the interface of the GPU tests' device backend (s_gemm, softmax, pv_gemm) answered by the device
  arithmetic restated in fp32: three-term fp16x2 products a1 b0 + a0 b1 + a0 b0 accumulated in fp32 at the exponents
  6 / 6 (S) and 14 / 6 (PV), un-scaled at the end, the range predicate |x 2^e| > 65504 (split 0: plain fp32), and
  softmax_rows' max / exp / sum / scale. It allocates the same NaN-prefilled, pitched buffers with sentinel rows.

Cached tensors are shared: callers must not modify them.
"""
import functools

import torch

from tests import attention_ref as ar

F32, F64 = torch.float32, torch.float64
REL = 2.0 ** -21
FP16_MAX = ar.FP16_MAX
E_S = (ar.EA, ar.EB)      # the S GEMM's exponents (split_gemm(gs, 6, ..., 6))
E_PV = (ar.EP, ar.EV)     # the PV GEMM's (split_gemm(go, 14, ..., 6))
PAD_C = 8                 # NaN columns after N in every GEMM output row (ldc = N + 8)
PAD_SM = 4                # softmax_rows' own tests: ld = L + 4 (rows stay 16-byte aligned)
SENT_ROWS = 4             # NaN rows past the last row of every output
PICK_BATCH = 256          # kPickBatch: the plans pass pick_Z = kPickBatch heads


def f32(x):
    return float(torch.tensor(x, dtype=F32))


def sid(shape):
    return 'x'.join(map(str, shape))


# shape, layout, nominal pick_Z (0: the actual Z), the score distributions run on it (select first)
CASES = [
    dict(shape=(3, 1, 36, 64), layout='blocks', pick_Z=0, dists=['select', 'peaked', 'equal']),
    dict(shape=(2, 1, 40, 128), layout='blocks', pick_Z=0, dists=['select', 'ramp40', 'near_fp16']),
    dict(shape=(2, 3, 64, 72), layout='blocks', pick_Z=0, dists=['select', 'desc200', 'offset']),
    dict(shape=(1, 2, 100, 32), layout='legacy', pick_Z=0, dists=['select', 'flat', 'offset']),
    dict(shape=(2, 2, 256, 64), layout='legacy', pick_Z=0, dists=['select', 'peaked', 'ramp40']),
    dict(shape=(1, 1, 576, 64), layout='blocks', pick_Z=0, dists=['select', 'desc200', 'offset']),
    dict(shape=(2, 1, 136, 128), layout='blocks', pick_Z=PICK_BATCH, dists=['select', 'flat', 'near_fp16']),
]
TAIL_SHAPES = [c['shape'] for c in CASES if c['shape'][2] % 32 != 0 or c['shape'][3] % 32 != 0]
ALL_DISTS = ['flat', 'peaked', 'ramp40', 'desc200', 'offset', 'select', 'equal', 'near_fp16']
CASE_DISTS = [(c, d) for c in CASES for d in c['dists']]
ISOLATION_SHAPE = (2, 2, 100, 32)
FUSED_SHAPES = ar.L256_SHAPES
FUSED_DISTS = ar.L256_DISTS + ['peaked', 'offset']
SOFTMAX_L = [36, 100, 256, 500, 576, 1024]
SOFTMAX_ROWS = 37


def case_id(c):
    return sid(c['shape']) + ('_pick' if c['pick_Z'] else '')


def scales(shape, layout):
    """(alpha, b_scale) of the plans: blocks alpha = Dh^-1/2, no B scaling; legacy alpha = b_scale = Dh^-1/4."""
    Dh = shape[3]
    if layout == 'legacy':
        return f32(Dh ** -0.25), f32(Dh ** -0.25)
    return f32(Dh ** -0.5), 0.0


def pick_of(c):
    """(pick_M, pick_Z) the device hook gets, or None: dm_gemm's own choice."""
    return (0, c['pick_Z'] * c['shape'][1]) if c['pick_Z'] else None


# ---------------------------------------------------------------------------------------------------- row layouts
def offsets(shape, layout):
    """Float offsets of q, k, v in a row and the head stride (AttnArgs q0 / k0 / v0 / hs)."""
    B, H, L, Dh = shape
    C = H * Dh
    if layout == 'legacy':
        return dict(q0=0, k0=Dh, v0=2 * Dh, hs=3 * Dh)
    return dict(q0=0, k0=C, v0=2 * C, hs=Dh)


def pack_rows(q, k, v, layout):
    """[B, heads, L, Dh] x 3 -> rows [B L][3 C]: 'blocks' q | k | v, 'legacy' per head [q; k; v]."""
    B, H, L, Dh = q.shape
    t = [x.permute(0, 2, 1, 3).reshape(B * L, H, Dh) for x in (q, k, v)]
    if layout == 'legacy':
        return torch.stack(t, dim=2).reshape(B * L, 3 * H * Dh).contiguous()
    return torch.cat([x.reshape(B * L, H * Dh) for x in t], dim=1).contiguous()


def unpack_rows(rows, shape, layout):
    """The device's addressing restated: element (b, h, l, d) of part p at rows[b L + l][p0 + h hs + d]."""
    B, H, L, Dh = shape
    o = offsets(shape, layout)
    out = []
    for p0 in (o['q0'], o['k0'], o['v0']):
        heads = [rows[:, p0 + h * o['hs']:p0 + h * o['hs'] + Dh].reshape(B, L, Dh) for h in range(H)]
        out.append(torch.stack(heads, dim=1))
    return out


def outside_mask(shape, layout, b=0, h=0):
    """True at every element of the rows that does not belong to image b, head h."""
    B, H, L, Dh = shape
    o = offsets(shape, layout)
    m = torch.ones((B * L, 3 * H * Dh), dtype=torch.bool)
    for p0 in (o['q0'], o['k0'], o['v0']):
        m[b * L:(b + 1) * L, p0 + h * o['hs']:p0 + h * o['hs'] + Dh] = False
    return m


# ---------------------------------------------------------------------------------------------------------- cases
def generate(shape, dist):
    """attention_ref.generate plus test_gpu_pesser's `equal` (all keys identical) and `near_fp16` (+-1000)."""
    from tests.test_gpu_pesser import _equal_rows, _near_fp16
    if dist == 'equal':
        return _equal_rows(shape)
    if dist == 'near_fp16':
        return _near_fp16(shape)
    return ar.generate(shape, dist)


def _scaled(x, s):
    return x if s in (0.0, 1.0) else x * torch.tensor(s, dtype=F32)


def bound(e32, ref):
    return 2.0 * e32 + REL * ref.abs().max().item()


def _err32(y32, ref):
    return (y32.to(F64) - ref).abs().max().item()


def case_from_rows(rows, shape, layout, alpha, b_scale):
    """Everything derived from the fp32 rows the device reads. ops[split] are the float64 operands that arithmetic
    multiplies: the decoded fp16x2 pieces (2) or the effective fp32 values (0)."""
    q_rows, k_rows, v = unpack_rows(rows, shape, layout)
    q_eff, k_eff = _scaled(q_rows, alpha), _scaled(k_rows, b_scale)
    dec = ar.pack_planes(q_eff, k_eff, v, E_S[0], E_S[1], E_PV[1])[3]
    c = dict(rows=rows, shape=shape, layout=layout, alpha=alpha, b_scale=b_scale, q_eff=q_eff, k_eff=k_eff, v=v,
             ops={2: dec, 0: (q_eff.to(F64), k_eff.to(F64), v.to(F64))}, ref={})
    for split, (qd, kd, vd) in c['ops'].items():
        S = qd @ kd.transpose(-1, -2)
        S_e32 = _err32(qd.float() @ kd.float().transpose(-1, -2), S)
        O = ar.attention_f64(qd, kd, vd)
        O_e32 = _err32(ar.attention_f32(qd, kd, vd), O)
        c['ref'][split] = dict(S=S, S_e32=S_e32, S_bound=bound(S_e32, S), O=O, O_e32=O_e32, O_bound=bound(O_e32, O))
    return c


@functools.lru_cache(maxsize=None)
def case(shape, dist, layout, alpha, b_scale):
    """One (shape, distribution, layout, scales). The generated (q, k, v) are the EFFECTIVE operands: the rows hold
    q / alpha and k / b_scale in fp32, and the device's products fl32(row alpha) round as they do there."""
    q, k, v, pi = generate(shape, dist)
    q_rows = q if alpha in (0.0, 1.0) else (q / alpha).float()
    k_rows = k if b_scale in (0.0, 1.0) else (k / b_scale).float()
    c = case_from_rows(pack_rows(q_rows, k_rows, v, layout), shape, layout, alpha, b_scale)
    c['pi'] = pi
    return c


def table_case(c, dist):
    return case(c['shape'], dist, c['layout'], *scales(c['shape'], c['layout']))


def softmax_refs(x):
    """fp32 scores [..., L] -> dict(ref float64 softmax of those scores, e32, bound); max|ref| <= 1."""
    ref = torch.softmax(x.to(F64), dim=-1)
    e32 = _err32(torch.softmax(x.to(F32), dim=-1), ref)
    return dict(ref=ref, e32=e32, bound=bound(e32, ref))


def pv_refs(P, vd, split):
    """fp32 P [B, heads, L, L] (what the PV GEMM reads) and the v operand -> float64 P v of the operands that
    arithmetic multiplies (split 2: P decoded after its 2^14 split), e32, bound."""
    if split == 2:
        hi, lo = ar.split_planes(P, E_PV[0])
        Pd = torch.ldexp(hi.to(F64) + lo.to(F64), torch.tensor(-E_PV[0]))
    else:
        Pd = P.to(F64)
    ref = Pd @ vd
    e32 = _err32(Pd.float() @ vd.float(), ref)
    return dict(ref=ref, e32=e32, bound=bound(e32, ref))


def select_margin(c):
    """Smallest lead (nats) of the winning key over every other key, on the decoded operands."""
    qd, kd, _ = c['ops'][2]
    S = qd @ kd.transpose(-1, -2)
    win = torch.gather(S, 3, c['pi'][..., None])
    rest = S.scatter(3, c['pi'][..., None], float('-inf'))
    return (win[..., 0] - rest.amax(dim=-1)).min().item()


def max_scaled(c):
    """Largest |operand 2^e| any split of the chain sees: q_eff, k_eff, v at 2^6 (P 2^14 <= 16384)."""
    return max(x.abs().max().item() for x in (c['q_eff'], c['k_eff'], c['v'])) * 2.0 ** 6


@functools.lru_cache(maxsize=None)
def integer_case(shape, layout):
    """Small-integer operands with power-of-two scales: q, k in [-4, 4], v in [-8, 8], alpha = 1/2, b_scale = 1/4,
    and a 'P' of multiples of 1/4 in [0, 3.75] (x 2^14 = 61440, inside fp16). Every product and partial sum is exact
    in fp32 and in the fp16x2 split, so both arithmetics must return the float64 result exactly."""
    B, H, L, Dh = shape
    g = torch.Generator().manual_seed(ar._seed(shape, 'integer-' + layout))
    q = torch.randint(-4, 5, shape, generator=g).float()
    k = torch.randint(-4, 5, shape, generator=g).float()
    v = torch.randint(-8, 9, shape, generator=g).float()
    P = torch.randint(0, 16, (B, H, L, L), generator=g).float() / 4.0
    alpha, b_scale = 0.5, 0.25
    S = (q.to(F64) * alpha) @ (k.to(F64) * b_scale).transpose(-1, -2)
    return dict(rows=pack_rows(q, k, v, layout), shape=shape, layout=layout, alpha=alpha, b_scale=b_scale, P=P, S=S,
                O=P.to(F64) @ v.to(F64))


@functools.lru_cache(maxsize=None)
def softmax_case(L):
    """SOFTMAX_ROWS rows of L scores: rows 0..2 all-equal (3.25, 250, -250), then rows of N(0, 4) scores shifted
    by 0, +250 and -250 in turn, and every seventh row x 8 (peaked)."""
    g = torch.Generator().manual_seed(ar._seed((SOFTMAX_ROWS, L), 'softmax'))
    x = torch.randn((SOFTMAX_ROWS, L), generator=g) * 2.0
    x[6::7] *= 8.0
    x += torch.tensor([0.0, 250.0, -250.0])[torch.arange(SOFTMAX_ROWS) % 3][:, None]
    for r, val in enumerate((3.25, 250.0, -250.0)):
        x[r] = val
    return x


# -------------------------------------------------------------------------------------------------- the emulation
def emu_gemm(a, bt, split, ea, eb):
    """a [..., M, K] @ bt [..., K, N] in the device arithmetic restated in fp32 -> (fp32 result, range flag)."""
    if split == 0:
        return a @ bt, 0
    flag = int((torch.ldexp(a, torch.tensor(ea)).abs() > FP16_MAX).any() or
               (torch.ldexp(bt, torch.tensor(eb)).abs() > FP16_MAX).any())
    a0, a1 = (t.to(F32) for t in ar.split_planes(a, ea))
    b0, b1 = (t.to(F32) for t in ar.split_planes(bt, eb))
    acc = (a1 @ b0 + a0 @ b1) + a0 @ b0
    return acc * 2.0 ** -(ea + eb), flag


def emu_softmax(x):
    """softmax_rows_kernel's expression in fp32: e = exp(x - max), e (1 / sum e)."""
    e = torch.exp(x - x.amax(dim=-1, keepdim=True))
    return e * (1.0 / e.sum(dim=-1, keepdim=True))


def s_buffer(shape):
    B, H, L, _ = shape
    return torch.full((B * H * L + SENT_ROWS, L + PAD_C), float('nan'))


def o_buffer(shape):
    B, H, L, Dh = shape
    return torch.full((B * L + SENT_ROWS, H * Dh + PAD_C), float('nan'))


class EmuBackend:
    """The device backend's interface on the CPU. A spec is a dict(rows, shape, layout, alpha, b_scale, split,
    pick = (pick_M, pick_Z) | None, sub = (Z1, Z2) | None: the leading images / heads computed, P for pv_gemm: the
    [B heads L + SENT_ROWS, L + PAD_C] buffer softmax left)."""
    name = 'emulation'

    def s_gemm(self, s):
        """-> dict(C [B heads L + SENT_ROWS, L + PAD_C], flag, labels)."""
        B, H, L, Dh = s['shape']
        Z1, Z2 = s.get('sub') or (B, H)
        q, k, _ = unpack_rows(s['rows'], s['shape'], s['layout'])
        a, b = _scaled(q[:Z1, :Z2], s['alpha']), _scaled(k[:Z1, :Z2], s['b_scale'])
        y, flag = emu_gemm(a, b.transpose(-1, -2), s['split'], *E_S)
        out = s_buffer(s['shape'])
        out[:B * H * L].view(B, H, L, L + PAD_C)[:Z1, :Z2, :, :L] = y
        return dict(C=out, flag=flag, labels=None)

    def softmax(self, x, rows, L, ld, offset=0):
        """softmax_rows on a copy of the flat fp32 buffer x, the first row `offset` floats in -> the buffer."""
        out = x.clone()
        v = out.view(-1)[offset:offset + rows * ld].view(rows, ld)
        v[:, :L] = emu_softmax(v[:, :L])
        return out

    def pv_gemm(self, s):
        """-> dict(C [B L + SENT_ROWS, heads Dh + PAD_C], flag, labels)."""
        B, H, L, Dh = s['shape']
        Z1, Z2 = s.get('sub') or (B, H)
        _, _, v = unpack_rows(s['rows'], s['shape'], s['layout'])
        P = s['P'][:B * H * L].view(B, H, L, L + PAD_C)[:Z1, :Z2, :, :L]
        y, flag = emu_gemm(P, v[:Z1, :Z2], s['split'], *E_PV)
        out = o_buffer(s['shape'])
        o = out[:B * L].view(B, L, H * Dh + PAD_C)
        for h in range(Z2):
            o[:Z1, :, h * Dh:(h + 1) * Dh] = y[:, h]
        return dict(C=out, flag=flag, labels=None)
