// 3x3 stride-1 convolution in the conv-half arithmetic: ONE v_mfma_f32_16x16x32_f16 product per
// MAC, where conv_k32.hip spends three on its fp16x2 split and conv_wino.hip two -- the opt-in throughput option of
// the UNet plans (dm_unet_set_conv_half), the conv sibling of linear_h16.hip.
//
// Numerics: a' = fp16_rne(prologue(x1)) and a2' = fp16_rne(x2) come ONLY as images, fp16 planes [B][H][W][C] written
// once per conv by conv_h16_image (conv_k32's prologue expressions -- the affine in fp32, silu_fast -- so a' is bit
// for bit piece 0 of the split conv_k32 does on load; unscaled, as there). w' is piece 0 of the fp16x2 fragment image
// split_conv_weights already holds (the per-output-channel power-of-two row scale included), read in place: the
// option owns no weight copy. acc = sum_k a' w' over both K segments in the MFMA's fp32 accumulator, times
// ws_rowscale[n] (exact), then conv_k32's fp32 epilogue (StagedEpilogue: bias, per-image row vector, residual,
// pitched 16-B stores, the consumer's GroupNorm chunk partials). |prologue(x1)| or |x2| > 65504 raises range_flag at
// the image pass (a plain vector store); the kernel itself checks nothing.
//
// Kernel: conv_k32's variant-1 / variant-10 structure with one piece. 128 x 128 blocks of four waves, 64 x 64 wave
// tiles (4 x 4 tiles of 16 x 16: 64 accumulator registers); convs of more than 256 input channels run eight waves of
// 64 x 32 with a second accumulator set (a two-level sum: see the kernel). Per 32-channel chunk the halo patch of the plane (at most
// 208 pixels x 64 B) goes into LDS once -- four threads per pixel, one 16-B load each, no conversion: zero padding by
// address (the static zero page with a zero chunk stride), never a select on loaded data -- and the 9 taps read
// shifted A fragments from it, one K = 32 MFMA step per tap; the segment-2 chunks follow as plain K steps on 128 rows
// of the second plane. B fragments (piece 0) come from L2 into a 2-deep register ring, as in conv_k32 / linear_h16.
// LDS: a pixel row is 160 B (10 16-B slots: the ds_read_b128 lane groups of a 16-row fragment are conflict free,
// conv_k32's pitch), the two chunk buffers side by side inside it (buffer b at byte 64 b: a shift by 4 slots moves
// every lane of a group alike), 208 x 160 B = 33 KB, shared with the epilogue's slabs (34 / 36 KB). One barrier per
// chunk; the next chunk's patch travels in two halves (loaded at taps 0 / 4, stored at taps 3 / 7).
// Tile forms (PatchGeom): 1 -- whole rows of 8- / 16- / 32-wide maps (8 x 8 maps: two images per tile, an odd last
// image alone); 2 -- 4 rows x 32 columns of 64- .. 256-wide maps (t2d_pixel order). The form depends on the shape
// only and there is no split-K, so image i of a batch equals its own B = 1 result bit for bit.
#include <string>

#include "dm_common.h"
#include "dm_kernels.h"
#include "mfma_tile.h"
#include "split16.h"
#include "conv_epilogue.h"

namespace dm {

namespace {

constexpr int kHC = 32;      // input channels per chunk = K of one tap's MFMA step
constexpr int kHRow = 80;    // LDS pixel pitch in fp16 (160 B); chunk buffer b at +32 b
constexpr int kHFlush = 8;   // chunks per first-level accumulation (even: the main loop takes two chunks per turn)
constexpr int kHMaxP = 208;  // patch pixels: 32-wide 6 x 34, 16-wide 10 x 18, 8 x 8 maps 2 x 10 x 10, 2-D tiles 6 x 34

// conv_h16_image: one thread per 8 consecutive channels of a pixel of an NHWC fp32 view (channel pitch >= C):
// conv_k32's prologue expressions, one rounding to fp16, the plane [pixel][C]. PRO 0: none, 1: affine + SiLU,
// 2: the affine alone.
template <int PRO>
__global__ void __launch_bounds__(256) conv_h16_image_kernel(const float* __restrict__ x, int pitch, int C, long npix,
                                                             int hw, const float* __restrict__ sc,
                                                             const float* __restrict__ sh, void* out_,
                                                             int* range_flag) {
  _Float16* out = reinterpret_cast<_Float16*>(out_);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int per = C / 8;
  if (i >= npix * per) return;
  const long p = i / per;
  const int c = (int)(i - p * per) * 8;
  const float* src = x + (size_t)p * pitch + c;
  f4 v0 = *reinterpret_cast<const f4*>(src), v1 = *reinterpret_cast<const f4*>(src + 4);
  if (PRO) {
    const size_t o = (size_t)(p / hw) * C + c;
    const f4 s0 = *reinterpret_cast<const f4*>(sc + o), s1 = *reinterpret_cast<const f4*>(sc + o + 4);
    const f4 h0 = *reinterpret_cast<const f4*>(sh + o), h1 = *reinterpret_cast<const f4*>(sh + o + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a0 = v0[e] * s0[e] + h0[e], a1 = v1[e] * s1[e] + h1[e];
      v0[e] = PRO == 1 ? silu_fast(a0) : a0;
      v1[e] = PRO == 1 ? silu_fast(a1) : a1;
    }
  }
  f16x8 h;
  float mx = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = (_Float16)v0[e];
    h[4 + e] = (_Float16)v1[e];
    mx = fmaxf(mx, fmaxf(fabsf(v0[e]), fabsf(v1[e])));
  }
  *reinterpret_cast<f16x8*>(out + (size_t)p * C + c) = h;
  if (mx > 65504.f && range_flag) *range_flag = 1;
}

// WN 64: four waves of 64 x 64. WN 32 (LONGK: more than kHFlush chunks, Cin1 > 256): eight waves of 64 x 32 and the
// two-level accumulation below -- both accumulator sets are the registers of one 64 x 64 set.
template <bool T2D, int WN>
__global__ void __launch_bounds__(2 * (128 / WN) * 64) __attribute__((amdgpu_waves_per_eu(2, 2)))
conv_h16_kernel(ConvArgs a, PatchGeom g) {
  constexpr int BM = 128, BN = 128, WM = 64, NT = (BM / WM) * (BN / WN) * 64;
  constexpr bool LONGK = WN == 32;
  constexpr int NWN = BN / WN, TM = WM / 16, TN = WN / 16;
  constexpr int SROWS = NT / 4, PJ = (kHMaxP + SROWS - 1) / SROWS;  // patch pixels per loader pass; 4 or 2 passes
  constexpr int HP = PJ / 2;                                        // passes per loader half
  constexpr int WD = 2;
  typedef StagedEpilogue<WN> Epi;
  constexpr int LDS_H = kHMaxP * kHRow > (NT / 64) * 32 * Epi::EP * 2 ? kHMaxP * kHRow : (NT / 64) * 32 * Epi::EP * 2;
  __shared__ __attribute__((aligned(16))) _Float16 patch[LDS_H];

  const int Ho = a.Hout, Wo = a.Wout, HWo = Ho * Wo;
  const int M = a.B * HWo, N = a.Cout;
  const int nN = ceil_div(N, BN);
  const int bid = xcd_remap_p(blockIdx.x, gridDim.x);
  const int mt = bid / nN, nt = bid - mt * nN;  // N tiles fastest: the blocks of one M tile share its patch in L2
  const int m0 = mt * BM, n0 = nt * BN;
  const int b0 = m0 / HWo;
  const int tl2 = (m0 - b0 * HWo) / BM, ntx2 = Wo / g.TW;
  const int y0 = T2D ? (tl2 / ntx2) * g.TH : (m0 - b0 * HWo) / Wo;
  const int x0 = T2D ? (tl2 - (tl2 / ntx2) * ntx2) * g.TW : 0;

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave / NWN, wn = wave % NWN;
  const int l16 = lane & 15, q = lane >> 4;
  const int srow = t >> 2, sq = t & 3;  // loader: pixel slot, 8-channel quarter of the chunk

  // ---- patch loader: pixel p = srow + 64 j of the TB x PH x PW patch; outside the map (and beyond the batch or the
  // patch) the zero page with a zero chunk stride
  const _Float16* psrc[PJ];
  int pstep[PJ];
  const int PHW = g.PH * g.PW;
#pragma unroll
  for (int j = 0; j < PJ; ++j) {
    const int p = srow + SROWS * j;
    const int img = p / PHW;
    const int rem = p - img * PHW;
    const int pr = rem / g.PW, pc = rem - pr * g.PW;
    const int b = b0 + img;
    const int iy = y0 - 1 + pr, ix = x0 + pc - 1;
    const bool ok = p < g.P && b < a.B && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
    psrc[j] = ok ? a.h16_a1 + ((size_t)(b * a.Hin + iy) * a.Win + ix) * a.Cin1 + 8 * sq
                 : reinterpret_cast<const _Float16*>(kZeroPage) + 8 * sq;
    pstep[j] = ok ? kHC : 0;
  }

  // ---- B operand: piece 0 of the fp16x2 fragment images [16-slice][32-col group][piece][2 lane groups][32][8]
  const int ngrp = ceil_div(N, 32);
  const size_t sl = (size_t)ngrp * 1024;  // fp16 elements per 16-deep slice
  const _Float16* wbase[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * WN + j * 16 + l16;
    const int grp = min(col >> 5, ngrp - 1);  // columns >= N: clamped / zero padding, never stored
    wbase[j] = reinterpret_cast<const _Float16*>(a.ws) + (size_t)grp * 1024 + ((q & 1) * 32 + (col & 31)) * 8;
  }
  const size_t qoff = (size_t)(q >> 1) * 9 * sl;  // k-groups 2, 3: the chunk's second 16-slice of the tap
  // step kt = c * 9 + tap of the main segment: 16-slices 2c * 9 + tap (+ 9 for k-groups 2, 3)
  auto slice_off = [&](int kt) { return (size_t)(kt + (kt / 9) * 9) * sl + qoff; };
  f16x8 bq[WD][TN];
  auto load_b = [&](f16x8 (&dst)[TN], size_t off) {
#pragma unroll
    for (int j = 0; j < TN; ++j) dst[j] = *reinterpret_cast<const f16x8*>(wbase[j] + off);
  };

  // ---- A-fragment patch rows of this lane (row l16 of each 16-row tile)
  int abase0[TM];
  const int tile_rows = g.TH * g.TW;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int ml = wm * WM + i * 16 + l16;
    const int fimg = ml / tile_rows;
    const int rem = ml - fimg * tile_rows;
    const int fy = rem / g.TW, fx = rem - fy * g.TW;
    abase0[i] = ((fimg * g.PH + fy) * g.PW + fx) * kHRow + q * 8;
  }

  // the next chunk's patch in two halves (passes 0-1, then 2-3) through two registers
  static_assert(PJ == 2 * HP, "two loader halves");
  f16x8 rp[HP];
  auto load_patch = [&](int chunk, int j0) {
#pragma unroll
    for (int j = j0; j < j0 + HP; ++j) rp[j - j0] = *reinterpret_cast<const f16x8*>(psrc[j] + chunk * pstep[j]);
  };
  auto store_patch = [&](int buf, int j0) {
#pragma unroll
    for (int j = j0; j < j0 + HP; ++j) {
      const int p = srow + SROWS * j;
      if (p < kHMaxP) *reinterpret_cast<f16x8*>(patch + p * kHRow + buf * kHC + sq * 8) = rp[j - j0];
    }
  };

  f4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  // one K = 32 step: A rows at LDS element offsets abase[i] + off, B in registers
  auto compute = [&](const int (&abase)[TM], int off, const f16x8 (&bv)[TN]) {
    f16x8 av[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) av[i] = *reinterpret_cast<const f16x8*>(patch + abase[i] + off);
    __builtin_amdgcn_sched_barrier(0);  // the step's fragment reads issued before its first MFMA
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[i], bv[j], acc[i][j], 0, 0, 0);
  };

  // Two-level accumulation: one accumulator over all of K = 9 Cin1 is a sequential fp32 chain of 9 Cin1 / 32 MFMA
  // steps (576 at Cin1 = 2048), whose rounding error grows with its length; every kHFlush chunks (72 steps) the
  // running sums move into a second accumulator set. The schedule depends on the shape only (batch-invariant), and
  // integer operands stay exact in any order.
  f4 tot[LONGK ? TM : 1][LONGK ? TN : 1];
#pragma unroll
  for (int i = 0; i < (LONGK ? TM : 1); ++i)
#pragma unroll
    for (int j = 0; j < (LONGK ? TN : 1); ++j) tot[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  auto flush = [&]() {
#pragma unroll
    for (int i = 0; i < (LONGK ? TM : 0); ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        tot[i][j] = tot[i][j] + acc[i][j];
        acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
      }
  };
  const int nch = a.Cin1 / kHC, kt_end = nch * 9;
#pragma unroll
  for (int d = 0; d < WD; ++d) load_b(bq[d], slice_off(min(d, kt_end - 1)));
  load_patch(0, 0);
  store_patch(0, 0);
  load_patch(0, HP);
  store_patch(0, HP);
  __syncthreads();
  // One barrier per chunk: chunk c is read from buffer c & 1 while chunk c + 1 goes into the other buffer (free since
  // every wave passed the previous chunk's barrier): passes 0-1 loaded at tap 0 and stored at tap 3, passes 2-3 loaded
  // at tap 4 and stored at tap 7. After the last chunk the reload goes into the unused buffer.
  for (int c0 = 0; c0 < nch; c0 += 2) {
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int c = c0 + cc;
      if (c >= nch) break;
      const int cn = min(c + 1, nch - 1);
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int kt = c * 9 + tap;
        const int slot = (cc * 9 + tap) % WD;
        if (tap == 0 || tap == 4) {
          load_patch(cn, tap == 0 ? 0 : HP);
          __builtin_amdgcn_sched_barrier(0);
        }
        compute(abase0, ((tap / 3) * g.PW + tap % 3) * kHRow + cc * kHC, bq[slot]);
        load_b(bq[slot], slice_off(min(kt + WD, kt_end - 1)));
        __builtin_amdgcn_sched_barrier(0);  // keep the refill WD taps ahead
        if (tap == 3 || tap == 7) store_patch(cc ^ 1, tap == 3 ? 0 : HP);
      }
      __syncthreads();
    }
    if (LONGK && (c0 + 2) % kHFlush == 0 && c0 + 2 < nch) flush();
  }

  // ---- segment 2: the 1x1 product of the second plane (the ResBlock shortcut), K = Cin2 in 32-channel steps on the
  // tile's 128 rows (buffer 0), un-pipelined
  if (a.Cin2 > 0) {
    constexpr int RJ = BM / SROWS;
    const size_t s2 = (size_t)(9 * a.Cin1 / 16) * sl + (size_t)(q >> 1) * sl;  // 16-slices 9 Cin1 / 16 + 2 c2 + (q >> 1)
    int abase[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) abase[i] = (wm * WM + i * 16 + l16) * kHRow + q * 8;
    const _Float16* xsrc[RJ];
#pragma unroll
    for (int j = 0; j < RJ; ++j) {  // rows >= M read clamped data: never stored
      const int m = min(m0 + srow + SROWS * j, M - 1);
      xsrc[j] = a.h16_a2 + (T2D ? t2d_pixel(m, HWo, Wo, g.TH, g.TW) : (size_t)m) * a.Cin2 + 8 * sq;
    }
    for (int c2 = 0; c2 < a.Cin2 / kHC; ++c2) {
      f16x8 r[RJ];
#pragma unroll
      for (int j = 0; j < RJ; ++j) r[j] = *reinterpret_cast<const f16x8*>(xsrc[j] + c2 * kHC);
      load_b(bq[0], s2 + (size_t)(2 * c2) * sl);
#pragma unroll
      for (int j = 0; j < RJ; ++j) *reinterpret_cast<f16x8*>(patch + (srow + SROWS * j) * kHRow + sq * 8) = r[j];
      __syncthreads();
      compute(abase, 0, bq[0]);
      __syncthreads();
    }
  }

  // ---- epilogue (conv_k32's): per 32 of the wave's 64 rows the accumulators, row scale undone, go to this wave's
  // slab [32][WN + 4] fp32 of the (now free) patch buffer; then 4 consecutive columns per lane: bias, row vector,
  // residual, 16-B store. The wave's 64 rows are one 64-pixel chunk of one image (HW % 64 == 0): its GroupNorm partials.
  float* st = reinterpret_cast<float*>(patch) + wave * 32 * Epi::EP;
  const int wrow0 = m0 + wm * WM;
  Epi epi(a, M, HWo, b0, (HWo % BM) == 0, n0 + wn * WN, lane);
  if (T2D) epi.t2d(Wo, g.TH, g.TW);
  float cs[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) cs[j] = a.ws_rowscale[min(n0 + wn * WN + j * 16 + l16, N - 1)];
#pragma unroll
  for (int i = 0; i < (LONGK ? TM : 0); ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = tot[i][j] + acc[i][j];
#pragma unroll
  for (int h = 0; h < WM / 32; ++h) {
#pragma unroll
    for (int i = 2 * h; i < 2 * h + 2; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[((i - 2 * h) * 16 + 4 * q + r) * Epi::EP + j * 16 + l16] = acc[i][j][r] * cs[j];
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes are visible to its reads
    __builtin_amdgcn_wave_barrier();
    epi.rows(st, wrow0 + 32 * h);
    __builtin_amdgcn_wave_barrier();  // the next slab's writes reuse the region
    if (a.gn_part && (h & 1)) epi.emit(wrow0 + 32 * (h - 1));
  }
}

// form 1's geometry: conv_patch_geom's whole-row 128-pixel tiles of an 8- / 16- / 32-wide map
bool rows_geom(const ConvArgs& a, PatchGeom& g) {
  if (a.Wout != 8 && a.Wout != 16 && a.Wout != 32) return false;
  return conv_patch_geom(a, 128, g) && g.P <= kHMaxP && g.TB <= 2 && g.TW == a.Wout;
}
// form 2's: 4 output rows x 32 columns per tile, a 6 x 34 patch (conv_k32's T2D)
bool t2d_geom_h(const ConvArgs& a, PatchGeom& g) {
  if (a.Wout < 64 || a.Wout > 256 || a.Wout % 32 != 0 || a.Hout % 4 != 0) return false;
  g.TB = 1;
  g.TH = 4;
  g.TW = 32;
  g.PH = 6;
  g.PW = 34;
  g.P = 204;
  return true;
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

H16Form conv_h16_form(const ConvArgs& a) {
  if (a.tile < 0 || a.tile > 2) return H16Form::None;
  // the covered convs
  if (a.taps != 9 || a.stride != 1 || a.upsample != 0 || a.ksplit > 1) return H16Form::None;
  if (a.Cin1 < kHC || a.Cin1 % kHC != 0 || a.Cin2 < 0 || a.Cin2 % kHC != 0 || a.Cout <= 0 || a.Cout % 32 != 0) return H16Form::None;
  if (a.K != 9 * a.Cin1 + a.Cin2 || a.B <= 0 || a.Hin != a.Hout || a.Win != a.Wout) return H16Form::None;
  if ((long)a.Hout * a.Wout < 64 || (long)a.B * a.Hout * a.Wout >= (1L << 31)) return H16Form::None;
  if (!(a.ws && a.ws_np == 2 && a.ws_rowscale && al16(a.ws))) return H16Form::None;
  if (a.Cin2 > 0 && !a.x2) return H16Form::None;
  if (!al16(a.h16_a1) || !al16(a.h16_a2)) return H16Form::None;
  if (!staged_epilogue_ok(a)) return H16Form::None;
  if (a.gn_part && !conv_h16_can_emit(a)) return H16Form::None;
  PatchGeom g;
  const H16Form form = rows_geom(a, g) ? H16Form::Rows : t2d_geom_h(a, g) ? H16Form::T2D : H16Form::None;
  return (a.tile == 0 || a.tile == (int)form) ? form : H16Form::None;  // (tile 1 / 2 force Rows / T2D)
}

bool conv_h16_ok(const ConvArgs& a) { return conv_h16_form(a) != H16Form::None; }

// StagedEpilogue<64>'s rule: every wave's 64 rows are one 64-pixel chunk of one image, groups of 4, 8, 16 or 32 channels
bool conv_h16_can_emit(const ConvArgs& a) {
  if (a.gn_G <= 0 || a.Cout % a.gn_G != 0 || (a.Hout * a.Wout) % 64 != 0) return false;
  const int cpg = a.Cout / a.gn_G;
  return cpg == 4 || cpg == 8 || cpg == 16 || cpg == 32;
}

static const char* h16_name(H16Form form, bool longk) {
  return form == H16Form::T2D ? (longk ? "conv_h16_kernel<true,32>" : "conv_h16_kernel<true,64>")
                   : (longk ? "conv_h16_kernel<false,32>" : "conv_h16_kernel<false,64>");
}

std::string conv_h16_label(const ConvArgs& a, H16Form form) { return h16_name(form, a.Cin1 / kHC > kHFlush); }

int conv_h16_image(const ConvArgs& a, _Float16* plane1, _Float16* plane2, hipStream_t st) {
  auto launch = [&](const float* x, int pitch, int C, long npix, int hw, const float* sc, const float* sh, int pro,
                    _Float16* out) -> int {
    DM_REQUIRE(x && out && C > 0 && C % 8 == 0 && pitch >= C && pitch % 4 == 0 && al16(x) && al16(out),
               "conv_h16_image: C % 8 == 0 and 16-byte aligned rows");
    DM_REQUIRE(!pro || (sc && sh && al16(sc) && al16(sh)), "conv_h16_image: GroupNorm tables");
    const long blocks = (npix * (C / 8) + 255) / 256;
    DM_REQUIRE(blocks > 0 && blocks < (1L << 31), "conv_h16_image: too many pixels");
    void* o = out;
    if (pro == 1)
      hipLaunchKernelGGL(conv_h16_image_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, x, pitch, C, npix, hw, sc,
                         sh, o, a.range_flag);
    else if (pro == 2)
      hipLaunchKernelGGL(conv_h16_image_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, st, x, pitch, C, npix, hw, sc,
                         sh, o, a.range_flag);
    else
      hipLaunchKernelGGL(conv_h16_image_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, x, pitch, C, npix, hw, sc,
                         sh, o, a.range_flag);
    DM_LAUNCH_CHECK();
    return DM_OK;
  };
  DM_REQUIRE(a.B > 0 && a.Hin > 0 && a.Win > 0, "conv_h16_image: empty problem");
  if (plane1) {
    const int pro = a.pro_scale ? (a.pro_nosilu ? 2 : 1) : 0;
    if (const int rc = launch(a.x1, a.x1_pitch, a.Cin1, (long)a.B * a.Hin * a.Win, a.Hin * a.Win, a.pro_scale,
                              a.pro_shift, pro, plane1))
      return rc;
  }
  if (plane2 && a.Cin2 > 0) {
    if (const int rc = launch(a.x2, a.x2_pitch, a.Cin2, (long)a.B * a.Hout * a.Wout, a.Hout * a.Wout, nullptr, nullptr,
                              0, plane2))
      return rc;
  }
  return DM_OK;
}

int conv2d_h16(const ConvArgs& a, hipStream_t st) {
  const H16Form form = conv_h16_form(a);
  DM_REQUIRE(form != H16Form::None && a.h16_a1 && (a.Cin2 == 0 || a.h16_a2),
             "conv_h16: needs the fp16 image plane(s), fp16x2 split weights and a covered 3x3 stride-1 shape");
  PatchGeom g;
  if (form == H16Form::Rows) rows_geom(a, g);
  else t2d_geom_h(a, g);
  const int M = a.B * a.Hout * a.Wout;
  const int blocks = ceil_div(M, 128) * ceil_div(a.Cout, 128);
  const bool longk = a.Cin1 / kHC > kHFlush;
  if (form == H16Form::Rows && longk) hipLaunchKernelGGL((conv_h16_kernel<false, 32>), dim3(blocks), dim3(512), 0, st, a, g);
  else if (form == H16Form::Rows) hipLaunchKernelGGL((conv_h16_kernel<false, 64>), dim3(blocks), dim3(256), 0, st, a, g);
  else if (longk) hipLaunchKernelGGL((conv_h16_kernel<true, 32>), dim3(blocks), dim3(512), 0, st, a, g);
  else hipLaunchKernelGGL((conv_h16_kernel<true, 64>), dim3(blocks), dim3(256), 0, st, a, g);
  note_launch(h16_name(form, longk));
  DM_LAUNCH_CHECK();
  return DM_OK;
}

}  // namespace dm

/* Test hooks (tests/test_gpu_conv_h16.py), synchronous, allocate nothing; not in the public header.
 * dm_debug_conv_h16_image: the image pass of `d` alone: the plane [B][Hin][Win][Cin] of prologue(x) at `image`, then,
 * where d has a second segment, the plane [B][Hout][Wout][Cin2] of x2 at the next 16-byte boundary after it.
 * dm_debug_conv_h16: the image pass, then the conv on it. tile 0: the automatic form; 1: whole rows of 8- / 16- /
 * 32-wide maps; 2: 2-D tiles of 64- .. 256-wide maps. A conv conv_h16_ok refuses (a forced form on a shape it does
 * not take included) returns DM_ERR_UNSUPPORTED and launches nothing. w_split must be a DM_SPLIT_FP16X2 image. With
 * gn_part (dm_debug_conv_h16_gn) also the GroupNorm(G) chunk partials of the stored output. */
static int h16_desc(const dm_conv_desc* d, void* image, int tile, dm::ConvArgs& a) {
  using namespace dm;
  if (!d || !d->x || !d->w || !d->y || !image) { set_error("null tensor"); return DM_ERR_ARG; }
  if (!d->w_split || d->w_split_kind != DM_SPLIT_FP16X2) {
    set_error("conv_h16: w_split must be a DM_SPLIT_FP16X2 image");
    return DM_ERR_ARG;
  }
  if (tile < 0 || tile > 2) { set_error("conv_h16: tile must be 0, 1 or 2"); return DM_ERR_ARG; }
  a = ConvArgs{};
  a.x1 = d->x; a.x1_pitch = d->x_pitch; a.Cin1 = d->Cin; a.Hin = d->Hin; a.Win = d->Win;
  a.taps = d->taps; a.stride = d->stride; a.upsample = d->upsample;
  a.x2 = d->x2; a.x2_pitch = d->x2_pitch; a.Cin2 = d->Cin2;
  a.w = d->w; a.K = d->K;
  a.y = d->y; a.y_pitch = d->y_pitch; a.Cout = d->Cout; a.B = d->B; a.Hout = d->Hout; a.Wout = d->Wout;
  a.bias = d->bias; a.rowvec = d->rowvec; a.rowvec_pitch = d->rowvec_pitch;
  a.res = d->res; a.res_pitch = d->res_pitch;
  a.tile = tile;
  a.pro_scale = d->pro_scale; a.pro_shift = d->pro_shift; a.pro_nosilu = d->pro_nosilu;
  a.ksplit = d->ksplit;
  a.ws = d->w_split; a.ws_np = DM_SPLIT_FP16X2;
  a.range_flag = d->range_flag;
  a.h16 = 1;
  a.h16_a1 = reinterpret_cast<const _Float16*>(image);
  if (a.B > 0 && a.Hin > 0 && a.Win > 0 && a.Cin1 > 0 && a.Cin2 > 0) {
    const size_t n1 = ((size_t)a.B * a.Hin * a.Win * a.Cin1 * 2 + 15) & ~(size_t)15;
    a.h16_a2 = reinterpret_cast<const _Float16*>(reinterpret_cast<const char*>(image) + n1);
  }
  if (a.Cout > 0 && a.K > 0) a.ws_rowscale = split_conv_rowscale(a.ws, 1, a.Cout, a.K);
  return DM_OK;
}

static int h16_sync(int rc, void* stream) {
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == DM_OK) { dm::set_error("sync"); return DM_ERR_HIP; }
  return rc;
}

extern "C" int dm_debug_conv_h16_image(const dm_conv_desc* d, void* image, void* stream) {
  dm::ConvArgs a;
  if (const int rc = h16_desc(d, image, 0, a)) return rc;
  if ((reinterpret_cast<uintptr_t>(image) & 15) != 0 || a.Cin1 % 8 != 0 || a.Cin2 % 8 != 0) {
    dm::set_error("conv_h16_image: 16-byte aligned planes of C % 8 == 0 channels");
    return DM_ERR_UNSUPPORTED;
  }
  return h16_sync(dm::conv_h16_image(a, const_cast<_Float16*>(a.h16_a1), const_cast<_Float16*>(a.h16_a2),
                                     (hipStream_t)stream), stream);
}

extern "C" int dm_debug_conv_h16_gn(const dm_conv_desc* d, void* image, int tile, int G, void* part, void* stream) {
  dm::ConvArgs a;
  if (const int rc = h16_desc(d, image, tile, a)) return rc;
  if (part) {
    a.gn_part = (double2*)part;
    a.gn_G = G;
  }
  if (!dm::conv_h16_ok(a)) {
    dm::set_error("conv_h16: conv_h16_ok refuses the conv (shape, tile form, alignment or GroupNorm groups)");
    return DM_ERR_UNSUPPORTED;
  }
  int rc = dm::conv_h16_image(a, const_cast<_Float16*>(a.h16_a1), const_cast<_Float16*>(a.h16_a2), (hipStream_t)stream);
  if (rc == DM_OK) rc = dm::conv2d_h16(a, (hipStream_t)stream);
  return h16_sync(rc, stream);
}

extern "C" int dm_debug_conv_h16(const dm_conv_desc* d, void* image, int tile, void* stream) {
  return dm_debug_conv_h16_gn(d, image, tile, 0, nullptr, stream);
}
