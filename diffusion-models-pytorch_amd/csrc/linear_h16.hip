// Static-weight GEMM C = epilogue(A' W'^T) in the half-precision arithmetic DM_MATH_FP16: ONE
// v_mfma_f32_16x16x32_f16 product per MAC (linear_k32.hip spends three on its fp16x2 split), fp32 accumulation --
// the opt-in throughput mode of the DiT / MDT token GEMMs (qkv, proj, fc1, fc2, skip_linear, final layer).
//
// Numerics: a' = fp16_rne(prologue(a) * alpha * 2^ea) comes ONLY as an image, one fp16 plane [M][K] written once per
// GEMM by linear_h16_image / linear_h16_image_cat (the single-plane siblings of linear_presplit_a /
// linear_presplit_cat: the same expressions, so a' is bit for bit piece 0 of the fp16x2 image) or by a producer's
// epilogue (GemmArgs::c_split here: fc1 writes fc2's image). w' = fp16_rne(w * 2^er(row)) is piece 0 of the fp16x2
// fragment image split_conv_weights already holds, read in place: the mode owns no weight copy. acc = sum_k a' w'
// in the MFMA's fp32 accumulator, times 2^-(ea + er) exactly, then linear_k32's fp32 epilogue (bias, residual / gated
// residual, SiLU / GELU-tanh, the q / k / v operand planes -- hi + lo pieces of the fp32 accumulator: attention stays
// fp16x2). |a * 2^ea| > 65504 raises range_flag at the image pass (and at the c_split / plane epilogues).
//
// Block 128 x 128, four waves of 128 x 32 (8 x 2 tiles of 16 x 16), as linear_k32: per K = 32 step a wave issues 8
// ds_read_b128 (4 LDS cycles each: 128 LDS cycles per CU-step of four waves) against 16 MFMAs (~16 cycles each: 256),
// so the LDS array is at half its rate where one product per fragment pair stands in for three. K is staged 64
// channels at a time (two steps per barrier), double-buffered in LDS as rows of 64 fp16 with a 160-B pitch (10 16-B
// slots: row r of a 16-row fragment read lands on slot 10 r + q mod 16 -- even for the lanes of k-group q, odd for
// those of q + 1, all 16 of a ds_read_b128 lane group distinct). A rows come as whole 128-B cache lines (8 threads
// per row span), two stages ahead in registers; B fragments from L2 into a 2-deep register ring. No split-K tail:
// a tile's sum has one order whatever the batch, so a row's result is bit-identical at every batch size.
#include "dm_common.h"
#include "dm_kernels.h"
#include "mfma_tile.h"
#include "split16.h"

namespace dm {

namespace {

constexpr int kHP = 80;    // LDS row pitch in fp16 (160 B) of one 64-channel stage
constexpr int kHBM = 128;  // block rows
constexpr int kHBN = 128;  // block columns
constexpr int kHGM = 4;    // M tiles per group of the tile order

// The attention operand planes from the qkv projection's fp32 accumulator: linear_k32.hip's plane_slab /
// plane_block (the expressions of conv_patch3.hip's attn_plane_epilogue), kept textually the same here so the two
// arithmetics hand the flash kernel planes of one format. q * alpha * 2^ea and k * b_scale * 2^eb as
// [B][heads][2][L][Dh], v * 2^ev transposed as [B][heads][2][Dh][L]; plane 0 = fp16(x), plane 1 = fp16(x - plane 0).
__device__ __forceinline__ void h16_locate(const GemmArgs& g, int col, int& part, int& h, int& d) {
  const int Dh = g.ap_Dh, C = g.ap_heads * Dh;
  if (g.ap_vonly) {
    part = 2;
    h = col / Dh;
    d = col - h * Dh;
  } else if (g.ap_legacy) {
    h = col / (3 * Dh);
    part = (col - h * 3 * Dh) / Dh;
    d = col - h * 3 * Dh - part * Dh;
  } else {
    part = col / C;
    h = (col - part * C) / Dh;
    d = col - part * C - h * Dh;
  }
}

__device__ __forceinline__ void h16_split8(const GemmArgs& g, int part, const float (&x)[8], f16x8& hi, f16x8& lo,
                                           bool& bad) {
  const float scale = part == 0 ? g.ap_alpha : part == 1 ? g.ap_bscale : 1.f;
  const bool use_scale = part == 0 ? g.ap_alpha != 1.0f : part == 1 && g.ap_bscale != 0.0f && g.ap_bscale != 1.0f;
  const float pw = ldexpf(1.f, part == 0 ? g.ap_ea : part == 1 ? g.ap_eb : g.ap_ev);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float y = (use_scale ? x[e] * scale : x[e]) * pw;
    const _Float16 h0 = (_Float16)y;
    hi[e] = h0;
    lo[e] = (_Float16)(y - (float)h0);
    bad |= fabsf(y) > 65504.f;
  }
}

// one 32 x WN slab of a wave (any L with L % 8 == 0; 8-column groups located one by one: Dh % 8 == 0)
template <int WN>
__device__ __forceinline__ void h16_plane_slab(const GemmArgs& g, const float* st, int EP, int row0, int col0,
                                               int lane, bool& bad) {
  if (col0 >= g.N) return;
  const int Dh = g.ap_Dh;
  int part, h0, d0;
  h16_locate(g, col0, part, h0, d0);
  const size_t plane = (size_t)g.ap_L * Dh;
  const float* bias = g.bias ? g.bias + col0 : nullptr;
  if (part < 2) {  // q / k: 8 consecutive d of one token per item
    _Float16* dst = part == 0 ? g.ap_q : g.ap_k;
    constexpr int G8 = WN / 8;
    for (int it = lane; it < 32 * G8; it += 64) {
      const int row = it / G8, c8 = it - row * G8;
      const int m = row0 + row;
      if (m >= g.M) continue;
      int pt, h, d;
      h16_locate(g, col0 + 8 * c8, pt, h, d);
      float x[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = st[row * EP + 8 * c8 + e] + (bias ? bias[8 * c8 + e] : 0.f);
      f16x8 hi, lo;
      h16_split8(g, part, x, hi, lo, bad);
      const int b = m / g.ap_L, tok = m - b * g.ap_L;
      _Float16* p = dst + ((size_t)b * g.ap_heads + h) * 2 * plane + (size_t)tok * Dh + d;
      *reinterpret_cast<f16x8*>(p) = hi;
      *reinterpret_cast<f16x8*>(p + plane) = lo;
    }
  } else {  // v: 8 consecutive tokens of one d per item
    for (int it = lane; it < WN * 4; it += 64) {
      const int col = it % WN, r8 = it / WN;
      const int m = row0 + 8 * r8;  // tokens m .. m + 7 lie in one image (L % 8 == 0)
      if (m >= g.M) continue;
      int pt, h, d;
      h16_locate(g, col0 + col, pt, h, d);
      float x[8];
      const float bc = bias ? bias[col] : 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = st[(8 * r8 + e) * EP + col] + bc;
      f16x8 hi, lo;
      h16_split8(g, 2, x, hi, lo, bad);
      const int b = m / g.ap_L, tok = m - b * g.ap_L;
      _Float16* p = g.ap_v + ((size_t)b * g.ap_heads + h) * 2 * plane + (size_t)d * g.ap_L + tok;
      *reinterpret_cast<f16x8*>(p) = hi;
      *reinterpret_cast<f16x8*>(p + plane) = lo;
    }
  }
}

// the whole 128 x 128 block tile (L % 128 == 0: its rows lie in one image), 256 contiguous bytes per 16 threads
__device__ __forceinline__ void h16_plane_block(const GemmArgs& g, const float* tile, int TP, int m0, int n0, int t,
                                                bool& bad) {
  const int Dh = g.ap_Dh;
  const size_t plane = (size_t)g.ap_L * Dh;
  const int b = m0 / g.ap_L, tok0 = m0 - b * g.ap_L;
  const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  {  // q / k: item (row, 8-column group), 16 groups per row; a thread keeps its column group
    const int c8 = t & 15, col = n0 + 8 * c8;
    int part, h, d;
    h16_locate(g, min(col, g.N - 1), part, h, d);
    if (col < g.N && part < 2) {
      const f4 b0 = g.bias ? *reinterpret_cast<const f4*>(g.bias + col) : zero4;
      const f4 b1 = g.bias ? *reinterpret_cast<const f4*>(g.bias + col + 4) : zero4;
      _Float16* base = (part == 0 ? g.ap_q : g.ap_k) + ((size_t)b * g.ap_heads + h) * 2 * plane + (size_t)tok0 * Dh + d;
#pragma unroll 2
      for (int row = t >> 4; row < 128; row += 16) {
        if (m0 + row >= g.M) break;
        const f4 v0 = *reinterpret_cast<const f4*>(tile + row * TP + 8 * c8) + b0;
        const f4 v1 = *reinterpret_cast<const f4*>(tile + row * TP + 8 * c8 + 4) + b1;
        const float x[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        f16x8 hi, lo;
        h16_split8(g, part, x, hi, lo, bad);
        _Float16* p = base + (size_t)row * Dh;
        *reinterpret_cast<f16x8*>(p) = hi;
        *reinterpret_cast<f16x8*>(p + plane) = lo;
      }
    }
  }
  // v: item (4-column group, 8-token group), 16 token groups per column group
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int it = t + 256 * k;
    const int r8 = it & 15, cq = it >> 4, col = n0 + 4 * cq;
    if (col >= g.N || m0 + 8 * r8 >= g.M) continue;  // M % 8 == 0 (L % 128 == 0)
    int part, h, d;
    h16_locate(g, col, part, h, d);
    if (part != 2) continue;
    const f4 bc = g.bias ? *reinterpret_cast<const f4*>(g.bias + col) : zero4;
    f4 v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = *reinterpret_cast<const f4*>(tile + (8 * r8 + e) * TP + 4 * cq);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float x[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = v[e][c] + bc[c];
      f16x8 hi, lo;
      h16_split8(g, 2, x, hi, lo, bad);
      _Float16* p = g.ap_v + ((size_t)b * g.ap_heads + h) * 2 * plane + (size_t)(d + c) * g.ap_L + tok0 + 8 * r8;
      *reinterpret_cast<f16x8*>(p) = hi;
      *reinterpret_cast<f16x8*>(p + plane) = lo;
    }
  }
}

// linear_h16_image: one thread per 8 consecutive channels of a row: linear_presplit_a's expressions (prologue,
// alpha, 2^ea), rounded once to fp16, at [m][c .. c + 7] of the plane.
template <int PRO>
__global__ void __launch_bounds__(256) h16_image_kernel(GemmArgs g, void* out_) {
  _Float16* out = reinterpret_cast<_Float16*>(out_);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int per_row = g.K / 8;
  if (i >= (long)g.M * per_row) return;
  const int m = (int)(i / per_row), c = (int)(i - (long)m * per_row) * 8;
  const float* a = g.A + (size_t)m * g.lda + c;
  f4 v0 = *reinterpret_cast<const f4*>(a), v1 = *reinterpret_cast<const f4*>(a + 4);
  if (PRO == 1) {
    const size_t o = (size_t)(m / g.pro_rows) * g.K + c;
    const f4 s0 = *reinterpret_cast<const f4*>(g.pro_scale + o), s1 = *reinterpret_cast<const f4*>(g.pro_scale + o + 4);
    const f4 h0 = *reinterpret_cast<const f4*>(g.pro_shift + o), h1 = *reinterpret_cast<const f4*>(g.pro_shift + o + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v0[e] = v0[e] * s0[e] + h0[e];
      v1[e] = v1[e] * s1[e] + h1[e];
    }
  } else if (PRO == 2) {
    const float2 lns = g.ln_stats[m];
    const size_t o = (size_t)(m / g.ln_rows) * g.ln_pitch + c;
    const f4 s0 = *reinterpret_cast<const f4*>(g.ln_scale + o), s1 = *reinterpret_cast<const f4*>(g.ln_scale + o + 4);
    const f4 h0 = *reinterpret_cast<const f4*>(g.ln_shift + o), h1 = *reinterpret_cast<const f4*>(g.ln_shift + o + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v0[e] = ((v0[e] - lns.x) * lns.y) * (1.0f + s0[e]) + h0[e];
      v1[e] = ((v1[e] - lns.x) * lns.y) * (1.0f + s1[e]) + h1[e];
    }
  }
  if (g.alpha != 1.0f) {
    v0 = v0 * g.alpha;
    v1 = v1 * g.alpha;
  }
  const float apow = ldexpf(1.f, g.split_ea);
  v0 = v0 * apow;
  v1 = v1 * apow;
  f16x8 h;
  float mx = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = (_Float16)v0[e];
    h[4 + e] = (_Float16)v1[e];
    mx = fmaxf(mx, fmaxf(fabsf(v0[e]), fabsf(v1[e])));
  }
  *reinterpret_cast<f16x8*>(out + (size_t)m * g.K + c) = h;
  if (mx > 65504.f && g.range_flag) *g.range_flag = 1;
}

// linear_h16_image_cat: the image of [x | skip] (two [M][D] matrices side by side, D % 8 == 0), no prologue
__global__ void __launch_bounds__(256) h16_image_cat_kernel(const float* __restrict__ x, const float* __restrict__ skip,
                                                            long M, int D, int ea, void* out_, int* range_flag) {
  _Float16* out = reinterpret_cast<_Float16*>(out_);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int K = 2 * D, per_row = K / 8;
  if (i >= M * per_row) return;
  const long m = i / per_row;
  const int c = (int)(i - m * per_row) * 8;
  const float* a = c < D ? x + (size_t)m * D + c : skip + (size_t)m * D + (c - D);
  const float apow = ldexpf(1.f, ea);
  const f4 v0 = *reinterpret_cast<const f4*>(a) * apow, v1 = *reinterpret_cast<const f4*>(a + 4) * apow;
  f16x8 h;
  float mx = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = (_Float16)v0[e];
    h[4 + e] = (_Float16)v1[e];
    mx = fmaxf(mx, fmaxf(fabsf(v0[e]), fabsf(v1[e])));
  }
  *reinterpret_cast<f16x8*>(out + (size_t)m * K + c) = h;
  if (mx > 65504.f && range_flag) *range_flag = 1;
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) linear_h16_kernel(GemmArgs g) {
  constexpr int WM = 128, WN = 32, NW = 4;
  constexpr int BM = kHBM, BN = kHBN, TM = WM / 16, TN = WN / 16, WD = 2, NWN = BN / WN;
  static_assert((BM / WM) * NWN == NW, "one wave tile per wave");
  constexpr int NT = NW * 64, RS = NT / 8, NU = BM / RS;  // A loader: row step, rows per thread
  constexpr int STAGE = BM * kHP;                         // fp16 elements per buffer
  constexpr int TP = BN + 4;                              // the plane epilogue's block tile pitch (fp32)
  constexpr int LDS_H = 2 * STAGE > BM * TP * 2 ? 2 * STAGE : BM * TP * 2;
  __shared__ __attribute__((aligned(16))) _Float16 abuf[LDS_H];

  const int M = g.M, N = g.N, K = g.K;
  // grouped tile order (linear_k32's): consecutive tiles of one XCD sweep all N tiles of kHGM M tiles
  const int nN = ceil_div(N, BN), nM = ceil_div(M, BM);
  const int bid = xcd_remap_p((int)blockIdx.x, (int)gridDim.x);
  const int tgrp = bid / (kHGM * nN), gm0 = tgrp * kHGM, gsz = min(kHGM, nM - gm0);
  const int r = bid - tgrp * (kHGM * nN);
  const int nt = r / gsz, mt = gm0 + (r - nt * gsz);
  const int m0 = mt * BM, n0 = nt * BN;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wn = wave;
  const int l16 = lane & 15, q = lane >> 4;

  // A loader: 16-B slot a3s (8 fp16 of one k-group) of the stage's 128-B row span in tile rows a3r + 32 u
  const int a3s = t & 7, a3r = t >> 3;
  const f4* asp = reinterpret_cast<const f4*>(g.as) + a3s;
  const size_t apitch = (size_t)K / 8;  // f4 per image row
  f4 ra[2][NU];                         // A rows of two stages in flight (stage s in ra[s & 1])
  auto load_a = [&](f4 (&dst)[NU], int st) {
    if (m0 + BM <= M) {
      const f4* b0 = asp + (size_t)(m0 + a3r) * apitch + 8 * st;
#pragma unroll
      for (int u = 0; u < NU; ++u) dst[u] = b0[(size_t)(RS * u) * apitch];
    } else {  // the last, partial tile clamps each row (rows >= M are never stored)
#pragma unroll
      for (int u = 0; u < NU; ++u) dst[u] = asp[(size_t)min(m0 + a3r + RS * u, M - 1) * apitch + 8 * st];
    }
  };
  auto store_a = [&](const f4 (&src)[NU], int buf) {
    _Float16* d3 = abuf + buf * STAGE + a3r * kHP + a3s * 8;
#pragma unroll
    for (int u = 0; u < NU; ++u) *reinterpret_cast<f4*>(d3 + RS * u * kHP) = src[u];
  };

  // B: piece 0 of the fragment images [16-slice][32-col group][piece][lane group][32][8]; K32 step kk reads
  // 16-slices 2 kk + (q >> 1), lane group q & 1
  const int ngrp = ceil_div(N, 32);
  const size_t sl = (size_t)ngrp * 1024;
  const _Float16* wbase[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * WN + j * 16 + l16;
    const int grp = min(col >> 5, ngrp - 1);
    wbase[j] = reinterpret_cast<const _Float16*>(g.ws) + (size_t)(q >> 1) * sl + (size_t)grp * 1024 +
               ((q & 1) * 32 + (col & 31)) * 8;
  }
  f16x8 bq[WD][TN];
  auto load_b = [&](f16x8 (&dst)[TN], int kk) {
#pragma unroll
    for (int j = 0; j < TN; ++j) dst[j] = *reinterpret_cast<const f16x8*>(wbase[j] + (size_t)(2 * kk) * sl);
  };

  f4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  auto compute = [&](int buf, int s, const f16x8 (&bv)[TN]) {
    const _Float16* As = abuf + buf * STAGE + l16 * kHP + s * 32 + q * 8;
    f16x8 av[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) av[i] = *reinterpret_cast<const f16x8*>(As + i * 16 * kHP);
    // all of the step's fragment reads issued before its first MFMA (they return in order)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[i], bv[j], acc[i][j], 0, 0, 0);
  };

  const int nst = K / 64, nkk = 2 * nst;
#pragma unroll
  for (int d = 0; d < WD; ++d) load_b(bq[d], min(d, nkk - 1));
  load_a(ra[0], 0);
  load_a(ra[1], min(1, nst - 1));
  store_a(ra[0], 0);
  __syncthreads();
  // One barrier per stage. Stage st: the A rows of stage st + 2 are loaded (into the registers stage st's rows
  // left) before step 0; after step 1 stage st + 1 goes into the other buffer.
  auto stage = [&](int st, f4 (&cur)[NU], f4 (&nxt)[NU]) {
    load_a(cur, min(st + 2, nst - 1));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int kk = 2 * st + s;
      compute(st & 1, s, bq[s]);
      load_b(bq[s], min(kk + WD, nkk - 1));
      __builtin_amdgcn_sched_barrier(0);
    }
    store_a(nxt, (st + 1) & 1);
    __syncthreads();
  };
  for (int st = 0; st < nst; st += 2) {
    stage(st, ra[0], ra[1]);
    if (st + 1 < nst) stage(st + 1, ra[1], ra[0]);
  }

  // ---- epilogue (linear_k32's): per 32-row slab of the wave's rows, acc * rowscale * 2^-ea to LDS ([32][36] fp32),
  // then 4 consecutive columns per lane: bias, residual / gated residual, activation, 16-B store
  bool bad = false;
  constexpr int EP = WN + 4, LPR = WN / 4, RPI = 64 / LPR;
  float* stg = reinterpret_cast<float*>(abuf) + wave * 32 * EP;
  const float unscale = ldexpf(1.f, -g.split_ea);
  float cs[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) cs[j] = g.ws_rowscale[min(n0 + wn * WN + j * 16 + l16, N - 1)] * unscale;
  const int c4 = lane % LPR, rsub = lane / LPR;
  const int ncol = n0 + wn * WN + 4 * c4;
  const bool c_ok = ncol < N;  // N % 4 == 0
  const int nc = c_ok ? ncol : 0;
  const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const f4 bias4 = g.bias ? *reinterpret_cast<const f4*>(g.bias + nc) : zero4;
  if (g.ap_q && g.ap_L % BM == 0) {  // attention planes from the whole block tile (the loop ended on a barrier)
    float* tile = reinterpret_cast<float*>(abuf);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) tile[(16 * i + 4 * q + rr) * TP + wn * WN + 16 * j + l16] = acc[i][j][rr] * cs[j];
    __syncthreads();
    h16_plane_block(g, tile, TP, m0, n0, t, bad);
    if (bad && g.range_flag) *g.range_flag = 1;
    return;
  }
#pragma unroll
  for (int h = 0; h < WM / 32; ++h) {
#pragma unroll
    for (int i = 2 * h; i < 2 * h + 2; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) stg[((i - 2 * h) * 16 + 4 * q + rr) * EP + j * 16 + l16] = acc[i][j][rr] * cs[j];
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's slab is visible to its reads
    __builtin_amdgcn_wave_barrier();
    const int row0 = m0 + 32 * h;
    if (g.ap_q) {
      h16_plane_slab<WN>(g, stg, EP, row0, n0 + wn * WN, lane, bad);
      __builtin_amdgcn_wave_barrier();
      continue;
    }
    f4 rs4[32 / RPI], gt4[32 / RPI];
    if (g.res) {
#pragma unroll
      for (int it = 0; it < 32 / RPI; ++it) {
        const int m = min(row0 + it * RPI + rsub, M - 1);
        rs4[it] = *reinterpret_cast<const f4*>(g.res + (size_t)(g.res_mod > 0 ? m % g.res_mod : m) * g.ld_res + nc);
        gt4[it] = g.gate ? *reinterpret_cast<const f4*>(g.gate + (size_t)(m / g.gate_rows) * g.gate_pitch + nc) : zero4;
      }
    }
#pragma unroll
    for (int it = 0; it < 32 / RPI; ++it) {
      const int row = it * RPI + rsub;
      const int m = row0 + row;
      f4 v = *reinterpret_cast<const f4*>(stg + row * EP + 4 * c4);
      if (g.bias) v = v + bias4;
      if (g.res) v = g.gate ? rs4[it] + gt4[it] * v : v + rs4[it];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (g.act == 1) v[e] = silu_f(v[e]);
        else if (g.act == 2) v[e] = gelu_tanh_f(v[e]);
      }
      if (g.c_split) {  // the next GEMM's image: linear_h16_image's expressions (no prologue, alpha 1)
        const float cp = ldexpf(1.f, g.c_split_ea);
        f16x4 h0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float y = v[e] * cp;
          h0[e] = (_Float16)y;
          bad |= fabsf(y) > 65504.f;
        }
        if (m < M && c_ok) *reinterpret_cast<f16x4*>(g.c_split + (size_t)m * N + ncol) = h0;
      } else if (m < M && c_ok) {
        *reinterpret_cast<f4*>(g.C + (size_t)m * g.ldc + ncol) = v;
      }
    }
    __builtin_amdgcn_wave_barrier();  // the next slab reuses the region
  }
  if (bad && g.range_flag) *g.range_flag = 1;
}

}  // namespace

// The launch form: the A image in g.as (no prologue left in the descriptor), the fp16x2 fragment image in g.ws.
bool linear_h16_ok(const GemmArgs& g) {
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (!(g.h16 && g.ws && g.ws_rowscale && g.as && al16(g.as) && g.Z1 == 1 && g.Z2 == 1 && !g.b_kn && g.b_scale == 0.0f))
    return false;
  if (g.M <= 0 || g.N <= 0 || g.K <= 0 || g.K % 64 != 0 || g.N % 4 != 0) return false;
  if (g.pro_scale || g.ln_stats || g.gn_part) return false;  // the prologue belongs to the image pass
  if (!g.C && !g.c_split && !g.ap_q) return false;
  if (g.C && (g.ldc % 4 != 0 || g.ldc < g.N || !al16(g.C))) return false;
  if (g.bias && !al16(g.bias)) return false;
  if (g.res && (g.ld_res % 4 != 0 || !al16(g.res))) return false;
  if (g.gate && (!g.res || g.gate_rows <= 0 || g.gate_pitch % 4 != 0 || !al16(g.gate))) return false;
  if (g.c_split && (g.N % 64 != 0 || g.ap_q || !al16(g.c_split))) return false;
  if (g.ap_vonly && (!g.ap_q || g.ap_legacy)) return false;
  if (g.ap_q && (g.ap_Dh % 8 != 0 || g.ap_L % 8 != 0 || (g.ap_heads * g.ap_Dh) % 32 != 0 ||
                 (g.ap_legacy && g.ap_Dh % 32 != 0)))
    return false;
  return true;
}

int linear_h16_image(const GemmArgs& g, _Float16* out, hipStream_t st) {
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  DM_REQUIRE(g.M > 0 && g.K % 64 == 0 && g.lda % 4 == 0 && al16(g.A) && al16(out) && !(g.pro_scale && g.ln_stats),
             "linear_h16_image: K % 64 == 0 and 16-byte aligned rows");
  DM_REQUIRE(!g.pro_scale || (g.pro_shift && g.pro_rows > 0 && al16(g.pro_scale) && al16(g.pro_shift)),
             "linear_h16_image: GroupNorm tables");
  DM_REQUIRE(!g.ln_stats || (g.ln_scale && g.ln_shift && g.ln_rows > 0 && g.ln_pitch % 4 == 0 && al16(g.ln_scale) &&
                             al16(g.ln_shift)),
             "linear_h16_image: LayerNorm tables");
  const long n = (long)g.M * (g.K / 8);
  const long blocks = (n + 255) / 256;
  DM_REQUIRE(blocks < (1L << 31), "linear_h16_image: too many rows");
  if (g.pro_scale)
    hipLaunchKernelGGL(h16_image_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, g, (void*)out);
  else if (g.ln_stats)
    hipLaunchKernelGGL(h16_image_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, st, g, (void*)out);
  else
    hipLaunchKernelGGL(h16_image_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, g, (void*)out);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

int linear_h16_image_cat(const float* x, const float* skip, long M, int D, int ea, _Float16* out, int* range_flag,
                         hipStream_t st) {
  DM_REQUIRE(M > 0 && D > 0 && D % 32 == 0 &&
                 ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(skip) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
             "linear_h16_image_cat: D % 32 == 0 and 16-byte aligned rows");
  const long n = M * (2 * D / 8);
  const long blocks = (n + 255) / 256;
  DM_REQUIRE(blocks < (1L << 31), "linear_h16_image_cat: too many rows");
  hipLaunchKernelGGL(h16_image_cat_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, skip, M, D, ea, (void*)out,
                     range_flag);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

int linear_h16(const GemmArgs& g, hipStream_t st) {
  DM_REQUIRE(linear_h16_ok(g), "linear_h16: needs the fp16 A image, pre-split weights, K % 64 == 0, 16-byte aligned 4-column rows");
  const int tiles = ceil_div(g.M, kHBM) * ceil_div(g.N, kHBN);
  hipLaunchKernelGGL(linear_h16_kernel, dim3(tiles), dim3(256), 0, st, g);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

}  // namespace dm
