// Nearest-2x upsample + 3x3 conv (models/modules.py:62-65: Upsample) as a sub-pixel convolution along y and a
// Winograd-style F(2,3) along x, on the fp16x2 split matrix cores of conv_k32.hip / conv_wino.hip.
//
// On a nearest-upsampled row two of a 3-tap filter's taps read the same low-res pixel, so of the four F(2,3) planes
// one vanishes. Along x, for low-res pixel j and the tap-row weights g = (g0, g1, g2):
//   V0 = x[j-1] - x[j]      V1 = x[j]              V2 = x[j+1] - x[j]     (x = 0 outside the map)
//   U0 = g0                 U1 = g0 + g1 + g2      U2 = g2
//   m_b = sum over (channel, tap row) of V_b U_b,   out[2j] = m0 + m1,   out[2j+1] = m1 + m2.
// Along y the sum stays direct in the sub-pixel form: output row 2i takes low-res rows i - 1 and i with the weights
// w_y0 and w_y1 + w_y2, output row 2i + 1 rows i and i + 1 with w_y0 + w_y1 and w_y2. That is 2 py x 3 planes x 2 tap
// rows = 12 products per low-res pixel and (cin, cout) pair where the four 4-tap sub-pixel convs (conv_k32) take 16.
// The six U matrices (py, b), K = 2 Cin each in chunk-major order [chunk][tap row][32], are formed once in float64
// from the torch weight (subwino_pack_kernel) and split like every other weight (split_conv_weights, nmat 6, ntap 2:
// one power-of-two row scale per output channel over all six, since the output transform adds planes). V is formed
// in fp32 in the loader (one rounding per difference) and split hi / lo; the output transform is fp32.
//
// Block: 512 threads, persistent over the tiles of one image (four 4 x 4 images): a tile is 64 low-res pixels (256
// output pixels) x 128 output channels. Wave w holds the 16-column eighth w of the tile with all six (py, b) planes x
// 4 M-tiles of 16 low-res pixels: 24 accumulator tiles (96 registers), so the output transform is register-local.
// Per 32-channel chunk a wave walks 12 steps (b, row offset r in {-1, 0, +1}, the (py, tap row) pairs that read row
// offset r: one for r = -1 / +1, two for r = 0), each 4 M-tiles x 3 MFMAs (a1 w0 + a0 w1 + a0 w0): 144 MFMAs per wave,
// 1152 per tile and chunk, the count of conv_wino's 128-pixel tile.
// LDS: per chunk the three V planes, [b][patch pixel rows][piece][4 k-groups][8] fp16 with conv_k32's 160-B row pitch
// and conv_wino's k-group swizzle, double buffered, one barrier per chunk. B: raw buffer loads from the U images into
// a register ring of 6 steps (48 registers), the wave-uniform part of each address in the scalar offset.
// Loader: lane = (patch pixel, 4-channel quad); the x neighbours by DPP row shifts (bound_ctrl zeroes at the row's
// ends; maps narrower than the 16-lane row select their own edges).
// Epilogue: (m0 + m1, m1 + m2) x row scale + bias, 16-B stores to the 2 x 2 output pixels of each low-res pixel
// (pitched: the output can be a concat slice), the consumer's GroupNorm partials per (parity, 64 low-res pixels) --
// the cover StagedEpilogue::sub emits -- or per image for the 4 x 4 maps.
#include <cstdlib>
#include <string>

#include "dm_common.h"
#include "dm_kernels.h"
#include "mfma_tile.h"
#include "split16.h"

namespace dm {

namespace {

#define DM_SW_INL __attribute__((always_inline))

constexpr int kSC = 32;                      // input channels per chunk (K of one MFMA step)
constexpr int kSRowH = 80;                   // LDS row pitch in fp16 (160 B)
constexpr int kSNR = 96;                     // patch pixel rows per plane at most: 6 x 16, 10 x 8, 4 x 6 x 4
constexpr int kSBuf = 3 * kSNR * kSRowH;     // fp16 per patch buffer (46080 B)
constexpr int kSD = 6;                       // B ring depth in steps (12 steps per chunk: slots are compile-time)
constexpr int kSSteps = 12;

// the k-group's low bit XORed with bit 2 of the pixel row (conv_wino.hip wswz): 16 consecutive rows from any base
// that is a multiple of 4 read conflict-free
__device__ __forceinline__ int sswz(int r) { return (r >> 2) & 1; }

// DPP row shift by one lane, 0 where the source lane is outside the 16-lane row (bound_ctrl)
__device__ __forceinline__ float sw_shr(float v) {  // from lane - 1
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xF, 0xF, true));
}
__device__ __forceinline__ float sw_shl(float v) {  // from lane + 1
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x101, 0xF, 0xF, true));
}

// W: the low-res map's width -- 16 (tiles of 4 rows), 8 (one 8 x 8 image per tile) or 4 (four 4 x 4 images per tile).
// PROM: input prologue, 0 (none) only.
template <int W, int PROM>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) conv_subwino_kernel(ConvArgs a) {
  static_assert(PROM == 0, "no prologue variant");
  constexpr int IMGS = W == 4 ? 4 : 1, RIMG = 64 / W / IMGS, PRI = RIMG + 2;
  constexpr int PR = IMGS * PRI, NR = PR * W;   // patch rows, patch pixel rows (LDS rows) per plane
  static_assert(NR <= kSNR, "patch plane");
  constexpr int NSET = NR * 8 / 64;             // loader sets of 64 (pixel, quad) units: 12 (W 16, 4) / 10 (W 8)
  static_assert(NSET * 64 == NR * 8 && NSET > 8 && NSET <= 16, "loader sets");
  constexpr int IROW = W == 4 ? 24 : 16;        // LDS rows from one M-tile to the next
  __shared__ __attribute__((aligned(16))) _Float16 patch[2 * kSBuf];
  __shared__ double gxr[4 * 32 * 2];            // GroupNorm: [parity / image][wave][q] {sum, sum of squares}

  const int Hl = a.Hin, HWl = Hl * W, Ho = a.Hout, Wo = a.Wout;
  const int N = a.Cout, nN = N / 128;
  const int MT = IMGS * HWl / 64;               // row tiles of the image group
  const int groups = ceil_div(a.B, IMGS);
  const int parts = (int)gridDim.x / groups;
  const int g0 = (int)blockIdx.x / parts, part = (int)blockIdx.x - g0 * parts;
  const int b0 = g0 * IMGS;
  const int tpb = MT * nN / parts;
  const int t_first = part * tpb, t_end = t_first + tpb;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int l16 = lane & 15, q = lane >> 4;
  const int nch = a.Cin1 / kSC;

  // ---- loader: set s = wave and, for the first NSET - 8 waves, 8 + wave; set s = 16-row group s / 2, channel quads
  // 4 (s & 1) + lane / 16
  const bool has2 = wave_u < NSET - 8;
  int lR[2], lq[2], lcol[2], limg[2], lpr[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int s_ = k ? 8 + (has2 ? wave_u : 0) : wave_u;
    const int G = s_ >> 1;
    lq[k] = 4 * (s_ & 1) + q;
    lR[k] = 16 * G + l16;
    if (W == 16) {
      lpr[k] = G; lcol[k] = l16; limg[k] = 0;
    } else if (W == 8) {
      lpr[k] = 2 * G + (l16 >> 3); lcol[k] = l16 & 7; limg[k] = 0;
    } else {
      const int p = 4 * G + (l16 >> 2);
      limg[k] = p / PRI; lpr[k] = p - limg[k] * PRI; lcol[k] = l16 & 3;
    }
  }
  // B (the U images) by raw buffer loads: the lane's column 16 (wave & 1) + l16 of its 32-column group and k-group
  // q (lane group q & 1 of the 16-slice; k-groups 2, 3: the chunk's second 16-slice, 2 slices on) in voffset
  const int ngrp = ceil_div(N, 32);
  const int sl = ngrp * 1024;         // fp16 per 16-deep slice of a U image
  const int nsl = a.Cin1 / 8;         // slices per U matrix (K = 2 Cin1)
  const __amdgpu_buffer_rsrc_t wrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.subwino_ws), 0, 0x7FFFFFFF, 0x00020000);
  const int vb = ((q & 1) * 32 + 16 * (wave & 1) + l16) * 16 + (q >> 1) * 2 * sl * 2;

  // ---- per-tile state
  int mt = 0, n0 = 0, wcol = 0;
  const float* pp[2] = {nullptr, nullptr};
  auto set_tile = [&](int tile) DM_SW_INL {
    mt = tile % MT;
    n0 = (tile / MT) * 128;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int bi = b0 + limg[k];
      const int iy = (W == 16 ? mt * RIMG : 0) - 1 + lpr[k];
      const bool ok = iy >= 0 && iy < Hl && bi < a.B;
      pp[k] = ok ? a.x1 + ((size_t)(bi * Hl + iy) * W + lcol[k]) * a.x1_pitch + 4 * lq[k] : kZeroPage + 4 * lq[k];
    }
    wcol = __builtin_amdgcn_readfirstlane(((n0 + 16 * wave_u) >> 5) * 1024 * 2);
  };

  f4 rw[2];
  auto load_raw = [&](int c) DM_SW_INL {
    rw[0] = *reinterpret_cast<const f4*>(pp[0] + c * kSC);
    if (has2) rw[1] = *reinterpret_cast<const f4*>(pp[1] + c * kSC);
  };
  // set k's 4 channels of one pixel: V0 = x[j-1] - x[j], V1 = x[j], V2 = x[j+1] - x[j], split hi / lo, into buffer buf.
  // A V beyond fp16's range splits into an infinite piece, which every product carries into the accumulators: the
  // epilogue's finiteness check raises the range flag.
  auto finish_set = [&](int buf, int k) DM_SW_INL {
    const f4 e = rw[k];
    f4 vv[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float xm = sw_shr(e[j]), xp = sw_shl(e[j]);
      if (W < 16) {  // several map rows per DPP row: their boundaries are map edges too
        xm = lcol[k] == 0 ? 0.f : xm;
        xp = lcol[k] == W - 1 ? 0.f : xp;
      }
      vv[0][j] = xm - e[j];
      vv[1][j] = e[j];
      vv[2][j] = xp - e[j];
    }
    _Float16* dst = patch + buf * kSBuf + lR[k] * kSRowH + 8 * ((lq[k] >> 1) ^ sswz(lR[k])) + 4 * (lq[k] & 1);
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      f16x4 hi, lo;  // x = hi + lo, lo = fp16(x - hi) (the difference exact, one rounding to fp16)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        hi[j] = (_Float16)vv[v][j];
        lo[j] = (_Float16)(vv[v][j] - (float)hi[j]);
      }
      *reinterpret_cast<f16x4*>(dst + v * NR * kSRowH) = hi;
      *reinterpret_cast<f16x4*>(dst + v * NR * kSRowH + 32) = lo;
    }
  };
  auto finish = [&](int buf) DM_SW_INL {
    finish_set(buf, 0);
    if (has2) finish_set(buf, 1);
  };

  // ---- B ring: step s of chunk c = (b = s / 4, py = (s >> 1) & 1, tap row ty = s & 1): matrix 3 py + b, 16-slice
  // 4 c + ty (+ 2 for k-groups 2, 3)
  f16x8 bq[kSD][2];
  auto load_b = [&](f16x8 (&dst)[2], int c, int s) DM_SW_INL {
    const int mat = 3 * ((s >> 1) & 1) + (s >> 2);
    const int so = __builtin_amdgcn_readfirstlane(wcol + ((mat * nsl + 4 * c + (s & 1)) * sl) * 2);
#pragma unroll
    for (int p = 0; p < 2; ++p)
      dst[p] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, vb + p * 1024, so, 0));
  };

  // A fragment i of row offset r, plane b: LDS rows IROW i + (1 + r) W + l16 (contiguous: a 16-pixel M-tile is whole
  // map rows of one image); the swizzle bit of row C + l16 is that of l16, flipped where C / 4 is odd
  const int abase0 = l16 * kSRowH + 8 * (q ^ sswz(l16)), abase1 = l16 * kSRowH + 8 * (q ^ sswz(l16) ^ 1);

  f4 acc[2][3][4];
  for (int tile = t_first; tile < t_end; ++tile) {
    set_tile(tile);
#pragma unroll
    for (int s = 0; s < kSD; ++s) load_b(bq[s], 0, s);
    load_raw(0);
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[py][b][i] = f4{0.f, 0.f, 0.f, 0.f};
    finish(0);
    __syncthreads();

    for (int c = 0; c < nch; ++c) {
      const bool more = c + 1 < nch;
      const int cn = more ? c + 1 : c;
      if (more) load_raw(c + 1);
      const _Float16* Pb = patch + (c & 1) * kSBuf;
      f16x8 av[4][2];
#pragma unroll
      for (int s = 0; s < kSSteps; ++s) {
        const int b = s >> 2, u = s & 3, py = u >> 1;
        const int r = u == 0 ? -1 : u == 3 ? 1 : 0;
        if (u != 2) {  // (u 2 reads the fragments of u 1 again)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int C = IROW * i + (1 + r) * W;
            const _Float16* As = Pb + (b * NR + C) * kSRowH + (((C >> 2) & 1) ? abase1 : abase0);
            av[i][0] = *reinterpret_cast<const f16x8*>(As);
            av[i][1] = *reinterpret_cast<const f16x8*>(As + 32);
          }
        }
        const int slot = s % kSD;
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // (B, A): the transposed tile, lane (l16, q) = couts 4 q .. 4 q + 3 of pixel l16
          acc[py][b][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bq[slot][0], av[i][1], acc[py][b][i], 0, 0, 0);
          acc[py][b][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bq[slot][1], av[i][0], acc[py][b][i], 0, 0, 0);
          acc[py][b][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bq[slot][0], av[i][0], acc[py][b][i], 0, 0, 0);
        }
        // the refill, kSD steps on (past the tile's last chunk: that chunk's again, which nothing uses)
        load_b(bq[slot], s + kSD < kSSteps ? c : cn, (s + kSD) % kSSteps);
        // (pins the refill here: left free, the scheduler sinks each refill to just before its use and the ring
        // hides nothing)
        __builtin_amdgcn_sched_barrier(0);
      }
      if (more) finish((c + 1) & 1);
      __syncthreads();
    }

    // ---- epilogue: output transform, row scale, bias, 16-B stores; GroupNorm partials of the consumer
    const int ncol = n0 + 16 * wave + 4 * q;
    const f4 rs4 = *reinterpret_cast<const f4*>(a.subwino_rowscale + ncol);
    const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
    const f4 bias4 = a.bias ? *reinterpret_cast<const f4*>(a.bias + ncol) : zero4;
    f4 fin = zero4;  // inf / NaN in any m (an operand past fp16's range) makes fin non-finite
    double gs[4], gq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) gs[k] = gq[k] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int bi, iy, ix;
      if (W == 16) {
        bi = b0; iy = mt * RIMG + i; ix = l16;
      } else if (W == 8) {
        bi = b0; iy = 2 * i + (l16 >> 3); ix = l16 & 7;
      } else {
        bi = b0 + i; iy = l16 >> 2; ix = l16 & 3;
      }
      const bool ok = bi < a.B;
#pragma unroll
      for (int py = 0; py < 2; ++py) {
        f4 v[2];
        v[0] = (acc[py][0][i] + acc[py][1][i]) * rs4;
        v[1] = (acc[py][1][i] + acc[py][2][i]) * rs4;
        fin += v[0] + v[1];
        if (a.bias) {
          v[0] = v[0] + bias4;
          v[1] = v[1] + bias4;
        }
        float* dst = a.y + ((size_t)(bi * Ho + 2 * iy + py) * Wo + 2 * ix) * a.y_pitch + ncol;
        if (ok) {
          *reinterpret_cast<f4*>(dst) = v[0];
          *reinterpret_cast<f4*>(dst + a.y_pitch) = v[1];
        }
        if (a.gn_part) {
#pragma unroll
          for (int px = 0; px < 2; ++px) {
            const int k = W == 4 ? i : 2 * py + px;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              gs[k] += (double)v[px][e];
              gq[k] += (double)v[px][e] * v[px][e];
            }
          }
        }
      }
    }
    if (!__builtin_isfinite(fin[0] + fin[1] + fin[2] + fin[3]) && a.range_flag) *a.range_flag = 1;
    if (a.gn_part) {
      // per (parity / image, wave, q): the quad's sums over the wave's 16 pixel lanes, then per GroupNorm group the
      // quads in column order
#pragma unroll
      for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          gs[k] += __shfl_xor(gs[k], o);
          gq[k] += __shfl_xor(gq[k], o);
        }
        if (l16 == 0) {
          gxr[(k * 32 + wave * 4 + q) * 2] = gs[k];
          gxr[(k * 32 + wave * 4 + q) * 2 + 1] = gq[k];
        }
      }
      __syncthreads();
      const int cpg = N / a.gn_G, qpg = cpg / 4, ng = 128 / cpg;
      if (t < 4 * ng) {
        const int k = t / ng, g = t - k * ng;
        double s = 0.0, qq = 0.0;
        for (int j = 0; j < qpg; ++j) {
          s += gxr[(k * 32 + g * qpg + j) * 2];
          qq += gxr[(k * 32 + g * qpg + j) * 2 + 1];
        }
        // W 16 / 8: chunk (parity k, 64 low-res pixels mt) of image b0, StagedEpilogue::sub's cover; W 4: the one
        // chunk of image b0 + k
        const int nchl = W == 4 ? 1 : HWl / 64;
        const int bb = W == 4 ? b0 + k : b0;
        const int ch = W == 4 ? 0 : k * nchl + mt;
        const int nchunk = W == 4 ? 1 : 4 * nchl;
        if (bb < a.B) a.gn_part[((size_t)bb * nchunk + ch) * a.gn_G + n0 / cpg + g] = make_double2(s, qq);
      }
      // (the next tile writes gxr after its chunk barriers)
    }
  }
}

// U per (matrix 3 py + b, output channel, chunk, tap row ty, channel of the chunk) from the torch weight
// [Cout][Cin][3][3]: [6][Cout][2 Cin] in chunk-major order with 2 tap rows, float64 sums rounded once to fp32
__global__ void subwino_pack_kernel(const float* w, int Cout, int Cin, float* out) {
  const int Kp = 2 * Cin;
  const long total = 6L * Cout * Kp;
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= total) return;
  const int k = id % Kp;
  const long r = id / Kp;
  const int co = r % Cout, mat = r / Cout;
  const int py = mat / 3, b = mat - 3 * py;
  const int c = k / (2 * kSC), rem = k - c * 2 * kSC, ty = rem / kSC, ci = c * kSC + (rem - ty * kSC);
  const float* src = w + ((size_t)co * Cin + ci) * 9;
  double g[3];  // the tap row's weights, summed along y
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    const double w0 = src[x], w1 = src[3 + x], w2 = src[6 + x];
    g[x] = py == 0 ? (ty == 0 ? w0 : w1 + w2) : (ty == 0 ? w0 + w1 : w2);
  }
  out[id] = (float)(b == 0 ? g[0] : b == 1 ? g[0] + g[1] + g[2] : g[2]);
}

int g_subwino_ncu = 0;

}  // namespace

bool conv_subwino_shape_ok(const ConvArgs& a) {
  if (!(a.taps == 9 && a.stride == 1 && a.upsample == 2 && a.Cin2 == 0 && a.ksplit <= 1)) return false;
  if (a.Hout != 2 * a.Hin || a.Wout != 2 * a.Win) return false;
  // whole-row tiles of 64 low-res pixels: 16-wide maps in 4-row tiles, 8 x 8 maps, four 4 x 4 maps
  if (!((a.Win == 16 && a.Hin % 4 == 0) || (a.Win == 8 && a.Hin == 8) || (a.Win == 4 && a.Hin == 4))) return false;
  if (a.Cin1 < kSC || a.Cin1 % kSC != 0 || a.K != 4 * a.Cin1 || a.Cout % 128 != 0) return false;
  if (a.pro_scale || a.gin_part || a.res || a.rowvec || a.h16) return false;  // no prologue, bias-only epilogue
  if (a.x1_pitch % 4 != 0 || a.x1_pitch + a.Cin1 > kZeroPageFloats) return false;  // padding rows read the zero page
  if (a.y_pitch % 4 != 0 || a.y_pitch < a.Cout) return false;
  if (a.gn_part) {
    if (a.gn_G <= 0 || a.Cout % a.gn_G != 0) return false;
    const int cpg = a.Cout / a.gn_G;
    if (cpg % 4 != 0 || cpg > 32 || 128 % cpg != 0) return false;
  }
  return true;
}

bool conv_subwino_ok(const ConvArgs& a) {
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  return a.subwino_ws && a.subwino_rowscale && conv_subwino_shape_ok(a) && a.x1 && a.y && al16(a.x1) && al16(a.y) &&
         al16(a.subwino_ws) && (!a.bias || al16(a.bias));
}

size_t subwino_weights_bytes(int Cout, int Cin) { return split_conv_weights_bytes(6, Cout, 2 * Cin, 2); }

const float* subwino_rowscale(const void* ws, int Cout, int Cin) { return split_conv_rowscale(ws, 6, Cout, 2 * Cin); }

int subwino_pack(const float* w, int Cout, int Cin, float* out, hipStream_t st) {
  DM_REQUIRE(w && out && Cout > 0 && Cin > 0 && Cin % kSC == 0, "sub-pixel Winograd weights: Cin must be a multiple of 32");
  const long n = 6L * Cout * 2 * Cin;
  hipLaunchKernelGGL(subwino_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, Cout, Cin, out);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

int subwino_weights(const float* w, int Cout, int Cin, void* out, hipStream_t st) {
  DM_REQUIRE(w && out && Cout > 0 && Cin > 0 && Cin % kSC == 0, "sub-pixel Winograd weights: Cin must be a multiple of 32");
  const long n = 6L * Cout * 2 * Cin;
  float* tmp = nullptr;  // plan-build time only: synchronous
  DM_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&tmp), n * sizeof(float)));
  int rc = subwino_pack(w, Cout, Cin, tmp, st);
  if (rc == DM_OK) rc = split_conv_weights(tmp, 6, Cout, 2 * Cin, Cin, 2, 2, out, st);
  if (hipStreamSynchronize(st) != hipSuccess && rc == DM_OK) rc = DM_ERR_HIP;
  (void)hipFree(tmp);
  if (rc == DM_ERR_HIP) set_error("sub-pixel Winograd weights: kernel launch failed");
  return rc;
}

std::string conv_subwino_label(const ConvArgs& a) {
  return std::string("conv_subwino_kernel<") + std::to_string(a.Win) + ",0>";
}

int conv2d_subwino(const ConvArgs& a, hipStream_t st) {
  DM_REQUIRE(conv_subwino_ok(a), "conv: shape not supported by the sub-pixel Winograd kernel");
  // persistent blocks over one image group's tiles: parts per group = the smallest divisor of its tile count that
  // gives at least one block per CU (conv_wino.hip)
  if (!g_subwino_ncu) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&g_subwino_ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        g_subwino_ncu <= 0)
      g_subwino_ncu = 256;
  }
  const int imgs = a.Win == 4 ? 4 : 1, groups = ceil_div(a.B, imgs);
  const int tpi = (imgs * a.Hin * a.Win / 64) * (a.Cout / 128);
  int parts = tpi;
  for (int p = 1; p <= tpi; ++p)
    if (tpi % p == 0 && (long)groups * p >= g_subwino_ncu) {
      parts = p;
      break;
    }
  const int blocks = groups * parts;
#define DM_SUBWINO_LAUNCH(W_)                                                                    \
  if (a.Win == W_) {                                                                             \
    hipLaunchKernelGGL((conv_subwino_kernel<W_, 0>), dim3(blocks), dim3(512), 0, st, a);         \
    note_launch("conv_subwino_kernel<" #W_ ",0>");                                               \
  }
  DM_SUBWINO_LAUNCH(16) DM_SUBWINO_LAUNCH(8) DM_SUBWINO_LAUNCH(4)
#undef DM_SUBWINO_LAUNCH
  DM_LAUNCH_CHECK();
  return DM_OK;
}

}  // namespace dm
