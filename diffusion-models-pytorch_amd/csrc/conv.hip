// Implicit-GEMM 2-D convolution on NHWC activations, fp32 MFMA.
//
// Replaces the torch.nn.Conv2d calls of the reference denoisers:
//   3x3 stride 1 pad 1   models/unet.py:16,26,72,118
//   3x3 stride 2 pad 1   models/modules.py:72      (Downsample)
//   3x3 stride 2 over an input padded at the bottom / right only (ConvArgs::s2_pad0)
//                        models/stablediffusion/autoencoder.py:47-66 (the KL encoder's Downsample)
//   nearest-2x + 3x3     models/modules.py:62-65   (Upsample; the 2x image is
//                                                   never materialised)
//   1x1                  models/unet.py:28 (shortcut), modules.py:83-86
//
// GEMM view: out[m][n] = sum_k A[m][k] * W[n][k]
//   m = output pixel (b, oy, ox), n = output channel,
//   k = tap * Cin1 + c over segment 1 (the conv input), then Cin2 more k for
//   an optional segment 2: a 1x1 product of a second NHWC tensor at the output
//   resolution (the ResBlock shortcut conv folded into the second conv's K
//   loop: out = conv2(h) + W_s x + b_s in one pass).
// Epilogue: + bias[n] + rowvec[b][n] (timestep-embedding projection,
// models/unet.py:41) + residual[m][n] (models/unet.py:43), stored through a
// pitched view so outputs can land inside a wider concat buffer.
//
// Loader: every thread owns A_ITERS output pixels for the whole K loop. Per
// tap it derives a source row pointer and a validity bit (zero padding);
// the loads themselves are unconditional (invalid rows read a clamped, valid
// address and are zeroed by a select), so the compiler keeps the next
// K-slice's global loads in flight across the MFMA work of the current one
// instead of draining vmcnt at exec-masked branches.
#include "dm_common.h"
#include "dm_kernels.h"
#include "mfma_tile.h"

namespace dm {

namespace {

enum ConvMode { CM_3X3_S1 = 0, CM_3X3_S2 = 1, CM_3X3_UP = 2, CM_1X1 = 3 };

// Bijective XCD-aware remap of the linear block id (cdna_hip_programming.md
// §5.5 T1): blocks dispatched round-robin over 8 XCDs; consecutive logical ids
// land on the same XCD so the N-tiles of one M-tile share that XCD's L2.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
  const int q = nblk >> 3, r = nblk & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

template <int BM, int BN, int WM, int WN, int MODE>
__global__ void __launch_bounds__(256)
conv_igemm_kernel(ConvArgs a) {
  using Cfg = TileCfg<BM, BN, WM, WN>;
  __shared__ __attribute__((aligned(16))) float lds[Cfg::LDS_FLOATS];

  const int M = a.B * a.Hout * a.Wout;
  const int N = a.Cout;
  const int nN = ceil_div(N, BN);
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = bid / nN, nt = bid - (bid / nN) * nN;
  const int m0 = mt * BM, n0 = nt * BN;

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave / Cfg::NWN, wn = wave % Cfg::NWN;
  const int lc4 = t & 7;
  const int lrow = t >> 3;
  const int HWo = a.Hout * a.Wout;

  // Per-thread A rows: decode the output pixel once.
  int r_b[Cfg::A_ITERS], r_oy[Cfg::A_ITERS], r_ox[Cfg::A_ITERS];
  bool r_ok[Cfg::A_ITERS];
#pragma unroll
  for (int i = 0; i < Cfg::A_ITERS; ++i) {
    const int m = m0 + lrow + i * Cfg::ROWS_PER_PASS;
    r_ok[i] = m < M;
    const int mm = r_ok[i] ? m : M - 1;
    r_b[i] = mm / HWo;
    const int rem = mm - r_b[i] * HWo;
    r_oy[i] = rem / a.Wout;
    r_ox[i] = rem - r_oy[i] * a.Wout;
  }
  // B rows (output channels), clamped + validity.
  const float* wrow[Cfg::B_ITERS];
  bool w_ok[Cfg::B_ITERS];
#pragma unroll
  for (int j = 0; j < Cfg::B_ITERS; ++j) {
    const int n = n0 + lrow + j * Cfg::ROWS_PER_PASS;
    w_ok[j] = n < N;
    wrow[j] = a.w + (size_t)(w_ok[j] ? n : N - 1) * a.K + 4 * lc4;
  }

  const int taps = (MODE == CM_1X1) ? 1 : 9;
  const int nk1 = taps * (a.Cin1 / kBK);
  const int nk = nk1 + a.Cin2 / kBK;

  // Row pointers / validity for the current tap.
  const float* arow[Cfg::A_ITERS];
  bool a_ok[Cfg::A_ITERS];
  auto set_tap = [&](int tap) {
    const int ky = (MODE == CM_1X1) ? 1 : tap / 3;
    const int kx = (MODE == CM_1X1) ? 1 : tap - (tap / 3) * 3;
#pragma unroll
    for (int i = 0; i < Cfg::A_ITERS; ++i) {
      int iy, ix;
      bool ok = r_ok[i];
      if (MODE == CM_3X3_UP) {
        const int uy = r_oy[i] + ky - 1, ux = r_ox[i] + kx - 1;
        ok = ok && uy >= 0 && uy < 2 * a.Hin && ux >= 0 && ux < 2 * a.Win;
        iy = uy >> 1;
        ix = ux >> 1;
      } else if (MODE == CM_3X3_S2) {
        iy = 2 * r_oy[i] + ky - 1 + a.s2_pad0;
        ix = 2 * r_ox[i] + kx - 1 + a.s2_pad0;
        ok = ok && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
      } else {
        iy = r_oy[i] + ky - 1;
        ix = r_ox[i] + kx - 1;
        ok = ok && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
      }
      iy = min(max(iy, 0), a.Hin - 1);
      ix = min(max(ix, 0), a.Win - 1);
      a_ok[i] = ok;
      // zero padding by address (mfma_tile.h kZeroPage); rows >= M are clamped and discarded
      arow[i] = (ok || !r_ok[i]) ? a.x1 + ((size_t)(r_b[i] * a.Hin + iy) * a.Win + ix) * a.x1_pitch + 4 * lc4
                                 : kZeroPage + 4 * lc4;
    }
  };
  auto set_seg2 = [&]() {
#pragma unroll
    for (int i = 0; i < Cfg::A_ITERS; ++i) {
      const int m = min(m0 + lrow + i * Cfg::ROWS_PER_PASS, M - 1);
      a_ok[i] = r_ok[i];
      arow[i] = a.x2 + (size_t)m * a.x2_pitch + 4 * lc4;
    }
  };

  // Raw loaded registers; the zero-padding select is applied when they are
  // written to LDS (after the MFMA work), so no wait sits between the loads
  // and the compute that hides them.
  f4 ra[Cfg::A_ITERS], rb[Cfg::B_ITERS];
  bool ra_ok[Cfg::A_ITERS];
  const f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  // Loader state: K slice kt = chunk * taps + tap (chunk-major, matching the
  // packed weights), then segment 2.
  int ld_c = 0;
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int i = 0; i < Cfg::A_ITERS; ++i) {
      ra[i] = *reinterpret_cast<const f4*>(arow[i] + ld_c);
      ra_ok[i] = a_ok[i];
    }
#pragma unroll
    for (int j = 0; j < Cfg::B_ITERS; ++j) rb[j] = *reinterpret_cast<const f4*>(wrow[j] + kt * kBK);
    // advance to slice kt + 1 (wave-uniform control flow only)
    const int nx = kt + 1;
    if (nx < nk1) {
      const int chunk = (MODE == CM_1X1) ? nx : nx / 9;
      set_tap((MODE == CM_1X1) ? 0 : nx - chunk * 9);
      ld_c = chunk * kBK;
    } else if (nx == nk1) {
      ld_c = 0;
      set_seg2();
    } else {
      ld_c += kBK;
    }
  };

  auto store_tile = [&](int buf) {
    float* As = lds + buf * Cfg::STAGE;
    float* Bs = As + Cfg::A_ELEMS;
#pragma unroll
    for (int i = 0; i < Cfg::A_ITERS; ++i)
      *reinterpret_cast<f4*>(As + (lrow + i * Cfg::ROWS_PER_PASS) * kLDK + 4 * lc4) = ra[i];
#pragma unroll
    for (int j = 0; j < Cfg::B_ITERS; ++j)
      *reinterpret_cast<f4*>(Bs + (lrow + j * Cfg::ROWS_PER_PASS) * kLDK + 4 * lc4) = rb[j];  // rows >= N: discarded
  };

  f16v acc[Cfg::TM][Cfg::TN];
#pragma unroll
  for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (nk1 > 0) set_tap(0); else set_seg2();
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) load_tile(kt + 1);
    const float* As = lds + buf * Cfg::STAGE;
    const float* Bs = As + Cfg::A_ELEMS;
    mfma_slice<Cfg::TM, Cfg::TN>(As, Bs, wm * WM, wn * WN, lane, acc);
    if (more) store_tile(buf ^ 1);
    __syncthreads();
  }

  // Epilogue.
  const int lr = lane & 31, lh = lane >> 5;
  const bool block_one_image = (HWo % BM) == 0;
  const int b_blk = m0 / HWo;
#pragma unroll
  for (int j = 0; j < Cfg::TN; ++j) {
    const int n = n0 + wn * WN + j * 32 + lr;
    if (n >= N) continue;
    const float bn = a.bias ? a.bias[n] : 0.f;
    const float rv_blk = (a.rowvec && block_one_image) ? a.rowvec[(size_t)b_blk * a.rowvec_pitch + n] : 0.f;
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * WM + i * 32 + acc_row(r, lh);
        if (m >= M) continue;
        float v = acc[i][j][r];
        if (a.bias) v = v + bn;
        if (a.rowvec) v = v + (block_one_image ? rv_blk : a.rowvec[(size_t)(m / HWo) * a.rowvec_pitch + n]);
        if (a.res) v = v + a.res[(size_t)m * a.res_pitch + n];
        a.y[(size_t)m * a.y_pitch + n] = v;
      }
    }
  }
}

template <int BM, int BN, int WM, int WN>
int launch_conv_tile(const ConvArgs& a, int mode, hipStream_t st) {
  using Cfg = TileCfg<BM, BN, WM, WN>;
  const int M = a.B * a.Hout * a.Wout;
  const int blocks = ceil_div(M, BM) * ceil_div(a.Cout, BN);
  switch (mode) {
    case CM_3X3_S1:
      hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WM, WN, CM_3X3_S1>), dim3(blocks), dim3(Cfg::NT), 0, st, a);
      break;
    case CM_3X3_S2:
      hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WM, WN, CM_3X3_S2>), dim3(blocks), dim3(Cfg::NT), 0, st, a);
      break;
    case CM_3X3_UP:
      hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WM, WN, CM_3X3_UP>), dim3(blocks), dim3(Cfg::NT), 0, st, a);
      break;
    default:
      hipLaunchKernelGGL((conv_igemm_kernel<BM, BN, WM, WN, CM_1X1>), dim3(blocks), dim3(Cfg::NT), 0, st, a);
      break;
  }
  DM_LAUNCH_CHECK();
  return DM_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int conv_mode(const ConvArgs& a) {
  if (a.taps == 1) return CM_1X1;
  if (a.upsample) return CM_3X3_UP;
  return a.stride == 2 ? CM_3X3_S2 : CM_3X3_S1;
}

// The public forcing knob (dm_conv_desc.tile, ConvArgs::tile) -> the kernel form it names: the only place the numbers
// mean anything (DESIGN.md §4.21 has the table in words). 0 is the automatic choice. A forced form that does not fit
// falls back to Im2col (the halo-patch tiles 4..6 to their own shape, every other to 128 x 128), except 21 and 23,
// which are errors then. (A conv marked h16 reads tile as conv_h16_form does: 1 / 2 force H16Form::Rows / T2D.)
struct TileForm {
  ConvFamily family;
  ConvTile tile;
  K32Form k32;
};
constexpr TileForm tiled(ConvFamily f, ConvTile t) { return {f, t, K32Form::None}; }
constexpr TileForm k32_form(K32Form k) {
  return {k == K32Form::Small8 ? ConvFamily::K32Small : ConvFamily::K32, ConvTile::None, k};
}
constexpr int kNumTiles = 24;
const TileForm kTileForms[kNumTiles] = {
    /* 0 */ tiled(ConvFamily::Im2col, ConvTile::None),  // automatic
    /* 1 */ tiled(ConvFamily::Im2col, ConvTile::T128x128),
    /* 2 */ tiled(ConvFamily::Im2col, ConvTile::T128x64),
    /* 3 */ tiled(ConvFamily::Im2col, ConvTile::T64x64),
    /* 4 */ tiled(ConvFamily::Patch, ConvTile::T128x128),  // 4..6: fp32 (Patch) or split (Patch3) by the conv's weights
    /* 5 */ tiled(ConvFamily::Patch, ConvTile::T128x64),
    /* 6 */ tiled(ConvFamily::Patch, ConvTile::T64x64),
    /* 7 */ tiled(ConvFamily::Patch3, ConvTile::T256x256),  // 7..9: fp16x2 only
    /* 8 */ tiled(ConvFamily::Patch3, ConvTile::T512x128),
    /* 9 */ tiled(ConvFamily::Patch3, ConvTile::Seg128),
    /* 10 */ k32_form(K32Form::T128x128),
    /* 11 */ k32_form(K32Form::T128x64),
    /* 12 */ k32_form(K32Form::SplitK64x64),
    /* 13 */ k32_form(K32Form::SplitK64x128),
    /* 14 */ k32_form(K32Form::Seg64),
    /* 15 */ k32_form(K32Form::Small8),
    /* 16 */ k32_form(K32Form::Wide512),
    /* 17 */ k32_form(K32Form::BigTab),
    /* 18 */ k32_form(K32Form::S2),
    /* 19 */ k32_form(K32Form::T2D),
    /* 20 */ k32_form(K32Form::Rows64),
    /* 21 */ tiled(ConvFamily::Wino, ConvTile::None),
    /* 22 */ k32_form(K32Form::S2Seg),
    /* 23 */ tiled(ConvFamily::SubWino, ConvTile::None),
};

#define DM_REFUSE(cond, msg) \
  do {                       \
    if (!(cond)) return msg; \
  } while (0)

// a descriptor no kernel can be chosen for
const char* conv_check_problem(const ConvArgs& a) {
  DM_REFUSE(a.taps == 1 || a.taps == 9, "conv: taps must be 1 or 9");
  DM_REFUSE(a.stride == 1 || a.stride == 2, "conv: stride must be 1 or 2");
  DM_REFUSE(!a.upsample || (a.taps == 9 && a.stride == 1), "conv: upsample needs 3x3 stride 1");
  DM_REFUSE(a.upsample >= 0 && a.upsample <= 2, "conv: upsample must be 0, 1 (nearest) or 2 (sub-pixel)");
  DM_REFUSE(a.Cin1 % kBK == 0 && a.Cin2 % kBK == 0, "conv: input channels must be multiples of 32");
  DM_REFUSE(a.Cin1 + kBK <= kZeroPageFloats, "conv: too many input channels for the zero-padding page");
  DM_REFUSE(a.Cin1 > 0, "conv: no input channels");
  DM_REFUSE(a.K == (a.upsample == 2 ? 4 : a.taps) * a.Cin1 + a.Cin2, "conv: K mismatch");
  DM_REFUSE(a.upsample != 2 || a.Cin2 == 0, "conv: sub-pixel upsample has no second segment");
  DM_REFUSE(a.Cout > 0 && a.B > 0 && a.Hin > 0 && a.Win > 0, "conv: empty problem");
  if (a.upsample) {
    DM_REFUSE(a.Hout == 2 * a.Hin && a.Wout == 2 * a.Win, "conv: upsample output size");
  } else if (a.s2_pad0) {  // input padded (0, 1, 0, 1): floor((H + 1 - 3) / 2) + 1 output rows
    DM_REFUSE(a.s2_pad0 == 1 && a.taps == 9 && a.stride == 2, "conv: s2_pad0 is for 3x3 stride-2 convs");
    DM_REFUSE(a.Hin >= 2 && a.Win >= 2 && a.Hout == (a.Hin - 2) / 2 + 1 && a.Wout == (a.Win - 2) / 2 + 1,
              "conv: 3x3 stride-2 (bottom/right padding) output size");
  } else if (a.taps == 9) {
    DM_REFUSE(a.Hout == (a.Hin - 1) / a.stride + 1 && a.Wout == (a.Win - 1) / a.stride + 1, "conv: 3x3 output size");
  } else {
    DM_REFUSE(a.stride == 1 && a.Hout == a.Hin && a.Wout == a.Win, "conv: 1x1 output size");
  }
  const long M = (long)a.B * a.Hout * a.Wout;
  DM_REFUSE(M > 0 && M < (1L << 31), "conv: M out of range");
  return nullptr;
}

// operands every kernel refuses (a question asked before the buffers exist still gets its choice: ConvChoice::error)
const char* conv_check_operands(const ConvArgs& a) {
  DM_REFUSE(a.x1_pitch % 4 == 0 && a.y_pitch >= a.Cout && a.K % 4 == 0, "conv: pitch");
  DM_REFUSE(aligned16(a.x1) && aligned16(a.w), "conv: operands must be 16-byte aligned");
  DM_REFUSE(a.Cin2 == 0 || (a.x2 && aligned16(a.x2) && a.x2_pitch % 4 == 0), "conv: segment-2 operand");
  return nullptr;
}

// the kernel, given the facts every family shares (conv_choose)
const char* conv_choose_kernel(const ConvArgs& a, const TileForm& forced, bool automatic, bool pointwise, bool rows64,
                               ConvTile halo, ConvChoice& ch) {
  if (a.h16) {  // a conv the plan marked for the conv-half kernel
    ch.family = ConvFamily::H16;
    ch.h16 = conv_h16_form(a);
    ch.emits_gn = conv_h16_can_emit(a);
    DM_REFUSE(ch.h16 != H16Form::None && a.h16_a1 && (a.Cin2 == 0 || a.h16_a2),
              "conv_h16: needs the fp16 image plane(s), fp16x2 split weights and a covered 3x3 stride-1 shape");
    return nullptr;
  }
  DM_REFUSE(a.tile >= 0 && a.tile < kNumTiles, "conv: tile must be 0..23");
  // the sub-pixel Winograd upsample kernel: forced, or the conv has its weights
  if (forced.family == ConvFamily::SubWino || (automatic && a.subwino_ws)) {
    if (conv_subwino_ok(a)) {
      ch.family = ConvFamily::SubWino;
      ch.emits_gn = true;  // (conv_subwino_shape_ok's group rule)
      return nullptr;
    }
    DM_REFUSE(automatic, "conv: tile 23 needs sub-pixel Winograd weights and a shape conv_subwino_kernel takes");
  }
  // the Winograd F(2,3) kernel, likewise
  if (forced.family == ConvFamily::Wino || (automatic && a.wino_ws)) {
    if (conv_wino_ok(a)) {
      ch.emits_gn = a.ksplit > 1 ? conv_splitk_can_emit(a) : conv_wino_can_emit(a);
      if (!a.gn_part || ch.emits_gn) {
        ch.family = ConvFamily::Wino;
        return nullptr;
      }
      DM_REFUSE(automatic, "conv: GroupNorm statistics need groups of 4..32 channels");
      // (automatic choice) statistics the Winograd epilogue cannot emit: the direct kernels, below
    } else {
      DM_REFUSE(automatic, "conv: tile 21 needs Winograd weights and a shape conv_wino_kernel takes");
    }
  }
  // the direct kernels. K32 where a form is forced and fits, or the automatic choice takes one
  const bool force_k32 = forced.family == ConvFamily::K32 || forced.family == ConvFamily::K32Small;
  ch.k32 = force_k32 ? (conv_k32_variant_ok(a, forced.k32) ? forced.k32 : K32Form::None)
                     : automatic ? k32_choose(a, halo) : K32Form::None;
  ch.emits_gn = a.ksplit > 1            ? conv_splitk_can_emit(a)
                : ch.k32 != K32Form::None ? conv_k32_can_emit(a, ch.k32, rows64)
                                          : rows64 && conv_patch_can_emit(a);
  DM_REFUSE(!a.gn_part || ch.emits_gn, "conv: GroupNorm statistics need a 128-row halo-patch tile, whole 64-pixel "
                                       "chunks and groups within 32 channels");
  DM_REFUSE(!a.pro_scale || (ch.takes_prologue && a.pro_shift && aligned16(a.pro_scale) && aligned16(a.pro_shift)),
            "conv: the GroupNorm prologue needs a halo-patch shape (3x3 stride 1 / upsample, whole-row tiles)");
  if (ch.k32 != K32Form::None) {
    ch.family = ch.k32 == K32Form::Small8 || ch.k32 == K32Form::Small4 ? ConvFamily::K32Small : ConvFamily::K32;
    return nullptr;
  }
  const long M = (long)(a.pick_B > 0 ? a.pick_B : a.B) * a.Hout * a.Wout;
  const long b128 = ((M + 127) / 128) * ((a.Cout + 127) / 128);
  if (pointwise) {  // split 1x1: 128x128 tiles when they still give >= 2 blocks per CU, else 128x64
    ch.family = ConvFamily::Pointwise3;
    ch.tile = a.Cout >= 128 && b128 >= 512 ? ConvTile::T128x128 : ConvTile::T128x64;
    return conv_patch3_refuses(a, ch);
  }
  if (halo != ConvTile::None) {
    ch.tile = halo;
    if (conv_patch3_ok(a, halo, ch.geom)) {
      ch.family = ConvFamily::Patch3;
      return conv_patch3_refuses(a, ch);
    }
    if (halo == ConvTile::T128x128 || halo == ConvTile::T128x64 || halo == ConvTile::T64x64) {
      ch.family = ConvFamily::Patch;
      return conv_patch_refuses(a);
    }
    ch.tile = ConvTile::T128x128;  // a split-only tile that does not fit: Im2col
    return nullptr;
  }
  // Im2col: the forced tile, the im2col shape of a forced halo-patch tile that does not fit, 128 x 128 for any other
  // forced form that does not; else the 128x128 tile when it still yields >= 2 waves of blocks over 256 CUs
  DM_REFUSE(a.upsample != 2, "conv: the sub-pixel upsample runs on the halo-patch kernel only (shape has no "
                             "whole-row tiling)");
  if (!automatic) {
    ch.tile = forced.family == ConvFamily::Im2col || forced.family == ConvFamily::Patch ? forced.tile : ConvTile::T128x128;
    return nullptr;
  }
  const long b128x64 = ((M + 127) / 128) * ((a.Cout + 63) / 64);
  ch.tile = a.Cout >= 128 && b128 >= 512 ? ConvTile::T128x128 : b128x64 >= 512 ? ConvTile::T128x64 : ConvTile::T64x64;
  return nullptr;
}

#undef DM_REFUSE

const char* tile_dims(ConvTile t) {
  switch (t) {
    case ConvTile::T128x64: return "128,64,64,32";
    case ConvTile::T64x64: return "64,64,32,32";
    case ConvTile::T256x256: return "256,256,128,128";
    case ConvTile::T512x128: return "512,128,128,128";
    default: return "128,128,64,64";  // T128x128, Seg128
  }
}

}  // namespace

// The one decision. First the facts every family shares -- the forced form, the conv's halo-patch tiling and what
// the plans ask of it (takes_prologue, lds_tables: properties of that tiling, which the K32 and Winograd forms that
// replace a halo-patch tile inherit) -- then the kernel, in the order of precedence H16, SubWino, Wino, K32,
// Pointwise3, Patch3, Patch, Im2col.
ConvChoice conv_choose(const ConvArgs& a) {
  ConvChoice ch;
  if ((ch.error = conv_check_problem(a))) return ch;
  const bool automatic = a.tile == 0;
  const TileForm forced = a.tile > 0 && a.tile < kNumTiles ? kTileForms[a.tile] : kTileForms[0];
  const bool force_im2col = forced.family == ConvFamily::Im2col && forced.tile != ConvTile::None;
  const bool force_halo = forced.family == ConvFamily::Patch || forced.family == ConvFamily::Patch3;
  const bool pointwise = !force_im2col && conv_pw_ok(a);
  ConvTile halo = ConvTile::None;
  if (automatic || force_halo) halo = conv_patch_pick(a, forced.tile, ch.geom);
  if (halo == ConvTile::None) ch.geom = PatchGeom{};
  // another family's forced form that fits takes the prologue too
  const bool force_k32 = forced.family == ConvFamily::K32 || forced.family == ConvFamily::K32Small;
  const bool forced_fits = (force_k32 && conv_k32_variant_ok(a, forced.k32)) ||
                           (forced.family == ConvFamily::SubWino && conv_subwino_ok(a));
  ch.takes_prologue = forced_fits || pointwise || halo != ConvTile::None;
  ch.lds_tables = a.pro_scale && a.ws_np == 2 &&
                  (a.taps == 1 ? conv_pw_ok(a) : halo != ConvTile::None && conv_patch3_ok(a, halo, ch.geom));
  // whether the tile's waves own whole 64-row chunks (the 64-row tiles' waves do not): the statistics rules' premise
  const K32Form fk = forced.k32;
  const bool rows64 = forced_fits ? !(fk == K32Form::SplitK64x64 || fk == K32Form::SplitK64x128 ||
                                      fk == K32Form::Small8 || fk == K32Form::S2 || fk == K32Form::S2Seg)
                                  : pointwise || (halo != ConvTile::None && halo != ConvTile::T64x64);
  const char* refused = conv_choose_kernel(a, forced, automatic, pointwise, rows64, halo, ch);
  const char* operands = conv_check_operands(a);
  ch.error = operands ? operands : refused;
  return ch;
}

int conv2d_run(const ConvArgs& a, const ConvChoice& ch, hipStream_t st) {
  DM_REQUIRE(!ch.error, ch.error);
  switch (ch.family) {
    case ConvFamily::H16: return conv2d_h16(a, st);
    case ConvFamily::SubWino: return conv2d_subwino(a, st);
    case ConvFamily::Wino: return conv2d_wino(a, st);
    case ConvFamily::K32:
    case ConvFamily::K32Small: return conv2d_k32(a, ch.k32, st);
    case ConvFamily::Pointwise3:
    case ConvFamily::Patch3: return conv2d_patch3(a, ch, st);
    case ConvFamily::Patch: return conv2d_patch(a, ch.tile, ch.geom, st);
    case ConvFamily::Im2col: break;
  }
  const int mode = conv_mode(a);
  switch (ch.tile) {
    case ConvTile::T128x128: return launch_conv_tile<128, 128, 64, 64>(a, mode, st);
    case ConvTile::T128x64: return launch_conv_tile<128, 64, 64, 32>(a, mode, st);
    default: return launch_conv_tile<64, 64, 32, 32>(a, mode, st);
  }
}

// The exact kernel instantiation (matches the rocprofv3 kernel name with spaces removed).
std::string conv_label(const ConvArgs& a, const ConvChoice& ch) {
  const char* pro = a.pro_scale ? "true" : "false";
  switch (ch.family) {
    case ConvFamily::H16: return conv_h16_label(a, ch.h16);
    case ConvFamily::SubWino: return conv_subwino_label(a);
    case ConvFamily::Wino: return conv_wino_label(a);
    case ConvFamily::K32:
    case ConvFamily::K32Small: return conv_k32_label(a, ch.k32);
    case ConvFamily::Pointwise3:  // conv_patch3_kernel<128,BN,64,WN,3,128,PRO,false,2>
      return std::string("conv_patch3_kernel<") + tile_dims(ch.tile) + ",3,128," + pro + ",false,2>";
    case ConvFamily::Im2col:  // <BM,BN,WM,WN,MODE>
      return std::string("conv_igemm_kernel<") + tile_dims(ch.tile) + "," + std::to_string(conv_mode(a)) + ">";
    default: break;
  }
  // <BM,BN,WM,WN,MODE,MAXP,PRO,KSPLIT(,NP)>; rocprofv3 prints the defaulted arguments too. NP: 3 bf16x3, 2 fp16x2
  const bool x3 = ch.family == ConvFamily::Patch3;
  const int maxp = a.stride == 2                     ? kPatchS2Max
                   : ch.tile == ConvTile::T64x64     ? kPatch3Max64  // (= kPatchMax64)
                   : ch.tile == ConvTile::T256x256   ? kPatch3Max256
                   : ch.tile == ConvTile::T512x128   ? kPatch3Max512
                   : ch.tile == ConvTile::Seg128     ? kPatch3Seg
                                                     : (x3 ? kPatch3Max128 : kPatchMax128);
  return std::string(x3 ? "conv_patch3_kernel<" : "conv_patch_kernel<") + tile_dims(ch.tile) + "," +
         std::to_string(a.stride == 2 ? 4 : a.upsample) + "," + std::to_string(maxp) + "," + pro +
         (a.ksplit > 1 ? ",true" : ",false") + (x3 ? "," + std::to_string(a.ws_np) + ">" : ">");
}

// "family:variant" (dm_debug_conv_choice; tests/test_conv_dispatch_host.py)
std::string conv_choice_name(const ConvArgs& a, const ConvChoice& ch) {
  static const char* tiles[] = {"none", "128x128", "128x64", "64x64", "256x256", "512x128", "seg128"};
  static const char* k32[] = {"none", "t128x128", "t128x64", "splitk64x64", "splitk64x128", "seg64", "w8", "wide512",
                              "bigtab", "s2", "t2d", "rows64", "w4", "s2seg"};
  switch (ch.family) {
    case ConvFamily::Im2col: return std::string("im2col:") + tiles[(int)ch.tile];
    case ConvFamily::Patch: return std::string("patch:") + tiles[(int)ch.tile];
    case ConvFamily::Patch3: return std::string("patch3:") + tiles[(int)ch.tile];
    case ConvFamily::Pointwise3: return std::string("pw3:") + tiles[(int)ch.tile];
    case ConvFamily::K32: return std::string("k32:") + k32[(int)ch.k32];
    case ConvFamily::K32Small: return std::string("k32small:") + k32[(int)ch.k32];
    case ConvFamily::Wino: return a.Wout > 32 ? std::string("wino:wide") : "wino:w" + std::to_string(a.Wout);
    case ConvFamily::SubWino: return "subwino:w" + std::to_string(a.Win);
    case ConvFamily::H16: return ch.h16 == H16Form::T2D ? "h16:t2d" : "h16:rows";
  }
  return "";
}

}  // namespace dm
