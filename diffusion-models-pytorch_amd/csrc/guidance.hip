// Guided sampling on the sampled x_{t-1} (reference diffusions/guidance/): the DDPM update of
// sampler_step.h fused with cond_fn_sample of
//   * MaskGuidance (mask_guidance.py:52-62): sample + (noisy_known - sample) * mask, one elementwise launch;
//   * ILVR (ilvr.py:38-52): sample + phi(noisy_ref) - phi(sample) = sample + phi(noisy_ref - sample) by the
//     linearity of phi, the low-pass filter resize(resize(x, 1/N), N) of utils/resize_right.
// phi is separable and linear: four banded passes (down-H, down-W, up-H, up-W, the reference's order), each
// output an fp32 sum over its taps in tap order with separately rounded products (-ffp-contract=off). The
// kernels are table driven (AxisTable: weights [out][taps] + the left input index per output, taps that fall
// outside the axis read the reference's zero padding and are skipped); the host builds the tables with the
// reference's torch op sequence, so the kernels know nothing about the interpolation method.
//
// Launch layout
//   one launch (plane <= 64 x 64): one 256-thread block per (b, c) plane. LDS: X [H][W] (the plane, or
//     d = noisy_ref - sample), T1 [H/N][W | 1] (down-H; odd pitch), T2 [H/N][W/N] (down-W), T3 [H][W/N] (up-H);
//     the unguided sample stays in registers (16 per thread) until the last pass adds phi(d) to it.
//     Pass 1, 3, 4 run with the column index fastest over the lanes: consecutive LDS words per tap (pass 1, 3)
//     or one word per N lanes (pass 4, a broadcast), conflict-free, and coalesced global rows in and out.
//     Pass 2 reads T1 rows at a lane stride of N words; it runs with the row index fastest instead, so with the
//     odd row pitch the lanes of a wave fall on different banks.
//   two launches (larger planes): (1) one block per (plane, low-res row r): every thread owns a column, forms d
//     for the input rows of r's field of view (coalesced rows; the update's outputs are written by the block
//     that owns the row, row / N == r), accumulates down-H in a register, then the row of T1 goes through LDS for
//     down-W and T2 [H/N][W/N] -- 1/N^2 of a plane -- goes to the global scratch; (2) one block per (plane,
//     16 output rows): up-H of the rows' field of view from T2 into LDS [16][W/N], up-W from LDS, added to the
//     sample in place. noisy_ref and d never reach global memory.
#include "dm_common.h"
#include "dm_kernels.h"
#include "sampler_step.h"

namespace dm {

namespace {

constexpr int kNT = 256;
constexpr int kFusedPlane = 64 * 64;          // largest plane of the one-launch form
constexpr int kPerThread = kFusedPlane / kNT;  // its elements per thread
constexpr int kUpRows = 16;                    // output rows per block of the second launch

// noisy_known / noisy_ref of element e: q(x_{t_prev} | known) with the caller's noise, or `known` at t == 0
__device__ __forceinline__ float noisy_of(const GuideArgs& g, long e) {
  const float kn = g.known[e];
  return g.noise_known ? g.c_a * kn + g.c_b * g.eps_k[e] : kn;
}

__global__ void mask_step_kernel(StepArgs s, GuideArgs g) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = (long)s.C * s.HW;
  if (e >= per * s.B) return;
  const float sample = step_elem(s, e);
  long mi = e;
  if (g.mask_c == 1) {
    const long b = e / per;
    mi = b * s.HW + (e - b * per) % s.HW;
  }
  s.sample[e] = sample + (noisy_of(g, e) - sample) * g.mask[mi];  // mask_guidance.py:62 then base.py:137
}

// sum_k w[o][k] * src(left[o] + k) over the taps inside [0, n_in)
template <typename F>
__device__ __forceinline__ float axis_sum(const AxisTable& t, int o, F&& src) {
  const int left = t.left[o];
  const int k0 = max(0, -left), k1 = min(t.taps, t.n_in - left);
  const float* w = t.w + (size_t)o * t.taps;
  float acc = 0.f;
  for (int k = k0; k < k1; ++k) acc = acc + w[k] * src(left + k);
  return acc;
}

__host__ __device__ inline int t1_pitch(int W) { return W | 1; }

template <bool STEP>
__global__ void __launch_bounds__(kNT) lowpass_plane_kernel(Lowpass lp, StepArgs s, GuideArgs g,
                                                            const float* __restrict__ x, float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float smem_g[];
  const int H = lp.H, W = lp.W, Hn = lp.dh.n_out, Wn = lp.dw.n_out, HW = H * W, P1 = t1_pitch(W);
  float* X = smem_g;
  float* T1 = X + HW;
  float* T2 = T1 + Hn * P1;
  float* T3 = T2 + Hn * Wn;
  const long e0 = (long)blockIdx.x * HW;
  const int tid = threadIdx.x;
  float smp[kPerThread];
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const int i = tid + kNT * j;
    smp[j] = 0.f;
    if (i < HW) {
      if (STEP) {
        smp[j] = step_elem(s, e0 + i);
        X[i] = noisy_of(g, e0 + i) - smp[j];
      } else {
        X[i] = x[e0 + i];
      }
    }
  }
  __syncthreads();
  for (int idx = tid; idx < Hn * W; idx += kNT) {  // down-H
    const int r = idx / W, c = idx - r * W;
    T1[r * P1 + c] = axis_sum(lp.dh, r, [&](int row) { return X[row * W + c]; });
  }
  __syncthreads();
  for (int idx = tid; idx < Hn * Wn; idx += kNT) {  // down-W, row index fastest
    const int c2 = idx / Hn, r = idx - c2 * Hn;
    T2[r * Wn + c2] = axis_sum(lp.dw, c2, [&](int col) { return T1[r * P1 + col]; });
  }
  __syncthreads();
  for (int idx = tid; idx < H * Wn; idx += kNT) {  // up-H
    const int R = idx / Wn, c2 = idx - R * Wn;
    T3[idx] = axis_sum(lp.uh, R, [&](int row) { return T2[row * Wn + c2]; });
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {  // up-W
    const int i = tid + kNT * j;
    if (i < HW) {
      const int R = i / W, C = i - R * W;
      const float f = axis_sum(lp.uw, C, [&](int col) { return T3[R * Wn + col]; });
      if (STEP)
        s.sample[e0 + i] = smp[j] + f;
      else
        y[e0 + i] = f;
    }
  }
}

// first launch of the two-launch form: block = (plane, low-res row r)
template <bool STEP>
__global__ void __launch_bounds__(kNT) lowpass_down_kernel(Lowpass lp, StepArgs s, GuideArgs g,
                                                           const float* __restrict__ x, float* __restrict__ t2) {
  extern __shared__ __attribute__((aligned(16))) float smem_g[];  // one row of T1: [W]
  const int H = lp.H, W = lp.W, N = lp.N, Hn = lp.dh.n_out, Wn = lp.dw.n_out;
  const long p = blockIdx.x / Hn;
  const int r = blockIdx.x - p * Hn;
  const long e0 = p * (long)H * W;
  const int left = lp.dh.left[r], taps = lp.dh.taps;
  const float* w = lp.dh.w + (size_t)r * taps;
  // the rows of r's field of view and, with the update fused, the N rows this block owns
  int lo = max(left, 0), hi = min(left + taps, H);
  if (STEP) {
    lo = min(lo, r * N);
    hi = max(hi, (r + 1) * N);
  }
  for (int c = threadIdx.x; c < W; c += kNT) {
    float acc = 0.f;
    for (int row = lo; row < hi; ++row) {
      const long e = e0 + (long)row * W + c;
      float d;
      if (STEP) {
        const bool own = row / N == r;
        const float sample = step_elem(s, e, own);
        if (own) s.sample[e] = sample;
        d = noisy_of(g, e) - sample;
      } else {
        d = x[e];
      }
      const int k = row - left;
      if (k >= 0 && k < taps) acc = acc + w[k] * d;
    }
    smem_g[c] = acc;
  }
  __syncthreads();
  for (int c2 = threadIdx.x; c2 < Wn; c2 += kNT)
    t2[(p * Hn + r) * Wn + c2] = axis_sum(lp.dw, c2, [&](int col) { return smem_g[col]; });
}

// second launch: block = (plane, kUpRows output rows)
template <bool STEP>
__global__ void __launch_bounds__(kNT) lowpass_up_kernel(Lowpass lp, const float* __restrict__ t2, float* y,
                                                         int tiles) {
  extern __shared__ __attribute__((aligned(16))) float smem_g[];  // T3 rows of the tile: [kUpRows][W/N]
  const int H = lp.H, W = lp.W, Hn = lp.dh.n_out, Wn = lp.dw.n_out;
  const long p = blockIdx.x / tiles;
  const int R0 = (blockIdx.x - p * tiles) * kUpRows;
  const int rows = min(kUpRows, H - R0);
  const float* t2p = t2 + p * (long)Hn * Wn;
  for (int idx = threadIdx.x; idx < rows * Wn; idx += kNT) {
    const int Rl = idx / Wn, c2 = idx - Rl * Wn;
    smem_g[idx] = axis_sum(lp.uh, R0 + Rl, [&](int row) { return t2p[row * Wn + c2]; });
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < rows * W; idx += kNT) {
    const int Rl = idx / W, C = idx - Rl * W;
    const float f = axis_sum(lp.uw, C, [&](int col) { return smem_g[Rl * Wn + col]; });
    const long e = p * (long)H * W + (long)(R0 + Rl) * W + C;
    y[e] = STEP ? y[e] + f : f;  // STEP: y is the sample the first launch wrote
  }
}

size_t plane_smem(const Lowpass& lp) {
  const int Hn = lp.dh.n_out, Wn = lp.dw.n_out;
  return ((size_t)lp.H * lp.W + (size_t)Hn * t1_pitch(lp.W) + (size_t)Hn * Wn + (size_t)lp.H * Wn) * sizeof(float);
}

bool one_launch(const Lowpass& lp) { return lp.H * lp.W <= kFusedPlane && plane_smem(lp) <= 64 * 1024; }

template <bool STEP>
int lowpass_launch(const Lowpass& lp, const StepArgs& s, const GuideArgs& g, const float* x, float* y, long planes,
                   float* scratch, hipStream_t st) {
  if (planes == 0) return DM_OK;
  const int Hn = lp.dh.n_out;
  if (one_launch(lp)) {
    DM_REQUIRE(planes < (1L << 31), "low-pass filter: too many planes");
    hipLaunchKernelGGL(lowpass_plane_kernel<STEP>, dim3((unsigned)planes), dim3(kNT), plane_smem(lp), st, lp, s, g, x,
                       y);
    DM_LAUNCH_CHECK();
    return DM_OK;
  }
  DM_REQUIRE(scratch, "low-pass filter: this plane size needs the scratch of dm_lowpass_scratch_bytes");
  const int tiles = ceil_div(lp.H, kUpRows);
  DM_REQUIRE(planes * Hn < (1L << 31) && planes * tiles < (1L << 31), "low-pass filter: too many planes");
  hipLaunchKernelGGL(lowpass_down_kernel<STEP>, dim3((unsigned)(planes * Hn)), dim3(kNT), lp.W * sizeof(float), st,
                     lp, s, g, x, scratch);
  DM_LAUNCH_CHECK();
  hipLaunchKernelGGL(lowpass_up_kernel<STEP>, dim3((unsigned)(planes * tiles)), dim3(kNT),
                     (size_t)kUpRows * lp.dw.n_out * sizeof(float), st, lp, scratch, y, tiles);
  DM_LAUNCH_CHECK();
  return DM_OK;
}

}  // namespace

int lowpass_create(int H, int W, int N, const float* const w[4], const int* const left[4], const int taps[4],
                   hipStream_t st, Lowpass* out) {
  DM_REQUIRE(out, "low-pass plan: null output");
  DM_REQUIRE(H > 0 && W > 0 && N > 0 && H % N == 0 && W % N == 0, "low-pass plan: N must divide H and W");
  DM_REQUIRE(H <= 256 && W <= 256, "low-pass plan: planes up to 256 x 256");
  const int n_out[4] = {H / N, W / N, H, W}, n_in[4] = {H, W, H / N, W / N};
  size_t off[4][2], bytes = 0;
  for (int i = 0; i < 4; ++i) {
    DM_REQUIRE(w[i] && left[i] && taps[i] > 0 && taps[i] <= (1 << 16), "low-pass plan: null table or bad tap count");
    off[i][0] = bytes;
    bytes += (size_t)n_out[i] * taps[i] * sizeof(float);
    off[i][1] = bytes;
    bytes += (((size_t)n_out[i] * sizeof(int)) + 15) & ~(size_t)15;
    bytes = (bytes + 15) & ~(size_t)15;
  }
  char* dev = nullptr;
  DM_CHECK_HIP(hipMalloc(&dev, bytes));
  AxisTable t[4];
  for (int i = 0; i < 4; ++i) {
    hipError_t e = hipMemcpyAsync(dev + off[i][0], w[i], (size_t)n_out[i] * taps[i] * sizeof(float),
                                  hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
      e = hipMemcpyAsync(dev + off[i][1], left[i], (size_t)n_out[i] * sizeof(int), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) {
      (void)hipFree(dev);
      set_error(std::string("low-pass plan: table copy: ") + hipGetErrorString(e));
      return DM_ERR_HIP;
    }
    t[i] = AxisTable{reinterpret_cast<const float*>(dev + off[i][0]), reinterpret_cast<const int*>(dev + off[i][1]),
                     n_out[i], n_in[i], taps[i]};
  }
  // the host tables may go away once this returns
  if (hipError_t e = hipStreamSynchronize(st); e != hipSuccess) {
    (void)hipFree(dev);
    set_error(std::string("low-pass plan: table copy: ") + hipGetErrorString(e));
    return DM_ERR_HIP;
  }
  *out = Lowpass{H, W, N, t[0], t[1], t[2], t[3], dev};
  return DM_OK;
}

void lowpass_destroy(Lowpass* lp) {
  if (lp && lp->dev) {
    (void)hipFree(lp->dev);
    lp->dev = nullptr;
  }
}

long lowpass_scratch_floats(const Lowpass& lp, long planes) {
  return one_launch(lp) ? 0 : planes * (long)lp.dh.n_out * lp.dw.n_out;
}

int lowpass_apply(const Lowpass& lp, const float* x, float* y, long planes, float* scratch, hipStream_t st) {
  DM_REQUIRE(x && y && planes >= 0, "low-pass filter: null tensor or bad plane count");
  DM_REQUIRE(x != y, "low-pass filter: in place is not supported");
  return lowpass_launch<false>(lp, StepArgs{}, GuideArgs{}, x, y, planes, scratch, st);
}

int guided_step(const StepArgs& s, const GuideArgs& g, hipStream_t st) {
  DM_REQUIRE(s.xt && s.out_c && s.sample, "guided step: null tensor");
  DM_REQUIRE(s.euler == 0, "guided step: DDPM / DDIM updates only");
  DM_REQUIRE(s.Cm == s.C || s.Cm == 2 * s.C, "guided step: model output channels must be C or 2C");
  DM_REQUIRE(s.var_mode == 0 || s.Cm == 2 * s.C, "guided step: learned_range needs 2C model channels");
  DM_REQUIRE(g.known && (!g.noise_known || g.eps_k), "guided step: null known image or noise");
  const long total = (long)s.B * s.C * s.HW;
  if (g.kind == 1) {
    DM_REQUIRE(g.mask && (g.mask_c == 1 || g.mask_c == s.C), "guided step: the mask has 1 or C channels");
    if (total == 0) return DM_OK;
    hipLaunchKernelGGL(mask_step_kernel, dim3((unsigned)((total + kNT - 1) / kNT)), dim3(kNT), 0, st, s, g);
    DM_LAUNCH_CHECK();
    return DM_OK;
  }
  DM_REQUIRE(g.kind == 2, "guided step: kind must be 1 (mask) or 2 (ILVR)");
  DM_REQUIRE(g.lp && g.lp->dev && g.lp->H * g.lp->W == s.HW, "guided step: the low-pass plan does not match the image");
  return lowpass_launch<true>(*g.lp, s, g, nullptr, s.sample, (long)s.B * s.C, g.scratch, st);
}

}  // namespace dm
