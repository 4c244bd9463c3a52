// Native executor for the image encoder of the KL autoencoder (reference
// models/stablediffusion/autoencoder.py: Encoder :280-373, AutoEncoderKL.encode :516-520,
// DiagonalGaussianDistribution; the other half of vae_exec.hip's decoder).
//
// Forward: conv_in -> per level i = 0 .. L-1 num_res_blocks ResnetBlocks (the first of a level changes the width from
// ch * (1,)+ch_mult[i] to ch * ch_mult[i]) and, except at the last level, Downsample -- a 3x3 stride-2 conv of the
// input padded at the bottom and right only (ConvArgs::s2_pad0) -> mid.block_1 -> mid.attn_1 -> mid.block_2 ->
// norm_out -> SiLU -> conv_out (2 z_channels) -> quant_conv (1x1) -> mean | logvar -> clamp -> z.
// No attention outside the middle block, no time embedding.
//
// The blocks and their weights are vae_blocks.h's, shared with the decoder; the arithmetic state, the forward driver
// and the ABI bodies are exec_core.h's. The plan (per
// (B, H, W) and arithmetic) ends at conv_out's NCHW output; the posterior kernel runs after it on the caller's
// buffers, since the noise, the scale and which outputs are wanted change from call to call.
#include <algorithm>
#include <cmath>
#include <functional>
#include <map>
#include <memory>
#include <vector>

#include "dm_common.h"
#include "dm_kernels.h"
#include "plan.h"
#include "exec_pack.h"
#include "vae_blocks.h"

namespace dm {

namespace {

// Posterior: moments = quant_conv(h) (1x1 over the 2 zc channels, products accumulated in channel order with
// separately rounded adds, as vae_latent_in_kernel's post_quant_conv; w == null: h itself), mean | logvar,
// logvar clamped to [-30, 20], std = exp(0.5 logvar), z = scale * (mean + std * noise) (noise == null: scale * mean).
// h: [B][2 zc][HW] (conv3x3_small_out's NCHW planes); z: [B][zc][HW]; mom (nullable): [B][2 zc][HW] mean, clamped logvar.
constexpr int kVaeMaxZ = 4;
__global__ void vae_moments_kernel(const float* __restrict__ h, int ZC, long HW, long n, const float* __restrict__ w,
                                   const float* __restrict__ bias, const float* __restrict__ noise, float scale,
                                   float* __restrict__ z, float* __restrict__ mom) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (b, p)
  if (i >= n) return;
  const long b = i / HW, p = i - b * HW;
  const int C2 = 2 * ZC;
  float v[2 * kVaeMaxZ], m[2 * kVaeMaxZ];
#pragma unroll
  for (int c = 0; c < 2 * kVaeMaxZ; ++c) v[c] = c < C2 ? h[(b * C2 + c) * HW + p] : 0.f;
#pragma unroll
  for (int co = 0; co < 2 * kVaeMaxZ; ++co) {
    float acc = v[co];
    if (w && co < C2) {
      acc = 0.f;
#pragma unroll
      for (int c = 0; c < 2 * kVaeMaxZ; ++c)
        if (c < C2) acc = acc + w[co * C2 + c] * v[c];
      acc = acc + bias[co];
    }
    m[co] = acc;
  }
#pragma unroll
  for (int c = 0; c < kVaeMaxZ; ++c) {
    if (c >= ZC) break;
    float mean = 0.f, lv = 0.f;
#pragma unroll
    for (int k = 0; k < 2 * kVaeMaxZ; ++k) {  // (compile-time indices: m stays in registers)
      if (k == c) mean = m[k];
      if (k == ZC + c) lv = m[k];
    }
    lv = fminf(fmaxf(lv, -30.0f), 20.0f);
    float zz = mean;
    if (noise) zz = mean + expf(0.5f * lv) * noise[(b * ZC + c) * HW + p];
    z[(b * ZC + c) * HW + p] = scale * zz;
    if (mom) {
      mom[(b * C2 + c) * HW + p] = mean;
      mom[(b * C2 + ZC + c) * HW + p] = lv;
    }
  }
}

using vaeb::AttnW;
using vaeb::ConvW;
using vaeb::GnW;
using vaeb::ResW;
struct EncLevelW {
  std::vector<ResW> blocks;
  bool has_down = false;
  ConvW down;
};

}  // namespace

struct VaeEncoder : ExecNet {
  dm_vae_enc_arch arch;
  size_t in_w = 0, in_b = 0;  // conv_in, torch layout [ch][in_channels][3][3]
  std::vector<EncLevelW> levels;
  ResW mid1, mid2;
  AttnW attn;
  GnW out_gn;
  size_t out_w = 0, out_b = 0;
  size_t q_w = 0, q_b = 0;  // quant_conv [2 zc][2 zc], [2 zc]
  int c_top = 0;

  struct Plan : PlanBase {
    int B = 0, H = 0, W = 0, math = 0;
    float* x = nullptr;  // staged input, NCHW
    float* h = nullptr;  // conv_out's output [B][2 zc][H / f][W / f], NCHW
  };
  PlanCache<Plan> plans;
  float* out_packed = nullptr;  // conv_out weights as [9][C][CO] (small_out_pack)
  ~VaeEncoder() {
    if (out_packed) (void)hipFree(out_packed);
  }
  int build_plan(Plan& pl, int B, int H, int W);
  int get_plan(int B, int H, int W, int math, Plan** out) {
    conv_math = math;
    return plans.get([&](const Plan& p) { return p.B == B && p.H == H && p.W == W && p.math == math; },
                     [&](Plan& p) { return build_plan(p, B, H, W); }, out);
  }
};

static int vae_enc_validate(const dm_vae_enc_arch* a) {
  DM_REQUIRE(a != nullptr, "arch is null");
  DM_REQUIRE(a->n_levels >= 1 && a->n_levels <= DM_MAX_STAGES, "n_levels out of range");
  DM_REQUIRE(a->in_channels >= 1 && a->in_channels <= 4, "in_channels out of range (1..4)");
  DM_REQUIRE(a->z_channels >= 1 && a->z_channels <= 4, "z_channels out of range (1..4)");
  DM_REQUIRE(a->num_res_blocks >= 1, "num_res_blocks must be >= 1");
  DM_REQUIRE(a->norm_groups == 32, "norm_groups must be 32");
  DM_REQUIRE(a->norm_eps > 0.f, "norm_eps must be positive");
  DM_REQUIRE(a->ch >= 32 && a->ch % 32 == 0, "ch must be a positive multiple of 32");
  for (int i = 0; i < a->n_levels; ++i) {
    DM_REQUIRE(a->ch_mult[i] >= 1, "ch_mult must be >= 1");
    DM_REQUIRE((a->ch * a->ch_mult[i]) % 32 == 0 && a->ch * a->ch_mult[i] <= 1024,
               "level channels must be multiples of 32 (GroupNorm(32) / MFMA tiles), at most 1024");
  }
  return DM_OK;
}

static int vae_enc_count_params(const dm_vae_enc_arch& a) {
  auto rb = [](int cin, int cout) { return 8 + (cin != cout ? 2 : 0); };
  int n = 2;  // conv_in
  int cur = a.ch;
  for (int i = 0; i < a.n_levels; ++i) {
    const int out = a.ch * a.ch_mult[i];
    for (int j = 0; j < a.num_res_blocks; ++j) {
      n += rb(cur, out);
      cur = out;
    }
    if (i != a.n_levels - 1) n += 2;
  }
  n += 2 * rb(cur, cur) + 10;  // mid.block_1, mid.attn_1 (norm, q, k, v, proj_out), mid.block_2
  n += 4;                      // norm_out, conv_out
  if (a.quant) n += 2;
  return n;
}

static int vae_enc_create(const dm_vae_enc_arch* arch, const float* const* params, const int64_t* numels, int n_params,
                          hipStream_t st, VaeEncoder** out) {
  int rc = vae_enc_validate(arch);
  if (rc) return rc;
  const dm_vae_enc_arch a = *arch;
  const int expect = vae_enc_count_params(a);
  DM_REQUIRE(n_params == expect,
             "expected " + std::to_string(expect) + " parameter tensors, got " + std::to_string(n_params));
  refresh_toggles();
  auto m = std::make_unique<VaeEncoder>();
  m->arch = a;
  ParamReader rd{params, numels, n_params};
  Packer pk;
  vaeb::BlockReader br{rd, pk};
  const int zc = a.z_channels, L = a.n_levels, ic = a.in_channels;

  m->in_w = pk.raw(rd.take((int64_t)a.ch * ic * 9, "conv_in.weight"), (int64_t)a.ch * ic * 9);
  m->in_b = pk.raw(rd.take(a.ch, "conv_in.bias"), a.ch);
  // encoder.down.{i}: level i's first block takes the previous level's channels (ch at level 0; autoencoder.py:303-326)
  m->levels.resize(L);
  int cur = a.ch;
  for (int i = 0; i < L; ++i) {
    const int cout = a.ch * a.ch_mult[i];
    for (int j = 0; j < a.num_res_blocks; ++j) {
      m->levels[i].blocks.push_back(br.resblock(cur, cout));
      cur = cout;
    }
    if (i != L - 1) {
      m->levels[i].has_down = true;
      m->levels[i].down = br.conv3x3(cur, cur, "Downsample.conv.weight", "Downsample.conv.bias");
    }
  }
  m->c_top = cur;
  m->mid1 = br.resblock(cur, cur);
  m->attn = br.attn(cur);
  m->mid2 = br.resblock(cur, cur);
  m->out_gn = br.gn(cur, "norm_out");
  m->out_w = pk.raw(rd.take((int64_t)2 * zc * cur * 9, "conv_out.weight"), (int64_t)2 * zc * cur * 9);
  m->out_b = pk.raw(rd.take(2 * zc, "conv_out.bias"), 2 * zc);
  if (a.quant) {
    m->q_w = pk.raw(rd.take((int64_t)4 * zc * zc, "quant_conv.weight"), (int64_t)4 * zc * zc);
    m->q_b = pk.raw(rd.take(2 * zc, "quant_conv.bias"), 2 * zc);
  }
  if (!rd.err.empty()) {
    set_error(rd.err);
    return DM_ERR_ARG;
  }
  DM_REQUIRE(rd.pos == n_params, "parameter count mismatch after walk");
  m->arena_floats = pk.size;
  DM_CHECK_HIP(hipMalloc(&m->arena, pk.size * sizeof(float)));
  rc = run_pack_jobs(pk, m->arena, st);
  if (rc) return rc;
  *out = m.release();
  return DM_OK;
}

// ---------------------------------------------------------------------------
// plan (per batch size / image resolution / arithmetic)
// ---------------------------------------------------------------------------
int VaeEncoder::build_plan(Plan& pl, int B, int H, int W) {
  refresh_toggles();
  pl.toggles = toggles();
  ToggleScope scope(pl.toggles);
  pl.graph_enabled = toggles().graph;
  pl.B = B;
  pl.H = H;
  pl.W = W;
  pl.math = conv_math;
  if (const int rcf = ensure_range_flag()) return rcf;
  const int G = arch.norm_groups, zc = arch.z_channels, L = arch.n_levels, ic = arch.in_channels, ch = arch.ch;
  const float eps = arch.norm_eps;
  const int f = 1 << (L - 1);
  DM_REQUIRE(H % f == 0 && W % f == 0, "encoder plan: H and W must be multiples of 2^(n_levels - 1)");
  DM_REQUIRE((long)B * H * W < (1L << 31), "encoded batch too large: encode in smaller batches");
  const int h0 = H / f, w0 = W / f;

  // --- staging and the five activation buffers (each takes the largest tensor of the network)
  pl.x = pl.alloc((size_t)B * ic * H * W * 4);
  pl.h = pl.alloc((size_t)B * 2 * zc * h0 * w0 * 4);
  size_t max_t = (size_t)H * W * ch;
  int max_chunks = gn_num_chunks(H * W), max_c = ch;
  for (int i = 0; i < L; ++i) {
    const size_t hw = (size_t)(H >> i) * (W >> i);
    const int cout = ch * arch.ch_mult[i];
    const int cin = levels[i].blocks[0].cin;
    max_t = std::max(max_t, hw * std::max(cin, cout));
    max_chunks = std::max(max_chunks, gn_num_chunks((int)hw));
    max_c = std::max(max_c, std::max(cin, cout));
  }
  vaeb::BlockPlanner bp(this, pl, B, G, eps);
  bp.alloc(max_t, max_chunks, max_c, h0 * w0, attn.C);
  Plan* P_ = &pl;

  // --- conv_in on conv3x3_small_in (NCHW input, <= 4 channels), in slices of <= 128 output channels as the decoder's;
  // a single slice also emits the first ResnetBlock's GroupNorm statistics where the kernel can
  View x{bp.bufs[0], B, H, W, ch, ch};
  {
    double2* gp = nullptr;
    if (ch <= 128 && toggles().gn_fusion && conv3x3_small_in_can_emit(H, W, ch, G)) {
      gp = bp.emit_parts[bp.emit_next];
      bp.emit_next ^= 1;
      bp.gn_ready[x.p] = {gp, ch};
    }
    for (int c0 = 0; c0 < ch; c0 += 128) {
      const int cn = std::min(128, ch - c0);
      const float* w = P(in_w) + (size_t)c0 * ic * 9;
      const float* bb = P(in_b) + c0;
      const View ys{x.p + c0, B, H, W, cn, ch};
      pl.add("conv3x3_small_in", 2.0 * B * H * W * cn * 9 * ic, 4.0 * B * H * W * (ic + cn),
             [=](hipStream_t st) { return conv3x3_small_in(P_->x, B, ic, H, W, w, bb, cn, ys, st, gp, gp ? G : 0); });
    }
  }

  // --- levels, from the highest resolution downward
  for (int i = 0; i < L; ++i) {
    for (const ResW& r : levels[i].blocks) x = bp.resblock(r, x);
    if (!levels[i].has_down) continue;
    // Downsample (autoencoder.py:47-66): pad (0, 1, 0, 1), 3x3 stride 2 -- taps from 2o (s2_pad0); no prologue (the
    // block's output goes in as it is); the epilogue emits the next block's GroupNorm statistics where the tile can
    const ConvW cv = levels[i].down;
    View y{bp.next_buf(), B, x.H / 2, x.W / 2, cv.Cout, cv.Cout};
    ConvArgs c{};
    c.x1 = x.p; c.x1_pitch = x.pitch; c.Cin1 = cv.Cin; c.Hin = x.H; c.Win = x.W;
    c.taps = 9; c.stride = 2; c.s2_pad0 = 1;
    c.w = P(cv.w); c.K = cv.K;
    c.y = y.p; c.y_pitch = y.pitch; c.Cout = cv.Cout; c.B = B; c.pick_B = kPickBatch; c.Hout = y.H; c.Wout = y.W;
    c.bias = P(cv.bias);
    bp.emit_conv(c, y);
    bp.add_conv(c);
    x = y;
  }

  // --- middle
  x = bp.resblock(mid1, x);
  x = bp.attn_block(attn, x);
  x = bp.resblock(mid2, x);

  // --- exit: norm_out -> SiLU -> conv_out (2 zc channels), NCHW store
  {
    const View xin = x;
    const int C = xin.C, oc = 2 * zc;
    DM_REQUIRE(xin.H == h0 && xin.W == w0 && C == c_top, "encoder plan: output shape");
    const int nchunk = gn_num_chunks(h0 * w0);
    const GnW lg = out_gn;
    const double2* stl = bp.gn_stats(xin);
    float *gsc = bp.gsc, *gsh = bp.gsh;
    const float *gamma = P(lg.g), *beta = P(lg.b);
    GnFin fin;
    if (toggles().gn_fusion && C <= 512 && C % G == 0 && nchunk <= 64) {
      fin.part = stl; fin.G = G; fin.nchunk = nchunk; fin.n = (double)h0 * w0 * (C / G); fin.eps = eps;
      fin.gamma = gamma; fin.beta = beta;
    } else {
      pl.add("gn_finalize", 0, 8.0 * B * C,
             [=](hipStream_t st) { return gn_finalize(xin, G, stl, eps, gamma, beta, gsc, gsh, st); });
    }
    if (!out_packed) {
      DM_CHECK_HIP(hipMalloc(&out_packed, (size_t)9 * C * 8 * sizeof(float)));
      DM_REQUIRE(small_out_pack(P(out_w), oc, C, out_packed, nullptr) == DM_OK, "conv_out: weight packing failed");
      DM_CHECK_HIP(hipDeviceSynchronize());
    }
    const float* lw = out_packed;
    const float* lb = P(out_b);
    pl.add("conv3x3_small_out", 2.0 * B * h0 * w0 * oc * 9 * C, 4.0 * B * h0 * w0 * (C + oc), [=](hipStream_t st) {
      return fin.part ? conv3x3_small_out(xin, lw, lb, oc, P_->h, st, nullptr, nullptr, fin)
                      : conv3x3_small_out(xin, lw, lb, oc, P_->h, st, gsc, gsh);
    });
  }
  return DM_OK;
}

}  // namespace dm

// ===========================================================================
// C ABI
// ===========================================================================
struct dm_vae_encoder {
  dm::VaeEncoder* m;
};

extern "C" int dm_vae_encoder_param_count(const dm_vae_enc_arch* arch, int* n_params) {
  const int rc = dm::vae_enc_validate(arch);
  if (rc) return rc;
  if (!n_params) { dm::set_error("n_params is null"); return DM_ERR_ARG; }
  *n_params = dm::vae_enc_count_params(*arch);
  return DM_OK;
}

extern "C" int dm_vae_encoder_create(const dm_vae_enc_arch* arch, const float* const* params, const int64_t* numels,
                                     int n_params, void* stream, dm_vae_encoder** out) {
  if (!out || !params || !numels) { dm::set_error("null argument"); return DM_ERR_ARG; }
  dm::VaeEncoder* m = nullptr;
  const int rc = dm::vae_enc_create(arch, params, numels, n_params, (hipStream_t)stream, &m);
  if (rc) return rc;
  *out = new dm_vae_encoder{m};
  return DM_OK;
}

extern "C" int dm_vae_encoder_forward(dm_vae_encoder* e, const float* x, int B, int H, int W, const float* noise,
                                      float scale, float* z_out, float* moments_out, void* stream) {
  dm::VaeEncoder* m = dm::model_of(e);
  DM_ABI_MODEL(m);
  if (!x || !z_out) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  if (B <= 0 || H <= 0 || W <= 0) { dm::set_error("empty batch or image"); return DM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const int f = 1 << (m->arch.n_levels - 1);
  if (H % f != 0 || W % f != 0) {
    dm::set_error("image H and W must be multiples of " + std::to_string(f) + " (2^(n_levels - 1)), got " +
                  std::to_string(H) + " x " + std::to_string(W));
    return DM_ERR_ARG;
  }
  const int h0 = H / f, w0 = W / f;
  // the middle attention's score rows (L = h w floats) are read as 16-byte vectors by the GEMMs
  if (((long)h0 * w0) % 4 != 0) {
    dm::set_error("latent H x W must be a multiple of 4 (the middle attention's score rows)");
    return DM_ERR_UNSUPPORTED;
  }
  if ((long)B * H * W >= (1L << 31)) {
    dm::set_error("encoded batch too large: encode in smaller batches");
    return DM_ERR_ARG;
  }
  const int zc = m->arch.z_channels;
  const size_t nx = (size_t)B * m->arch.in_channels * H * W;
  using Plan = dm::VaeEncoder::Plan;
  return dm::run_forward(
      *m, st, [&](int math, Plan** pl) { return m->get_plan(B, H, W, math, pl); },
      [&](Plan& pl) {
        DM_CHECK_HIP(hipMemcpyAsync(pl.x, x, nx * sizeof(float), hipMemcpyDeviceToDevice, st));
        return DM_OK;
      },
      [&](Plan& pl) {
        // the posterior, on the caller's buffers (a fallback pass writes them again)
        const long hw = (long)h0 * w0, n = (long)B * hw;
        const float* qw = m->arch.quant ? m->P(m->q_w) : nullptr;
        const float* qb = m->arch.quant ? m->P(m->q_b) : nullptr;
        hipLaunchKernelGGL(dm::vae_moments_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pl.h, zc, hw, n,
                           qw, qb, noise, scale, z_out, moments_out);
        DM_LAUNCH_CHECK();
        return DM_OK;
      });
}

extern "C" int dm_vae_encoder_range_stats(const dm_vae_encoder* e, int64_t* fallbacks, int* active) {
  return dm::abi_range_stats(dm::model_of(e), fallbacks, active);
}
extern "C" int dm_vae_encoder_memory(const dm_vae_encoder* e, int64_t* weight_bytes, int64_t* workspace_bytes) {
  return dm::abi_memory(dm::model_of(e), weight_bytes, workspace_bytes);
}
extern "C" int dm_vae_encoder_plan_stats(const dm_vae_encoder* e, int64_t* builds, int* cached) {
  return dm::abi_plan_stats(dm::model_of(e), builds, cached);
}
extern "C" int dm_vae_encoder_set_math(dm_vae_encoder* e, int kind) {
  return dm::abi_set_math(dm::model_of(e), kind, true);
}
extern "C" int dm_vae_encoder_get_math(const dm_vae_encoder* e, int* kind) {
  if (dm::model_of(e) && !kind) { dm::set_error("kind is null"); return DM_ERR_ARG; }
  return dm::abi_get_math(dm::model_of(e), kind);
}
extern "C" int dm_vae_encoder_profile(dm_vae_encoder* e, int enable) {
  return dm::abi_profile(dm::model_of(e), enable);
}
extern "C" int dm_vae_encoder_profile_count(dm_vae_encoder* e, int* n_ops) {
  return dm::abi_profile_count(dm::model_of(e), n_ops);
}
extern "C" int dm_vae_encoder_profile_get(dm_vae_encoder* e, int i, char* label, int label_len, double* flops,
                                          double* bytes, double* ms_total, int64_t* launches) {
  return dm::abi_profile_get(dm::model_of(e), i, label, label_len, flops, bytes, ms_total, launches);
}
extern "C" void dm_vae_encoder_destroy(dm_vae_encoder* e) { dm::abi_destroy(e); }
