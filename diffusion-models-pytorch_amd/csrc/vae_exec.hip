// Native executor for the latent decoder of the KL autoencoder (reference
// models/stablediffusion/autoencoder.py: Decoder :376-483, AutoEncoderKL.decode :522-525; the network the
// reference's DiT wraps as diffusers' AutoencoderKL, models/dit/autoencoder.py).
//
// Forward: scale * z -> post_quant_conv (1x1) -> conv_in -> mid.block_1 -> mid.attn_1 -> mid.block_2 -> per
// level from the lowest resolution upward (num_res_blocks + 1) ResnetBlocks and, except at level 0, Upsample
// (nearest-2x + 3x3 conv) -> norm_out -> SiLU -> conv_out. No time embedding, no skips.
//
// Build time (dm_vae_decoder_create): the state_dict tensors (decoder.* in registration order, then
// post_quant_conv.*) are packed as the UNet executor packs its own (exec_pack.h): 3x3 convs -> [Cout][K]; a
// ResnetBlock's nin_shortcut is the second K segment of its conv2 (bias b2 + bs); q, k, v -> one [3C][C] weight;
// upsample convs also in the sub-pixel form. The plan (per (B, H, W) and arithmetic) runs over five activation
// buffers sized to the largest tensor of the network, reused by every level (a level's tensors die at its upsample).
// The ResnetBlock / attention weights and plan builders are vae_blocks.h's, shared with the encoder
// (vae_enc_exec.hip); the arithmetic state, the forward driver and the ABI bodies are exec_core.h's.
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

// Latent entry: zq[b][co][p] = bias[co] + sum_c w[co][c] * (scale * z[b][c][p]), NCHW planes (conv_in's
// conv3x3_small_in reads NCHW). scale * z first, as the reference's `1. / scale_factor * z` (models/dit/dit.py
// decode_latent), then the 1x1 post_quant_conv in channel order with separately rounded products. w == null: the
// scaling alone. post_quant_conv is not folded into conv_in's weights: its bias does not pass through conv_in's zero
// padding, so the border pixels would differ.
constexpr int kVaeMaxZ = 4;  // z_channels <= 4 (conv3x3_small_in's input channels)
__global__ void vae_latent_in_kernel(const float* __restrict__ z, int ZC, long HW, long n, float scale,
                                     const float* __restrict__ w, const float* __restrict__ bias,
                                     float* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (b, p)
  if (i >= n) return;
  const long b = i / HW, p = i - b * HW;
  float v[kVaeMaxZ];
#pragma unroll
  for (int c = 0; c < kVaeMaxZ; ++c) v[c] = c < ZC ? scale * z[(b * ZC + c) * HW + p] : 0.f;
#pragma unroll
  for (int co = 0; co < kVaeMaxZ; ++co) {
    if (co >= ZC) break;
    float acc = v[co];
    if (w) {
      acc = 0.f;
#pragma unroll
      for (int c = 0; c < kVaeMaxZ; ++c)
        if (c < ZC) acc = acc + w[co * ZC + c] * v[c];
      acc = acc + bias[co];
    }
    out[(b * ZC + co) * HW + p] = acc;
  }
}

using vaeb::AttnW;
using vaeb::ConvW;
using vaeb::GnW;
using vaeb::ResW;
struct LevelW {
  std::vector<ResW> blocks;
  bool has_up = false;
  ConvW up;
};

}  // namespace

struct VaeDecoder : ExecNet {
  dm_vae_arch arch;
  size_t pq_w = 0, pq_b = 0;  // post_quant_conv [zc][zc], [zc]
  size_t in_w = 0, in_b = 0;  // conv_in, torch layout [C][zc][3][3]
  ResW mid1, mid2;
  AttnW attn;
  std::vector<LevelW> levels;  // index = i_level (0: the highest resolution)
  GnW out_gn;
  size_t out_w = 0, out_b = 0;
  int c_top = 0, c_out = 0;    // channels at the latent resolution / before conv_out

  struct Plan : PlanBase {
    int B = 0, H = 0, W = 0, math = 0;
    float scale = 1.f;
    float* z = nullptr;    // staged input, NCHW
    float* out = nullptr;  // staged output, NCHW
  };
  PlanCache<Plan> plans;
  float* out_packed = nullptr;  // conv_out weights as [9][C][CO] (small_out_pack)
  // (the weight arena, the arithmetic and the fp16 range fallback: ExecNet)
  ~VaeDecoder() {
    if (out_packed) (void)hipFree(out_packed);
  }
  int build_plan(Plan& pl, int B, int H, int W);
  int get_plan(int B, int H, int W, int math, Plan** out) {
    conv_math = math;
    return plans.get([&](const Plan& p) { return p.B == B && p.H == H && p.W == W && p.math == math; },
                     [&](Plan& p) { return build_plan(p, B, H, W); }, out);
  }
};

static int vae_validate(const dm_vae_arch* a) {
  DM_REQUIRE(a != nullptr, "arch is null");
  DM_REQUIRE(a->n_levels >= 1 && a->n_levels <= DM_MAX_STAGES, "n_levels out of range");
  DM_REQUIRE(a->z_channels >= 1 && a->z_channels <= 4, "z_channels out of range (1..4)");
  DM_REQUIRE(a->out_channels >= 1 && a->out_channels <= 8, "out_channels out of range (1..8)");
  DM_REQUIRE(a->num_res_blocks >= 0, "num_res_blocks must be >= 0");
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

static int vae_count_params(const dm_vae_arch& a) {
  auto rb = [](int cin, int cout) { return 8 + (cin != cout ? 2 : 0); };
  int n = 2;  // conv_in
  int cur = a.ch * a.ch_mult[a.n_levels - 1];
  n += 2 * rb(cur, cur) + 10;  // mid.block_1, mid.attn_1 (norm, q, k, v, proj_out), mid.block_2
  for (int i = a.n_levels - 1; i >= 0; --i) {
    const int out = a.ch * a.ch_mult[i];
    for (int j = 0; j < a.num_res_blocks + 1; ++j) {
      n += rb(cur, out);
      cur = out;
    }
    if (i != 0) n += 2;
  }
  n += 4;  // norm_out, conv_out
  if (a.post_quant) n += 2;
  return n;
}

static int vae_create(const dm_vae_arch* arch, const float* const* params, const int64_t* numels, int n_params,
                      hipStream_t st, VaeDecoder** out) {
  int rc = vae_validate(arch);
  if (rc) return rc;
  const dm_vae_arch a = *arch;
  const int expect = vae_count_params(a);
  DM_REQUIRE(n_params == expect,
             "expected " + std::to_string(expect) + " parameter tensors, got " + std::to_string(n_params));
  refresh_toggles();
  auto m = std::make_unique<VaeDecoder>();
  m->arch = a;
  ParamReader rd{params, numels, n_params};
  Packer pk;
  const int zc = a.z_channels, L = a.n_levels;
  const int ctop = a.ch * a.ch_mult[L - 1];
  m->c_top = ctop;

  vaeb::BlockReader br{rd, pk};
  m->in_w = pk.raw(rd.take((int64_t)ctop * zc * 9, "conv_in.weight"), (int64_t)ctop * zc * 9);
  m->in_b = pk.raw(rd.take(ctop, "conv_in.bias"), ctop);
  m->mid1 = br.resblock(ctop, ctop);
  m->attn = br.attn(ctop);
  m->mid2 = br.resblock(ctop, ctop);
  // decoder.up.{i}: registered from i = 0 (the highest resolution), run from i = L - 1; level i's first block
  // takes the channels of level i + 1 (autoencoder.py:422-440)
  m->levels.resize(L);
  for (int i = 0; i < L; ++i) {
    const int cout = a.ch * a.ch_mult[i];
    int cin = i == L - 1 ? ctop : a.ch * a.ch_mult[i + 1];
    for (int j = 0; j < a.num_res_blocks + 1; ++j) {
      m->levels[i].blocks.push_back(br.resblock(cin, cout));
      cin = cout;
    }
    if (i != 0) {
      ConvW& c = m->levels[i].up;
      m->levels[i].has_up = true;
      const float* w = rd.take((int64_t)cout * cout * 9, "Upsample.conv.weight");
      const float* b = rd.take(cout, "Upsample.conv.bias");
      c.Cout = cout; c.Cin = cout; c.K = 9 * cout;
      c.w = pk.reserve((int64_t)cout * 9 * cout);
      pk.conv_at(w, cout, cout, 9, 9 * cout, 0, c.w);
      c.bias = pk.raw(b, cout);
      c.w_sub = pk.subpix(w, cout, cout);
    }
  }
  const int c0 = a.ch * a.ch_mult[0];
  m->c_out = c0;
  m->out_gn = br.gn(c0, "norm_out");
  m->out_w = pk.raw(rd.take((int64_t)a.out_channels * c0 * 9, "conv_out.weight"), (int64_t)a.out_channels * c0 * 9);
  m->out_b = pk.raw(rd.take(a.out_channels, "conv_out.bias"), a.out_channels);
  if (a.post_quant) {
    m->pq_w = pk.raw(rd.take((int64_t)zc * zc, "post_quant_conv.weight"), (int64_t)zc * zc);
    m->pq_b = pk.raw(rd.take(zc, "post_quant_conv.bias"), zc);
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
// plan (per batch size / latent resolution / arithmetic)
// ---------------------------------------------------------------------------
int VaeDecoder::build_plan(Plan& pl, int B, int H, int W) {
  refresh_toggles();
  pl.toggles = toggles();
  ToggleScope scope(pl.toggles);
  pl.graph_enabled = toggles().graph;
  pl.B = B;
  pl.H = H;
  pl.W = W;
  pl.math = conv_math;
  if (const int rcf = ensure_range_flag()) return rcf;
  const int G = arch.norm_groups, zc = arch.z_channels, L = arch.n_levels, oc = arch.out_channels;
  const float eps = arch.norm_eps;
  const int Hout = H << (L - 1), Wout = W << (L - 1);
  DM_REQUIRE((long)B * Hout * Wout < (1L << 31), "decoded batch too large: decode in smaller batches");
  auto Hl = [&](int lvl) { return H << (L - 1 - lvl); };
  auto Wl = [&](int lvl) { return W << (L - 1 - lvl); };

  // --- staging and the five activation buffers (each takes the largest tensor of the network: a level's block
  // tensors, and the upsample conv's output at the next resolution with this level's channels)
  pl.z = pl.alloc((size_t)B * zc * H * W * 4);
  pl.out = pl.alloc((size_t)B * oc * Hout * Wout * 4);
  float* zq = pl.alloc((size_t)B * zc * H * W * 4);
  size_t max_t = (size_t)H * W * c_top;
  int max_chunks = gn_num_chunks(H * W), max_c = c_top;
  for (int i = 0; i < L; ++i) {
    const size_t hw = (size_t)Hl(i) * Wl(i);
    const int cout = arch.ch * arch.ch_mult[i];
    const int cin = levels[i].blocks[0].cin;
    max_t = std::max(max_t, hw * std::max(cin, cout));
    if (i + 1 < L) max_t = std::max(max_t, hw * (size_t)(arch.ch * arch.ch_mult[i + 1]));  // the upsample's output
    max_chunks = std::max(max_chunks, gn_num_chunks((int)hw));
    max_c = std::max(max_c, std::max(cin, cout));
  }
  // the activation buffers and the block builders (vae_blocks.h)
  vaeb::BlockPlanner bp(this, pl, B, G, eps);
  bp.alloc(max_t, max_chunks, max_c, H * W, attn.C);
  float* const* bufs = bp.bufs;
  float *gsc = bp.gsc, *gsh = bp.gsh;
  Plan* P_ = &pl;

  // --- latent entry: scale, post_quant_conv
  {
    const float* w = arch.post_quant ? P(pq_w) : nullptr;
    const float* bb = arch.post_quant ? P(pq_b) : nullptr;
    const long hw = (long)H * W, n = (long)B * hw;
    pl.add("vae_latent_in_kernel", 2.0 * n * zc * zc, 8.0 * n * zc, [=](hipStream_t st) {
      hipLaunchKernelGGL(vae_latent_in_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P_->z, zc, hw, n,
                         P_->scale, w, bb, zq);
      DM_LAUNCH_CHECK();
      return DM_OK;
    });
  }
  // --- conv_in on conv3x3_small_in, in slices of <= 128 output channels (the kernel keeps a slice's weights in LDS;
  // 512 x 36 floats do not fit), each slice the kernel's own arithmetic for its channels
  View x{bufs[0], B, H, W, c_top, c_top};
  for (int c0 = 0; c0 < c_top; c0 += 128) {
    const int cn = std::min(128, c_top - c0);
    const float* w = P(in_w) + (size_t)c0 * zc * 9;
    const float* bb = P(in_b) + c0;
    const View ys{x.p + c0, B, H, W, cn, c_top};
    pl.add("conv3x3_small_in", 2.0 * B * H * W * cn * 9 * zc, 4.0 * B * H * W * (zc + cn),
        [=](hipStream_t st) { return conv3x3_small_in(zq, B, zc, H, W, w, bb, cn, ys, st); });
  }

  // --- middle
  x = bp.resblock(mid1, x);
  x = bp.attn_block(attn, x);  // mid.attn_1
  x = bp.resblock(mid2, x);

  // --- levels, from the lowest resolution upward
  for (int i = L - 1; i >= 0; --i) {
    for (const ResW& r : levels[i].blocks) x = bp.resblock(r, x);
    if (!levels[i].has_up) continue;
    const ConvW cv = levels[i].up;
    View y{bp.next_buf(), B, 2 * x.H, 2 * x.W, cv.Cout, cv.Cout};
    ConvArgs c{};
    c.x1 = x.p; c.x1_pitch = x.pitch; c.Cin1 = cv.Cin; c.Hin = x.H; c.Win = x.W;
    c.taps = 9; c.stride = 1; c.upsample = 1;
    c.w = P(cv.w); c.K = cv.K;
    c.y = y.p; c.y_pitch = y.pitch; c.Cout = cv.Cout; c.B = B; c.pick_B = kPickBatch; c.Hout = y.H; c.Wout = y.W;
    c.bias = P(cv.bias);
    {
      // the sub-pixel form (4 / 9 of the MFMA work) where its low-res shape tiles
      ConvArgs s = c;
      s.upsample = 2; s.w = P(cv.w_sub); s.K = 4 * c.Cin1;
      split_for(s);
      if (conv_choose(s).takes_prologue) c = s;
    }
    if (c.upsample == 2)
      bp.emit_conv(c, y);
    else
      bp.gn_ready.erase(y.p);
    bp.add_conv(c);
    x = y;
  }

  // --- image exit: norm_out -> SiLU -> conv_out, NCHW store
  {
    const View xin = x;
    const int C = xin.C;
    DM_REQUIRE(xin.H == Hout && xin.W == Wout && C == c_out, "decoder plan: output shape");
    const int nchunk = gn_num_chunks(Hout * Wout);
    const GnW lg = out_gn;
    const double2* stl = bp.gn_stats(xin);
    const float *gamma = P(lg.g), *beta = P(lg.b);
    GnFin fin;
    if (toggles().gn_fusion && C <= 512 && C % G == 0 && nchunk <= 64) {
      fin.part = stl; fin.G = G; fin.nchunk = nchunk; fin.n = (double)Hout * Wout * (C / G); fin.eps = eps;
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
    pl.add("conv3x3_small_out", 2.0 * B * Hout * Wout * oc * 9 * C, 4.0 * B * Hout * Wout * (C + oc),
        [=](hipStream_t st) {
          return fin.part ? conv3x3_small_out(xin, lw, lb, oc, P_->out, st, nullptr, nullptr, fin)
                          : conv3x3_small_out(xin, lw, lb, oc, P_->out, st, gsc, gsh);
        });
  }
  return DM_OK;
}

}  // namespace dm

// ===========================================================================
// C ABI
// ===========================================================================
struct dm_vae_decoder {
  dm::VaeDecoder* m;
};

extern "C" int dm_vae_decoder_param_count(const dm_vae_arch* arch, int* n_params) {
  const int rc = dm::vae_validate(arch);
  if (rc) return rc;
  if (!n_params) { dm::set_error("n_params is null"); return DM_ERR_ARG; }
  *n_params = dm::vae_count_params(*arch);
  return DM_OK;
}

extern "C" int dm_vae_decoder_create(const dm_vae_arch* arch, const float* const* params, const int64_t* numels,
                                     int n_params, void* stream, dm_vae_decoder** out) {
  if (!out || !params || !numels) { dm::set_error("null argument"); return DM_ERR_ARG; }
  dm::VaeDecoder* m = nullptr;
  const int rc = dm::vae_create(arch, params, numels, n_params, (hipStream_t)stream, &m);
  if (rc) return rc;
  *out = new dm_vae_decoder{m};
  return DM_OK;
}

extern "C" int dm_vae_decoder_forward(dm_vae_decoder* h, const float* z, int B, int H, int W, float scale, float* out,
                                      void* stream) {
  dm::VaeDecoder* m = dm::model_of(h);
  DM_ABI_MODEL(m);
  if (!z || !out) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  if (B <= 0 || H <= 0 || W <= 0) { dm::set_error("empty batch or latent"); return DM_ERR_ARG; }
  if (static_cast<const void*>(out) == static_cast<const void*>(z)) {
    dm::set_error("out must not alias z");
    return DM_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const int up = 1 << (m->arch.n_levels - 1);
  // the middle attention's score rows (L = H W floats) are read as 16-byte vectors by the GEMMs
  if (((long)H * W) % 4 != 0) {
    dm::set_error("latent H x W must be a multiple of 4 (the middle attention's score rows)");
    return DM_ERR_UNSUPPORTED;
  }
  if ((long)B * H * up * W * up >= (1L << 31)) {
    dm::set_error("decoded batch too large: decode in smaller batches");
    return DM_ERR_ARG;
  }
  const size_t nz = (size_t)B * m->arch.z_channels * H * W;
  const size_t no = (size_t)B * m->arch.out_channels * H * up * W * up;
  using Plan = dm::VaeDecoder::Plan;
  return dm::run_forward(
      *m, st, [&](int math, Plan** pl) { return m->get_plan(B, H, W, math, pl); },
      [&](Plan& pl) {
        if (pl.scale != scale) {  // the latent-entry launch reads the scale at capture time
          pl.scale = scale;
          pl.invalidate_graph();
        }
        DM_CHECK_HIP(hipMemcpyAsync(pl.z, z, nz * sizeof(float), hipMemcpyDeviceToDevice, st));
        return DM_OK;
      },
      [&](Plan& pl) {
        DM_CHECK_HIP(hipMemcpyAsync(out, pl.out, no * sizeof(float), hipMemcpyDeviceToDevice, st));
        return DM_OK;
      });
}

extern "C" int dm_vae_decoder_range_stats(const dm_vae_decoder* h, int64_t* fallbacks, int* active) {
  return dm::abi_range_stats(dm::model_of(h), fallbacks, active);
}
extern "C" int dm_vae_decoder_memory(const dm_vae_decoder* h, int64_t* weight_bytes, int64_t* workspace_bytes) {
  return dm::abi_memory(dm::model_of(h), weight_bytes, workspace_bytes);
}
extern "C" int dm_vae_decoder_plan_stats(const dm_vae_decoder* h, int64_t* builds, int* cached) {
  return dm::abi_plan_stats(dm::model_of(h), builds, cached);
}
extern "C" int dm_vae_decoder_set_math(dm_vae_decoder* h, int kind) {
  return dm::abi_set_math(dm::model_of(h), kind, true);
}
extern "C" int dm_vae_decoder_get_math(const dm_vae_decoder* h, int* kind) {
  if (dm::model_of(h) && !kind) { dm::set_error("kind is null"); return DM_ERR_ARG; }
  return dm::abi_get_math(dm::model_of(h), kind);
}
extern "C" int dm_vae_decoder_profile(dm_vae_decoder* h, int enable) {
  return dm::abi_profile(dm::model_of(h), enable);
}
extern "C" int dm_vae_decoder_profile_count(dm_vae_decoder* h, int* n_ops) {
  return dm::abi_profile_count(dm::model_of(h), n_ops);
}
extern "C" int dm_vae_decoder_profile_get(dm_vae_decoder* h, int i, char* label, int label_len, double* flops,
                                          double* bytes, double* ms_total, int64_t* launches) {
  return dm::abi_profile_get(dm::model_of(h), i, label, label_len, flops, bytes, ms_total, launches);
}
extern "C" void dm_vae_decoder_destroy(dm_vae_decoder* h) { dm::abi_destroy(h); }
