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

struct GnW { size_t g, b; };
struct ConvW {
  size_t w = 0, bias = 0;
  int Cout = 0, Cin = 0, K = 0;
  size_t w_sub = 0;  // sub-pixel weights [4][Cout][4 Cin] of an upsample conv
};
struct ResW {
  int cin, cout;
  GnW gn1, gn2;
  ConvW conv1, conv2;  // conv2 carries nin_shortcut as its second K segment when cin != cout
};
struct AttnW {
  int C;
  GnW gn;
  size_t wqkv, bqkv, wproj, bproj;
};
struct LevelW {
  std::vector<ResW> blocks;
  bool has_up = false;
  ConvW up;
};

}  // namespace

struct VaeDecoder {
  dm_vae_arch arch;
  float* arena = nullptr;
  size_t arena_floats = 0;
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
  // arithmetic and the fp16 range fallback: as UNetModel (unet_exec.hip)
  int base_math = conv_math_from_env();
  int conv_math = base_math;
  bool range_check = toggles().range_check;
  int* range_flag = nullptr;
  int* range_flag_host = nullptr;
  long range_fallbacks = 0;
  std::map<std::pair<const float*, int>, void*> split_w;
  std::map<std::pair<const float*, int>, void*> wino_w;
  size_t split_bytes = 0;
  std::map<const float*, int> w_exp;

  float* P(size_t off) const { return arena + off; }
  ~VaeDecoder() {
    plans.clear();
    if (out_packed) (void)hipFree(out_packed);
    for (auto& kv : split_w) (void)hipFree(kv.second);
    for (auto& kv : wino_w) (void)hipFree(kv.second);
    if (range_flag) (void)hipFree(range_flag);
    if (range_flag_host) (void)hipHostFree(range_flag_host);
    if (arena) (void)hipFree(arena);
  }
  void split_for(ConvArgs& c);
  void split_gemm(GemmArgs& g, int ea, const float* weight, size_t weight_n, int eb_act);
  int build_plan(Plan& pl, int B, int H, int W);
  int get_plan(int B, int H, int W, int math, Plan** out) {
    conv_math = math;
    return plans.get([&](const Plan& p) { return p.B == B && p.H == H && p.W == W && p.math == math; },
                     [&](Plan& p) { return build_plan(p, B, H, W); }, out);
  }
};

// The split copy (and, for the shapes conv_wino takes, the Winograd weights) of a conv's packed weights, as
// UNetModel::split_for; none: the conv stays on the fp32 kernels.
void VaeDecoder::split_for(ConvArgs& c) {
  c.ws = nullptr;
  c.ws_np = 0;
  c.ws_rowscale = nullptr;
  c.range_flag = nullptr;
  c.wino_ws = nullptr;
  c.wino_rowscale = nullptr;
  if (!conv_math || !(conv_split_eligible(c) || (conv_math == 2 && conv_seg_eligible(c)))) return;
  if (c.taps == 1 && conv_math != 2) return;  // the split 1x1 path is fp16x2 only
  const int nmat = c.upsample == 2 ? 4 : 1;
  const int ntap = c.upsample == 2 ? 4 : c.taps;
  const auto key = std::make_pair(c.w, conv_math);
  auto it = split_w.find(key);
  void* p = nullptr;
  if (it != split_w.end()) {
    p = it->second;
  } else {
    const size_t nb = split_conv_weights_bytes(nmat, c.Cout, c.K, conv_math);
    if (hipMalloc(&p, nb) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    if (split_conv_weights(c.w, nmat, c.Cout, c.K, c.Cin1, ntap, conv_math, p, nullptr) != DM_OK ||
        hipDeviceSynchronize() != hipSuccess) {
      (void)hipFree(p);
      return;
    }
    split_w[key] = p;
    split_bytes += nb;
  }
  c.ws = p;
  c.ws_np = conv_math;
  if (conv_math == 2) {
    c.ws_rowscale = split_conv_rowscale(p, nmat, c.Cout, c.K);
    c.range_flag = range_flag;
  }
  if (conv_math != 2 || !toggles().wino || !conv_wino_shape_ok(c)) return;
  if (c.Wout == 4) return;  // (4-pixel-wide maps: the Winograd kernel there is a split-K form the UNet plans tune)
  const int fold = c.Cin2 && (c.pro_scale || c.gin_part) && !c.pro_nosilu ? 1 : 0;
  auto iw = wino_w.find(std::make_pair(c.w, fold));
  void* wp = nullptr;
  if (iw != wino_w.end()) {
    wp = iw->second;
  } else {
    const size_t nb = wino_weights_bytes(c.Cout, c.Cin1, c.Cin2);
    if (hipMalloc(&wp, nb) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    if (wino_weights(c.w, c.Cout, c.Cin1, c.Cin2, fold, wp, nullptr) != DM_OK) {
      (void)hipFree(wp);
      return;
    }
    wino_w[std::make_pair(c.w, fold)] = wp;
    split_bytes += nb;
  }
  c.wino_ws = wp;
  c.wino_rowscale = wino_rowscale(wp, c.Cout, c.Cin1, c.Cin2);
  c.wino_fold = fold;
}

// fp16x2 attention GEMMs: operand exponents (exec_pack.h split_gemm_args)
void VaeDecoder::split_gemm(GemmArgs& g, int ea, const float* weight, size_t weight_n, int eb_act) {
  split_gemm_args(g, conv_math, w_exp, range_flag, ea, weight, weight_n, eb_act);
}

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

  auto gn = [&](int C, const char* what) {
    GnW g;
    g.g = pk.raw(rd.take(C, what), C);
    g.b = pk.raw(rd.take(C, what), C);
    return g;
  };
  auto resblock = [&](int cin, int cout) {
    ResW r;
    r.cin = cin;
    r.cout = cout;
    r.gn1 = gn(cin, "ResnetBlock.norm1");
    const float* w1 = rd.take((int64_t)cout * cin * 9, "ResnetBlock.conv1.weight");
    const float* b1 = rd.take(cout, "ResnetBlock.conv1.bias");
    r.conv1.Cout = cout; r.conv1.Cin = cin; r.conv1.K = 9 * cin;
    r.conv1.w = pk.reserve((int64_t)cout * 9 * cin);
    pk.conv_at(w1, cout, cin, 9, 9 * cin, 0, r.conv1.w);
    r.conv1.bias = pk.raw(b1, cout);
    r.gn2 = gn(cout, "ResnetBlock.norm2");
    const float* w2 = rd.take((int64_t)cout * cout * 9, "ResnetBlock.conv2.weight");
    const float* b2 = rd.take(cout, "ResnetBlock.conv2.bias");
    const int K2 = 9 * cout + (cin != cout ? cin : 0);
    r.conv2.Cout = cout; r.conv2.Cin = cout; r.conv2.K = K2;
    r.conv2.w = pk.reserve((int64_t)cout * K2);
    pk.conv_at(w2, cout, cout, 9, K2, 0, r.conv2.w);
    if (cin != cout) {
      const float* ws = rd.take((int64_t)cout * cin, "ResnetBlock.nin_shortcut.weight");
      const float* bs = rd.take(cout, "ResnetBlock.nin_shortcut.bias");
      pk.conv_at(ws, cout, cin, 1, K2, 9 * cout, r.conv2.w);
      r.conv2.bias = pk.reserve(cout);
      pk.add_at(b2, bs, cout, r.conv2.bias);
    } else {
      r.conv2.bias = pk.raw(b2, cout);
    }
    return r;
  };

  m->in_w = pk.raw(rd.take((int64_t)ctop * zc * 9, "conv_in.weight"), (int64_t)ctop * zc * 9);
  m->in_b = pk.raw(rd.take(ctop, "conv_in.bias"), ctop);
  m->mid1 = resblock(ctop, ctop);
  {
    AttnW& p = m->attn;
    const int C = ctop;
    p.C = C;
    p.gn = gn(C, "AttnBlock.norm");
    p.wqkv = pk.reserve((int64_t)3 * C * C);
    p.bqkv = pk.reserve(3 * C);
    for (int i = 0; i < 3; ++i) {
      pk.raw_at(rd.take((int64_t)C * C, "AttnBlock.{q,k,v}.weight"), (int64_t)C * C, p.wqkv + (size_t)i * C * C);
      pk.raw_at(rd.take(C, "AttnBlock.{q,k,v}.bias"), C, p.bqkv + (size_t)i * C);
    }
    p.wproj = pk.raw(rd.take((int64_t)C * C, "AttnBlock.proj_out.weight"), (int64_t)C * C);
    p.bproj = pk.raw(rd.take(C, "AttnBlock.proj_out.bias"), C);
  }
  m->mid2 = resblock(ctop, ctop);
  // decoder.up.{i}: registered from i = 0 (the highest resolution), run from i = L - 1; level i's first block
  // takes the channels of level i + 1 (autoencoder.py:422-440)
  m->levels.resize(L);
  for (int i = 0; i < L; ++i) {
    const int cout = a.ch * a.ch_mult[i];
    int cin = i == L - 1 ? ctop : a.ch * a.ch_mult[i + 1];
    for (int j = 0; j < a.num_res_blocks + 1; ++j) {
      m->levels[i].blocks.push_back(resblock(cin, cout));
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
  m->out_gn = gn(c0, "norm_out");
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
  if (!range_flag) {
    DM_CHECK_HIP(hipMalloc(&range_flag, sizeof(int)));
    DM_CHECK_HIP(hipMemset(range_flag, 0, sizeof(int)));
    DM_CHECK_HIP(hipHostMalloc(&range_flag_host, sizeof(int)));
  }
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
  float* bufs[3];
  for (auto& b : bufs) b = pl.alloc((size_t)B * max_t * 4);
  float* hbuf = pl.alloc((size_t)B * max_t * 4);   // conv1 output of a ResnetBlock
  float* abuf = pl.alloc((size_t)B * max_t * 4);   // GroupNorm + SiLU output where a conv has no fused prologue
  double2* part = (double2*)pl.alloc((size_t)B * max_chunks * G * sizeof(double2));
  double2* emit_parts[2];  // producer-emitted statistics alternate between two buffers (x's and y's)
  for (auto& e : emit_parts) e = (double2*)pl.alloc((size_t)B * max_chunks * G * sizeof(double2));
  float* gsc = pl.alloc((size_t)B * max_c * 4);
  float* gsh = pl.alloc((size_t)B * max_c * 4);
  // attention scratch: qkv rows, O rows, and the scores of `sb` images at a time (bounded score scratch)
  const int hw0 = H * W, Ca = attn.C;
  const size_t kScoreBudget = (size_t)256 << 20;
  const int sb = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, kScoreBudget / ((size_t)hw0 * hw0 * 4)));
  float* qkv = pl.alloc((size_t)B * hw0 * 3 * Ca * 4);
  float* Ob = pl.alloc((size_t)B * hw0 * Ca * 4);
  float* Sb = pl.alloc((size_t)sb * hw0 * hw0 * 4);

  Plan* P_ = &pl;
  VaeDecoder* self = this;
  auto add = [&](std::string label, double flops, double bytes, std::function<int(hipStream_t)> fn) {
    pl.add(std::move(label), flops, bytes, std::move(fn));
  };
  auto conv_cost = [](const ConvArgs& c, double& fl, double& by) {
    const double M = (double)c.B * c.Hout * c.Wout;
    fl = 2.0 * M * c.Cout * c.K;
    by = 4.0 * ((double)c.B * c.Hin * c.Win * c.Cin1 + M * c.Cin2 + (double)c.Cout * c.K + M * c.Cout +
                (c.res ? M * c.Cout : 0.0));
  };
  auto gemm_cost = [](const GemmArgs& g, double& fl, double& by) {
    const double Z = (double)g.Z1 * g.Z2;
    fl = 2.0 * Z * g.M * g.N * g.K;
    by = 4.0 * Z * ((double)g.M * g.K + (double)g.N * g.K + (double)g.M * g.N) + (g.res ? 4.0 * g.M * g.N : 0.0);
  };
  auto add_conv = [&](ConvArgs c) {
    split_for(c);
    c.k32_resolved = 1 + conv_k32_pick(c);
    double fl, by;
    conv_cost(c, fl, by);
    add(conv_label(c), fl, by, [=](hipStream_t st) { return conv2d_igemm(c, st); });
  };
  auto add_gemm = [&](const GemmArgs& g) {
    double fl, by;
    gemm_cost(g, fl, by);
    add(gemm_label(g), fl, by, [=](hipStream_t st) { return gemm_batched(g, st); });
  };

  // GroupNorm statistics a producer's epilogue emitted for a view (pointer -> partials)
  struct Ready { const double2* p; int C; };
  std::map<const float*, Ready> gn_ready;
  int emit_next = 0;
  auto emit_conv = [&](ConvArgs& c, const View& v) {
    gn_ready.erase(v.p);
    c.gn_part = nullptr;
    c.gn_G = 0;
    if (!toggles().gn_fusion) return;
    ConvArgs sk = c;
    sk.gn_part = reinterpret_cast<double2*>(16);  // placeholder: the shape check only
    sk.gn_G = G;
    split_for(sk);
    if (!conv_can_emit_gn(sk)) return;
    c.gn_part = emit_parts[emit_next];
    emit_next ^= 1;
    c.gn_G = G;
    // the buffer's previous owner (two producers ago) has been consumed; drop a stale entry that points at it
    for (auto it = gn_ready.begin(); it != gn_ready.end();)
      it = it->second.p == c.gn_part ? gn_ready.erase(it) : std::next(it);
    gn_ready[v.p] = {c.gn_part, v.C};
  };
  auto gn_stats = [&](const View& v) -> const double2* {
    auto it = gn_ready.find(v.p);
    if (it != gn_ready.end() && it->second.C == v.C) return it->second.p;
    add("gn_partial", 0, 4.0 * v.B * v.H * v.W * v.C, [=](hipStream_t st) { return gn_partial(v, G, part, st); });
    return part;
  };
  // GroupNorm(G) + SiLU of v as conv c's prologue: in-kernel finalize where the conv keeps its tables in LDS and the
  // map is small, else a gn_finalize launch (as the UNet plan's gn_prologue, at this network's eps)
  auto gn_prologue = [&](ConvArgs& c, const View& v, const double2* stp, const GnW& gw) {
    c.pro_scale = gsc;
    c.pro_shift = gsh;
    split_for(c);
    const long imgs = c.taps == 1 ? 127 / ((long)c.Hout * c.Wout) + 2 : [&] {
      PatchGeom gg{};
      conv_patch_pick(c, gg);
      return (long)gg.TB;
    }();
    const float* gamma = P(gw.g);
    const float* beta = P(gw.b);
    if (conv_lds_tables(c) && imgs * G <= 512 && v.C == c.Cin1 && gn_num_chunks(v.H * v.W) <= 64) {
      c.gin_part = stp; c.gin_G = G; c.gin_nchunk = gn_num_chunks(v.H * v.W);
      c.gin_n = (double)v.H * v.W * (v.C / G); c.gin_eps = eps;
      c.gin_gamma = gamma; c.gin_beta = beta; c.gin_ms = nullptr; c.gin_mb = nullptr; c.gin_mp = 0;
      return;
    }
    add("gn_finalize", 0, 8.0 * B * v.C,
        [=](hipStream_t st) { return gn_finalize(v, G, stp, eps, gamma, beta, gsc, gsh, st); });
  };

  int cur_buf = 0;
  auto next_buf = [&]() {
    cur_buf = (cur_buf + 1) % 3;
    return bufs[cur_buf];
  };

  // --- latent entry: scale, post_quant_conv
  {
    const float* w = arch.post_quant ? P(pq_w) : nullptr;
    const float* bb = arch.post_quant ? P(pq_b) : nullptr;
    const long hw = (long)H * W, n = (long)B * hw;
    add("vae_latent_in_kernel", 2.0 * n * zc * zc, 8.0 * n * zc, [=](hipStream_t st) {
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
    add("conv3x3_small_in", 2.0 * B * H * W * cn * 9 * zc, 4.0 * B * H * W * (zc + cn),
        [=](hipStream_t st) { return conv3x3_small_in(zq, B, zc, H, W, w, bb, cn, ys, st); });
  }

  auto resblock = [&](const ResW& r, const View& xin) -> View {
    const int Ho = xin.H, Wo = xin.W;
    View y{next_buf(), B, Ho, Wo, r.cout, r.cout};
    View va{abuf, B, Ho, Wo, r.cin, r.cin};
    View vh{hbuf, B, Ho, Wo, r.cout, r.cout};
    View va2{abuf, B, Ho, Wo, r.cout, r.cout};
    const int nchunk = gn_num_chunks(Ho * Wo);
    ConvArgs c1{};
    c1.x1 = xin.p; c1.x1_pitch = xin.pitch; c1.Cin1 = r.cin; c1.Hin = Ho; c1.Win = Wo;
    c1.taps = 9; c1.stride = 1;
    c1.w = P(r.conv1.w); c1.K = r.conv1.K;
    c1.y = hbuf; c1.y_pitch = r.cout; c1.Cout = r.cout; c1.B = B; c1.pick_B = kPickBatch; c1.Hout = Ho; c1.Wout = Wo;
    c1.bias = P(r.conv1.bias);
    ConvArgs c2{};
    c2.x1 = hbuf; c2.x1_pitch = r.cout; c2.Cin1 = r.cout; c2.Hin = Ho; c2.Win = Wo;
    c2.taps = 9; c2.stride = 1;
    c2.w = P(r.conv2.w); c2.K = r.conv2.K;
    c2.y = y.p; c2.y_pitch = y.pitch; c2.Cout = r.cout; c2.B = B; c2.pick_B = kPickBatch; c2.Hout = Ho; c2.Wout = Wo;
    c2.bias = P(r.conv2.bias);
    if (r.cin != r.cout) {
      c2.x2 = xin.p; c2.x2_pitch = xin.pitch; c2.Cin2 = r.cin;
    } else {
      c2.res = xin.p; c2.res_pitch = xin.pitch;
    }
    split_for(c1);
    split_for(c2);
    const bool fuse1 = conv_pick(c1) >= 3, fuse2 = conv_pick(c2) >= 3;
    const double2* st1 = gn_stats(xin);
    const GnW g1 = r.gn1, g2 = r.gn2;
    if (fuse1) {
      gn_prologue(c1, xin, st1, g1);
    } else {
      add("gn_apply", 0, 8.0 * B * Ho * Wo * r.cin, [=](hipStream_t st) {
        return gn_apply(xin, G, st1, nchunk, eps, self->P(g1.g), self->P(g1.b), nullptr, nullptr, 0, 1, va, st);
      });
      c1.x1 = abuf; c1.x1_pitch = r.cin;
    }
    emit_conv(c1, vh);
    add_conv(c1);
    const double2* st2 = gn_stats(vh);
    if (fuse2) {
      gn_prologue(c2, vh, st2, g2);
    } else {
      add("gn_apply", 0, 8.0 * B * Ho * Wo * r.cout, [=](hipStream_t st) {
        return gn_apply(vh, G, st2, nchunk, eps, self->P(g2.g), self->P(g2.b), nullptr, nullptr, 0, 1, va2, st);
      });
      c2.x1 = abuf;
    }
    emit_conv(c2, y);
    add_conv(c2);
    return y;
  };

  // --- middle
  x = resblock(mid1, x);
  {
    // mid.attn_1 (autoencoder.py:158-182): one head of C channels over L = H W tokens, scores scaled by C^-1/2.
    // Unfused: qkv (GroupNorm folded into its A load), per image S = (s q) k^T, softmax rows, O = P v, then proj_out
    // + residual. attn_flash / attn_fused stop at head dims 80 / L = 256 and do not take this shape.
    const AttnW p = attn;
    const int C = p.C, hw = hw0;
    const View xin = x;
    View y{next_buf(), B, H, W, C, C};
    const double2* sta = gn_stats(xin);
    const float sa = (float)std::pow((double)C, -0.5);
    ConvArgs cq{};
    cq.x1 = xin.p; cq.x1_pitch = xin.pitch; cq.Cin1 = C; cq.Hin = H; cq.Win = W; cq.taps = 1; cq.stride = 1;
    cq.w = P(p.wqkv); cq.K = C; cq.y = qkv; cq.y_pitch = 3 * C; cq.Cout = 3 * C; cq.B = B; cq.pick_B = kPickBatch;
    cq.Hout = H; cq.Wout = W; cq.bias = P(p.bqkv); cq.pro_scale = gsc; cq.pro_shift = gsh; cq.pro_nosilu = 1;
    split_for(cq);
    if (conv_pw_ok(cq)) {
      gn_prologue(cq, xin, sta, p.gn);
      add_conv(cq);
    } else {
      const GnW gw = p.gn;
      add("gn_finalize", 0, 8.0 * B * C,
          [=](hipStream_t st) { return gn_finalize(xin, G, sta, eps, self->P(gw.g), self->P(gw.b), gsc, gsh, st); });
      GemmArgs gq{};
      gq.M = B * hw; gq.N = 3 * C; gq.K = C; gq.Z1 = 1; gq.Z2 = 1; gq.pick_M = (long)kPickBatch * hw;
      gq.A = xin.p; gq.lda = xin.pitch; gq.Bm = P(p.wqkv); gq.ldb = C; gq.C = qkv; gq.ldc = 3 * C;
      gq.alpha = 1.f; gq.bias = P(p.bqkv);
      gq.pro_scale = gsc; gq.pro_shift = gsh; gq.pro_rows = hw;
      split_gemm(gq, 6, gq.Bm, (size_t)3 * C * C, 0);
      add_gemm(gq);
    }
    for (int b0 = 0; b0 < B; b0 += sb) {
      const int nb = std::min(sb, B - b0);
      const float* q0 = qkv + (size_t)b0 * hw * 3 * C;
      GemmArgs gs{};
      gs.M = hw; gs.N = hw; gs.K = C; gs.Z1 = nb; gs.Z2 = 1; gs.pick_Z = kPickBatch;
      gs.A = q0; gs.a_s1 = (long)hw * 3 * C; gs.lda = 3 * C;
      gs.Bm = q0 + C; gs.b_s1 = (long)hw * 3 * C; gs.ldb = 3 * C;
      gs.C = Sb; gs.c_s1 = (long)hw * hw; gs.ldc = hw;
      gs.alpha = sa;
      split_gemm(gs, 6, nullptr, 0, 6);
      add_gemm(gs);
      const long rows = (long)nb * hw;
      add("softmax_rows", 0, 8.0 * rows * hw, [=](hipStream_t st) { return softmax_rows(Sb, rows, hw, hw, st); });
      GemmArgs go{};
      go.M = hw; go.N = C; go.K = hw; go.Z1 = nb; go.Z2 = 1; go.pick_Z = kPickBatch;
      go.A = Sb; go.a_s1 = (long)hw * hw; go.lda = hw;
      go.Bm = q0 + 2 * C; go.b_s1 = (long)hw * 3 * C; go.ldb = 3 * C; go.b_kn = 1;
      go.C = Ob + (size_t)b0 * hw * C; go.c_s1 = (long)hw * C; go.ldc = C;
      go.alpha = 1.f;
      split_gemm(go, 14, nullptr, 0, 6);
      add_gemm(go);
    }
    ConvArgs cp{};
    cp.x1 = Ob; cp.x1_pitch = C; cp.Cin1 = C; cp.Hin = H; cp.Win = W; cp.taps = 1; cp.stride = 1;
    cp.w = P(p.wproj); cp.K = C; cp.y = y.p; cp.y_pitch = y.pitch; cp.Cout = C; cp.B = B; cp.pick_B = kPickBatch;
    cp.Hout = H; cp.Wout = W; cp.bias = P(p.bproj); cp.res = xin.p; cp.res_pitch = xin.pitch;
    split_for(cp);
    if (conv_pw_ok(cp)) {
      emit_conv(cp, y);
      add_conv(cp);
    } else {
      GemmArgs gp{};
      gp.M = B * hw; gp.N = C; gp.K = C; gp.Z1 = 1; gp.Z2 = 1; gp.pick_M = (long)kPickBatch * hw;
      gp.A = Ob; gp.lda = C; gp.Bm = P(p.wproj); gp.ldb = C; gp.C = y.p; gp.ldc = y.pitch;
      gp.alpha = 1.f; gp.bias = P(p.bproj); gp.res = xin.p; gp.ld_res = xin.pitch;
      split_gemm(gp, 6, gp.Bm, (size_t)C * C, 0);
      gn_ready.erase(y.p);
      add_gemm(gp);
    }
    x = y;
  }
  x = resblock(mid2, x);

  // --- levels, from the lowest resolution upward
  for (int i = L - 1; i >= 0; --i) {
    for (const ResW& r : levels[i].blocks) x = resblock(r, x);
    if (!levels[i].has_up) continue;
    const ConvW cv = levels[i].up;
    View y{next_buf(), B, 2 * x.H, 2 * x.W, cv.Cout, cv.Cout};
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
      if (conv_pick(s) >= 3) c = s;
    }
    if (c.upsample == 2)
      emit_conv(c, y);
    else
      gn_ready.erase(y.p);
    add_conv(c);
    x = y;
  }

  // --- image exit: norm_out -> SiLU -> conv_out, NCHW store
  {
    const View xin = x;
    const int C = xin.C;
    DM_REQUIRE(xin.H == Hout && xin.W == Wout && C == c_out, "decoder plan: output shape");
    const int nchunk = gn_num_chunks(Hout * Wout);
    const GnW lg = out_gn;
    const double2* stl = gn_stats(xin);
    GnFin fin;
    if (toggles().gn_fusion && C <= 512 && C % G == 0 && nchunk <= 64) {
      fin.part = stl; fin.G = G; fin.nchunk = nchunk; fin.n = (double)Hout * Wout * (C / G); fin.eps = eps;
      fin.gamma = P(lg.g); fin.beta = P(lg.b);
    } else {
      add("gn_finalize", 0, 8.0 * B * C,
          [=](hipStream_t st) { return gn_finalize(xin, G, stl, eps, self->P(lg.g), self->P(lg.b), gsc, gsh, st); });
    }
    if (!out_packed) {
      DM_CHECK_HIP(hipMalloc(&out_packed, (size_t)9 * C * 8 * sizeof(float)));
      DM_REQUIRE(small_out_pack(P(out_w), oc, C, out_packed, nullptr) == DM_OK, "conv_out: weight packing failed");
      DM_CHECK_HIP(hipDeviceSynchronize());
    }
    const float* lw = out_packed;
    const float* lb = P(out_b);
    add("conv3x3_small_out", 2.0 * B * Hout * Wout * oc * 9 * C, 4.0 * B * Hout * Wout * (C + oc),
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

#define DM_VAE_MODEL(h)                           \
  if (!(h) || !(h)->m) {                          \
    dm::set_error("null decoder");                \
    return DM_ERR_STATE;                          \
  }

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
  DM_VAE_MODEL(h);
  if (!z || !out) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  if (B <= 0 || H <= 0 || W <= 0) { dm::set_error("empty batch or latent"); return DM_ERR_ARG; }
  if (static_cast<const void*>(out) == static_cast<const void*>(z)) {
    dm::set_error("out must not alias z");
    return DM_ERR_ARG;
  }
  dm::VaeDecoder* m = h->m;
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
  if (const int rco = m->plans.pool->order(st)) return rco;
  const int rc_body = [&]() -> int {
    // at most two passes: the caller's arithmetic, then (fp16x2 met an activation beyond the fp16 range) bf16x3
    for (int math = m->base_math;;) {
      dm::VaeDecoder::Plan* plp = nullptr;
      const int rc0 = m->get_plan(B, H, W, math, &plp);
      if (rc0) return rc0;
      auto& pl = *plp;
      if (pl.scale != scale) {  // the latent-entry launch reads the scale at capture time
        pl.scale = scale;
        pl.invalidate_graph();
      }
      DM_CHECK_HIP(hipMemcpyAsync(pl.z, z, nz * sizeof(float), hipMemcpyDeviceToDevice, st));
      const int rc = pl.run(st);
      if (rc) return rc;
      DM_CHECK_HIP(hipMemcpyAsync(out, pl.out, no * sizeof(float), hipMemcpyDeviceToDevice, st));
      if (math != 2 || !m->range_check) break;
      DM_CHECK_HIP(hipMemcpyAsync(m->range_flag_host, m->range_flag, sizeof(int), hipMemcpyDeviceToHost, st));
      DM_CHECK_HIP(hipStreamSynchronize(st));
      if (!*m->range_flag_host) break;
      DM_CHECK_HIP(hipMemsetAsync(m->range_flag, 0, sizeof(int), st));
      m->range_fallbacks++;
      math = 3;
    }
    return DM_OK;
  }();
  const int rc_mark = m->plans.pool->mark(st);
  return rc_body ? rc_body : rc_mark;
}

extern "C" int dm_vae_decoder_range_stats(const dm_vae_decoder* h, int64_t* fallbacks, int* active) {
  DM_VAE_MODEL(h);
  if (fallbacks) *fallbacks = h->m->range_fallbacks;
  if (active) *active = h->m->base_math;
  return DM_OK;
}

extern "C" int dm_vae_decoder_memory(const dm_vae_decoder* h, int64_t* weight_bytes, int64_t* workspace_bytes) {
  DM_VAE_MODEL(h);
  if (weight_bytes) *weight_bytes = (int64_t)(h->m->arena_floats * sizeof(float) + h->m->split_bytes);
  if (workspace_bytes) *workspace_bytes = (int64_t)h->m->plans.pool->bytes();
  return DM_OK;
}

extern "C" int dm_vae_decoder_plan_stats(const dm_vae_decoder* h, int64_t* builds, int* cached) {
  DM_VAE_MODEL(h);
  if (builds) *builds = h->m->plans.builds;
  if (cached) *cached = (int)h->m->plans.plans.size();
  return DM_OK;
}

extern "C" int dm_vae_decoder_set_math(dm_vae_decoder* h, int kind) {
  DM_VAE_MODEL(h);
  if (kind != 0 && kind != DM_SPLIT_BF16X3 && kind != DM_SPLIT_FP16X2) {
    dm::set_error("decoder math must be 0 (fp32), DM_SPLIT_BF16X3 or DM_SPLIT_FP16X2");
    return DM_ERR_ARG;
  }
  if (kind != h->m->base_math) {
    h->m->base_math = kind;
    h->m->plans.clear();
  }
  return DM_OK;
}

extern "C" int dm_vae_decoder_get_math(const dm_vae_decoder* h, int* kind) {
  DM_VAE_MODEL(h);
  if (!kind) { dm::set_error("kind is null"); return DM_ERR_ARG; }
  *kind = h->m->base_math;
  return DM_OK;
}

extern "C" int dm_vae_decoder_profile(dm_vae_decoder* h, int enable) {
  DM_VAE_MODEL(h);
  if (!h->m->plans.current()) { dm::set_error("no plan yet: run dm_vae_decoder_forward once first"); return DM_ERR_STATE; }
  h->m->plans.current()->profile_enable(enable);
  return DM_OK;
}

extern "C" int dm_vae_decoder_profile_count(dm_vae_decoder* h, int* n_ops) {
  DM_VAE_MODEL(h);
  if (!h->m->plans.current() || !n_ops) { dm::set_error("no plan"); return DM_ERR_STATE; }
  *n_ops = (int)h->m->plans.current()->ops.size();
  return DM_OK;
}

extern "C" int dm_vae_decoder_profile_get(dm_vae_decoder* h, int i, char* label, int label_len, double* flops,
                                          double* bytes, double* ms_total, int64_t* launches) {
  DM_VAE_MODEL(h);
  if (!h->m->plans.current()) { dm::set_error("no plan"); return DM_ERR_STATE; }
  return h->m->plans.current()->profile_get(i, label, label_len, flops, bytes, ms_total, launches);
}

extern "C" void dm_vae_decoder_destroy(dm_vae_decoder* h) {
  if (!h) return;
  (void)hipDeviceSynchronize();
  delete h->m;
  delete h;
}
