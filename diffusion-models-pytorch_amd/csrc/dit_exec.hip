// Native executor for the DiT denoiser (models/dit/model.py:145-252).
//
// Build time (dm_dit_create): the state_dict tensors are consumed in
// registration order and copied into one library-owned arena; the adaLN
// modulation Linear of every block and of the final layer are stacked into ONE
// [depth * 6D + 2D][D] matrix, so all modulation vectors of a forward come from
// a single GEMM over SiLU(t_emb + y_emb).
//
// Forward: tokens stay resident as one [B * T][D] fp32 matrix x, updated in
// place by the gated-residual epilogues. Per block (dit/model.py:118-122):
//   row_stats(x) -> QKV GEMM with the LayerNorm + modulate prologue
//   -> S = (q * d^-1/2) k^T -> softmax -> O = P v -> proj GEMM, x += gate_msa * (.)
//   row_stats(x) -> fc1 GEMM (LN + modulate prologue, GELU-tanh epilogue)
//   -> fc2 GEMM, x += gate_mlp * (.)
// so norm1/norm2/modulate/gate never materialise. All GEMMs are the fp32 MFMA
// kernel of gemm.hip.
//
// MDTv2 (models/mdt/model.py:246-501, inference) is the same model object and the same per-block emission
// (build_plan's emit_block) with three additions: a learned relative-position bias inside every attention (the
// flash kernel's BW > 0 form, or softmax_rows_bias), skip_linear(cat[x, skip]) in front of the en_outblocks and
// de_blocks (emit_skip: one K = 2 D GEMM behind linear_presplit_cat), and the topology en_inblocks ->
// en_outblocks (skips popped last in, first out) -> + decoder_pos_embed -> de_blocks (skip = the embedded input).
#include <cmath>
#include <memory>
#include <vector>

#include <map>
#include "dm_common.h"
#include "dm_kernels.h"
#include "plan.h"
#include "exec_core.h"

namespace dm {

namespace {

struct BlockP {
  size_t qkv_w, qkv_b, proj_w, proj_b, fc1_w, fc1_b, fc2_w, fc2_b;
  // MDT (models/mdt/model.py:187-220): the block's relative-position bias table, transposed to [heads][bias_hs]
  // ((2W - 1)^2 entries used), once x log2(e) for the flash kernel and once in natural units for softmax_rows_bias;
  // skip_linear [D][2D] + bias where the block has one
  size_t bias_l2 = (size_t)-1, bias_nat = (size_t)-1, bias_raw = (size_t)-1;
  size_t skip_w = (size_t)-1, skip_b = (size_t)-1;
};

constexpr size_t kNone = (size_t)-1;

int dit_count(const dm_dit_arch& a) { return 8 + 10 * a.depth + 4; }
int mdt_half_depth(const dm_mdt_arch& a) { return (a.depth - a.decode_layer) / 2; }
// 10 leading tensors, 11 per block (2 * half_depth + decode_layer + the side block), skip_linear.{weight,bias} in
// the en_outblocks and de_blocks, 4 of the final layer
int mdt_count(const dm_mdt_arch& a) {
  const int hd = mdt_half_depth(a);
  return 10 + 11 * (2 * hd + a.decode_layer + 1) + 2 * (hd + a.decode_layer) + 4;
}
dm_dit_arch mdt_base(const dm_mdt_arch& a) {
  dm_dit_arch d{};
  d.input_size = a.input_size; d.patch_size = a.patch_size; d.in_channels = a.in_channels;
  d.hidden_size = a.hidden_size; d.depth = a.depth; d.num_heads = a.num_heads; d.mlp_hidden = a.mlp_hidden;
  d.num_classes = a.num_classes; d.null_class = a.null_class; d.learn_sigma = a.learn_sigma;
  return d;
}

int dit_validate(const dm_dit_arch* a) {
  DM_REQUIRE(a != nullptr, "arch is null");
  DM_REQUIRE(a->patch_size >= 1 && a->input_size % a->patch_size == 0, "input_size must be divisible by patch_size");
  DM_REQUIRE(a->in_channels >= 1 && (a->in_channels * a->patch_size * a->patch_size) % 4 == 0,
             "in_channels * patch_size^2 must be a multiple of 4");
  DM_REQUIRE(a->hidden_size >= 32 && a->hidden_size % 4 == 0, "hidden_size must be a multiple of 4");
  DM_REQUIRE(a->depth >= 1, "depth must be >= 1");
  DM_REQUIRE(a->num_heads >= 1 && a->hidden_size % a->num_heads == 0 && (a->hidden_size / a->num_heads) % 4 == 0,
             "hidden_size / num_heads must be a multiple of 4");
  DM_REQUIRE(a->mlp_hidden >= 4 && a->mlp_hidden % 4 == 0, "mlp hidden size must be a multiple of 4");
  DM_REQUIRE(a->num_classes >= 1, "num_classes must be >= 1");
  return DM_OK;
}

int mdt_validate(const dm_mdt_arch* a) {
  DM_REQUIRE(a != nullptr, "arch is null");
  const dm_dit_arch d = mdt_base(*a);
  const int rc = dit_validate(&d);
  if (rc) return rc;
  DM_REQUIRE(a->decode_layer >= 0 && a->depth - a->decode_layer >= 2,
             "decode_layer must leave at least one en_inblock / en_outblock pair");
  return DM_OK;
}

}  // namespace

// DiT and MDTv2 share this model: MDT (mdt true) adds the per-block bias tables, the skip_linear weights, the
// decoder position table and the en_in / en_out / de topology of build_plan.
struct DiTModel : ExecNet {
  dm_dit_arch arch;
  bool mdt = false;
  int half_depth = 0, decode_layer = 0;   // MDT: blocks = en_inblocks, en_outblocks, de_blocks (the executed ones)
  int W = 0, bias_hs = 0;                 // MDT: token grid width, floats per head of a transposed bias table
  size_t dpos = 0;                        // MDT: decoder_pos_embed
  int D = 0, T = 0, OC = 0, PP = 0, ada_total = 0;
  size_t pos, xw, xb, tw1, tb1, tw2, tb2, ytab, freqs, ada_w, ada_b, fin_w, fin_b;
  int n_freqs = 128;
  bool freqs_set = false;
  std::vector<BlockP> blocks;
  // Arithmetic of the token GEMMs (qkv, attention, proj, fc1, fc2, final), ExecNet's: 2 = fp16x2 split (gemm.hip
  // SPLIT; default unless DM_CONV_MATH=fp32|bf16x3), 0 = fp32 MFMA, which is also the range fallback. split_w holds
  // the fp16x2 fragment images of the token-GEMM weights (split_conv_weights, taps 1), built once: those GEMMs run
  // linear_k32 (K = 32 MFMA steps, no per-load split of the weights)
  DiTModel() {
    base_math = conv_math = conv_math_from_env() == 2 ? 2 : 0;
    fallback_math = 0;
  }
  bool linear_k32_on = true;
  // linear_k32's split-K tail (GemmArgs::sk_*): one 64-KB slab per resident block and one arrival counter per
  // tile, zeroed once (each tile's reducing block resets its counter); forwards of this model's plans are
  // stream-ordered (ScratchPool::order), so one set serves them all
  float* sk_ws = nullptr;
  unsigned* sk_cnt = nullptr;
  int sk_cap = 0;

  struct Plan : PlanBase {
    int B = 0;
    int math = 0;   // the arithmetic the plan was built with
    // plan-owned staging of the caller's tensors (graph replay reads fixed pointers)
    float* x = nullptr;
    int64_t* t = nullptr;
    int64_t* y = nullptr;  // -1 rows select the null class
    float* out = nullptr;
  };
  PlanCache<Plan> plans;  // LRU over B, scratch from one pool

  ~DiTModel() {
    if (sk_ws) (void)hipFree(sk_ws);
    if (sk_cnt) (void)hipFree(sk_cnt);
  }
  int build_plan(Plan& pl, int B);
  // DM_MATH_FP16 (m == 1): a plan of the fp16x2 arithmetic (conv_math 2: the attention products, the adaLN GEMM and
  // whatever linear_h16_ok refuses are built exactly as in that mode) whose covered static-weight token GEMMs run
  // linear_h16.hip on piece 0 of the same fragment images -- no second weight copy
  bool h16_plan = false;
  int get_plan(int B, int m, Plan** out) {
    h16_plan = m == DM_MATH_FP16;
    conv_math = h16_plan ? 2 : m;
    return plans.get([&](const Plan& p) { return p.B == B && p.math == m; }, [&](Plan& p) { return build_plan(p, B); },
                     out);
  }
};

// march null: DiT; else MDTv2 (arch = mdt_base(*march))
static int dit_create(const dm_dit_arch* arch, const dm_mdt_arch* march, const float* const* params,
                      const int64_t* numels, int n_params, hipStream_t st, DiTModel** out) {
  int rc = march ? mdt_validate(march) : dit_validate(arch);
  if (rc) return rc;
  const dm_dit_arch a = *arch;
  const bool mdt = march != nullptr;
  const int want = mdt ? mdt_count(*march) : dit_count(a);
  DM_REQUIRE(n_params == want, "expected " + std::to_string(want) + " parameter tensors, got " +
                                   std::to_string(n_params));
  refresh_toggles();  // the model's arithmetic and range check (member initialisers) from this snapshot
  auto m = std::make_unique<DiTModel>();
  m->arch = a;
  const int D = a.hidden_size, p = a.patch_size, C = a.in_channels, Hm = a.mlp_hidden;
  const int S = a.input_size / p;
  m->D = D;
  m->T = S * S;
  m->OC = a.learn_sigma ? 2 * C : C;
  m->PP = p * p;
  m->mdt = mdt;
  if (mdt) {
    m->half_depth = mdt_half_depth(*march);
    m->decode_layer = march->decode_layer;
    m->W = S;
    m->bias_hs = ((2 * S - 1) * (2 * S - 1) + 63) / 64 * 64;
  }
  const int n_exec = mdt ? 2 * m->half_depth + m->decode_layer : a.depth;   // executed blocks
  m->ada_total = n_exec * 6 * D + 2 * D;
  const int n_cls = a.num_classes + (a.null_class ? 1 : 0);

  // arena layout: everything 64-float aligned
  size_t size = 0;
  auto reserve = [&](int64_t n) { size_t off = size; size += ((size_t)n + 63) / 64 * 64; return off; };
  struct Copy { size_t dst; int idx; int64_t n; };
  std::vector<Copy> copies;
  int idx = 0;
  std::string err;
  auto take = [&](int64_t n, const char* what) {
    if (idx < n_params && numels[idx] != n && err.empty())
      err = "parameter " + std::to_string(idx) + " (" + what + "): expected " + std::to_string(n) + " elements, got " +
            std::to_string(numels[idx]);
    const size_t off = reserve(n);
    copies.push_back({off, idx++, n});
    return off;
  };
  auto take_at = [&](int64_t n, size_t dst, const char* what) {
    if (idx < n_params && numels[idx] != n && err.empty())
      err = "parameter " + std::to_string(idx) + " (" + what + "): expected " + std::to_string(n) + " elements, got " +
            std::to_string(numels[idx]);
    copies.push_back({dst, idx++, n});
  };

  m->pos = take((int64_t)m->T * D, "pos_embed");
  if (mdt) {
    m->dpos = take((int64_t)m->T * D, "decoder_pos_embed");
    take(D, "mask_token");   // training only
  }
  m->xw = take((int64_t)D * C * p * p, "x_embedder.proj.weight");
  m->xb = take(D, "x_embedder.proj.bias");
  m->tw1 = take((int64_t)D * 256, "t_embedder.mlp.0.weight");
  m->tb1 = take(D, "t_embedder.mlp.0.bias");
  m->tw2 = take((int64_t)D * D, "t_embedder.mlp.2.weight");
  m->tb2 = take(D, "t_embedder.mlp.2.bias");
  m->ytab = take((int64_t)n_cls * D, "y_embedder.embedding_table.weight");
  m->freqs = reserve(128);
  m->ada_w = reserve((int64_t)m->ada_total * D);
  m->ada_b = reserve(m->ada_total);
  const int n_rel = (2 * S - 1) * (2 * S - 1) + 3;   // BEiT table rows (the last 3, the cls entries, never indexed)
  for (int b = 0; b < (mdt ? n_exec + 1 : a.depth); ++b) {
    BlockP bp;
    bp.qkv_w = take((int64_t)3 * D * D, "attn.qkv.weight");
    bp.qkv_b = take(3 * D, "attn.qkv.bias");
    bp.proj_w = take((int64_t)D * D, "attn.proj.weight");
    bp.proj_b = take(D, "attn.proj.bias");
    if (mdt) {
      bp.bias_raw = take((int64_t)n_rel * a.num_heads, "attn.rel_pos_bias.relative_position_bias_table");
      bp.bias_l2 = reserve((int64_t)a.num_heads * m->bias_hs);
      bp.bias_nat = reserve((int64_t)a.num_heads * m->bias_hs);
    }
    bp.fc1_w = take((int64_t)Hm * D, "mlp.fc1.weight");
    bp.fc1_b = take(Hm, "mlp.fc1.bias");
    bp.fc2_w = take((int64_t)D * Hm, "mlp.fc2.weight");
    bp.fc2_b = take(D, "mlp.fc2.bias");
    if (b < n_exec) {
      take_at((int64_t)6 * D * D, m->ada_w + (size_t)b * 6 * D * D, "adaLN_modulation.1.weight");
      take_at(6 * D, m->ada_b + (size_t)b * 6 * D, "adaLN_modulation.1.bias");
    } else {   // MDT's side block: loaded, never executed at inference, its modulation never computed
      take((int64_t)6 * D * D, "sideblocks.adaLN_modulation.1.weight");
      take(6 * D, "sideblocks.adaLN_modulation.1.bias");
    }
    if (mdt && b >= m->half_depth && b < n_exec) {
      bp.skip_w = take((int64_t)D * 2 * D, "skip_linear.weight");
      bp.skip_b = take(D, "skip_linear.bias");
    }
    if (b < n_exec) m->blocks.push_back(bp);
  }
  m->fin_w = take((int64_t)m->PP * m->OC * D, "final_layer.linear.weight");
  m->fin_b = take(m->PP * m->OC, "final_layer.linear.bias");
  take_at((int64_t)2 * D * D, m->ada_w + (size_t)n_exec * 6 * D * D, "final_layer.adaLN_modulation.1.weight");
  take_at(2 * D, m->ada_b + (size_t)n_exec * 6 * D, "final_layer.adaLN_modulation.1.bias");
  if (!err.empty()) {
    set_error(err);
    return DM_ERR_ARG;
  }
  DM_REQUIRE(idx == n_params, "parameter count mismatch after walk");

  m->arena_floats = size;
  DM_CHECK_HIP(hipMalloc(&m->arena, size * sizeof(float)));
  for (auto& c : copies) {
    DM_REQUIRE(params[c.idx] != nullptr, "null parameter pointer");
    DM_CHECK_HIP(hipMemcpyAsync(m->arena + c.dst, params[c.idx], c.n * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  if (mdt) {
    // bias tables [n_rel][heads] -> [heads][bias_hs], x log2(e) in float64 rounded once (flash) and as they are
    DM_CHECK_HIP(hipStreamSynchronize(st));
    const int heads = a.num_heads, used = n_rel - 3, hs = m->bias_hs;
    std::vector<float> raw((size_t)n_rel * heads), tl2((size_t)heads * hs), tnat((size_t)heads * hs);
    for (const BlockP& bp : m->blocks) {
      DM_CHECK_HIP(hipMemcpy(raw.data(), m->P(bp.bias_raw), raw.size() * sizeof(float), hipMemcpyDeviceToHost));
      std::fill(tl2.begin(), tl2.end(), 0.f);
      std::fill(tnat.begin(), tnat.end(), 0.f);
      for (int h = 0; h < heads; ++h)
        for (int i = 0; i < used; ++i) {
          const float v = raw[(size_t)i * heads + h];
          tnat[(size_t)h * hs + i] = v;
          tl2[(size_t)h * hs + i] = (float)((double)v * 1.4426950408889634074);
        }
      DM_CHECK_HIP(hipMemcpy(m->P(bp.bias_l2), tl2.data(), tl2.size() * sizeof(float), hipMemcpyHostToDevice));
      DM_CHECK_HIP(hipMemcpy(m->P(bp.bias_nat), tnat.data(), tnat.size() * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  *out = m.release();
  return DM_OK;
}

int DiTModel::build_plan(Plan& pl, int B) {
  refresh_toggles();
  pl.toggles = toggles();
  ToggleScope scope(pl.toggles);
  pl.graph_enabled = toggles().graph;
  pl.B = B;
  const bool h16 = h16_plan;
  pl.math = h16 ? DM_MATH_FP16 : conv_math;
  const dm_dit_arch& a = arch;
  const int p = a.patch_size, C = a.in_channels, S = a.input_size, Hm = a.mlp_hidden;
  const int heads = a.num_heads, Dh = D / heads;
  const long M = (long)B * T;
  DM_REQUIRE((long)B * heads <= 65535, "batch * heads too large for one attention launch");

  if (const int rcf = ensure_range_flag()) return rcf;
  if (!sk_ws && toggles().lin_sk && linear_k32_slots() > 0) {
    const int slots = linear_k32_slots();
    DM_CHECK_HIP(hipMalloc(&sk_ws, (size_t)slots * 65536));
    DM_CHECK_HIP(hipMalloc(&sk_cnt, (size_t)slots * sizeof(unsigned)));
    DM_CHECK_HIP(hipMemset(sk_cnt, 0, (size_t)slots * sizeof(unsigned)));
    sk_cap = slots;
  }
  const bool sk_on = toggles().lin_sk && sk_ws;
  pl.x = pl.alloc((size_t)B * C * S * S * 4);
  pl.t = (int64_t*)pl.alloc((size_t)B * 8);
  pl.y = (int64_t*)pl.alloc((size_t)B * 8);
  pl.out = pl.alloc((size_t)B * OC * S * S * 4);
  float* e0 = pl.alloc((size_t)B * 256 * 4);
  float* e1 = pl.alloc((size_t)B * D * 4);
  float* temb = pl.alloc((size_t)B * D * 4);
  float* se = pl.alloc((size_t)B * D * 4);
  float* mods = pl.alloc((size_t)B * ada_total * 4);
  float* a0 = pl.alloc((size_t)M * C * p * p * 4);
  float* x = pl.alloc((size_t)M * D * 4);
  // MDT: the en_inblocks' outputs stay live as the en_outblocks' skips and the embedded input as the de_blocks'
  // (xs[0] = x, xs[i + 1] = en_inblock i's output: each block writes a fresh matrix, so no copies), plus one
  // working matrix for everything after them
  std::vector<float*> xs;
  float* xw_ = nullptr;
  if (mdt) {
    xs.push_back(x);
    for (int i = 0; i < half_depth; ++i) xs.push_back(pl.alloc((size_t)M * D * 4));
    xw_ = pl.alloc((size_t)M * D * 4);
  }
  float2* stats = (float2*)pl.alloc((size_t)M * sizeof(float2));
  float* qkv = pl.alloc((size_t)M * 3 * D * 4);
  float* Sb = nullptr;  // score matrix of the unfused attention path (allocated on first use)
  float* Ob = pl.alloc((size_t)M * D * 4);
  float* hb = pl.alloc((size_t)M * Hm * 4);
  float* lin = pl.alloc((size_t)M * PP * OC * 4);
  if (pl.alloc_failed) { set_error("workspace allocation failed"); return DM_ERR_HIP; }

  Plan* P_ = &pl;
  DiTModel* self = this;
  auto add_gemm = [&](const GemmArgs& g) {
    const double Z = (double)g.Z1 * g.Z2;
    const double fl = 2.0 * Z * g.M * g.N * g.K;
    const double by = 4.0 * Z * ((double)g.M * g.K + (double)g.N * g.K + (double)g.M * g.N) +
                      (g.res ? 4.0 * g.M * g.N : 0.0);
    pl.add(gemm_label(g), fl, by, [=](hipStream_t st) { return gemm_batched(g, st); });
  };
  // token GEMMs on linear_k32: LayerNorm-modulate (or nothing) + fp16x2 split of A once per GEMM
  // (linear_presplit_a) instead of once per 128-column tile inside it (27 x for qkv, 36 x for fc1);
  // one buffer shared by all of them (stream-ordered). DM_DIT_PRESPLIT=0: split inside the GEMM.
  const bool presplit_on = toggles().dit_presplit;
  _Float16* as_buf = nullptr;
  size_t as_bytes = 0;
  // LayerNorm statistics for the next GEMM with the LN + modulate prologue: computed by that GEMM's
  // row_stats_split pass (statistics + prologue + split in one read of the tokens) or by row_stats
  bool stats_pending = false;
  const float* stats_src = x;   // the token matrix the pending statistics are of
  const float ln_eps = 1e-6f;
  auto flush_stats = [&]() {
    if (!stats_pending) return;
    stats_pending = false;
    const float* sx = stats_src;
    pl.add("row_stats", 0, 4.0 * M * D, [=](hipStream_t st) { return row_stats(sx, M, D, ln_eps, stats, st); });
  };
  // DM_MATH_FP16: the A image (one fp16 plane) of a covered GEMM, always by its own pass (at every M: the kernel
  // takes A in no other form), LayerNorm statistics from row_stats first; the buffer is the split path's
  auto add_h16_gemm = [&](GemmArgs g) {
    if (g.as) {  // the image came from a producer (fc1's c_split)
      add_gemm(g);
      return;
    }
    const size_t need = (size_t)g.M * g.K * 2;
    if (need > as_bytes) {
      as_buf = reinterpret_cast<_Float16*>(pl.alloc(need));
      as_bytes = need;
    }
    flush_stats();
    _Float16* buf = as_buf;
    pl.add("linear_h16_image", 0, 6.0 * g.M * g.K, [=](hipStream_t st) { return linear_h16_image(g, buf, st); });
    g.as = buf;
    g.pro_scale = g.pro_shift = nullptr;
    g.ln_stats = nullptr;
    add_gemm(g);
  };
  auto add_token_gemm = [&](GemmArgs g) {
    if (g.h16) {
      add_h16_gemm(g);
      return;
    }
    // nominal-batch decision (pick_M = T * kPickBatch): the same kernels at every B, so results are
    // batch-invariant (each image's row block of B * T tokens runs the same code)
    if (g.ws && presplit_on && g.pick_M >= 4096) {
      const size_t need = (size_t)g.M * g.K * 4;
      if (need > as_bytes) {
        as_buf = reinterpret_cast<_Float16*>(pl.alloc(need));
        as_bytes = need;
      }
      GemmArgs g2 = g;
      g2.as = as_buf;
      g2.pro_scale = g2.pro_shift = nullptr;
      g2.ln_stats = nullptr;
      if (as_buf && linear_k32_ok(g2)) {
        _Float16* buf = as_buf;
        if (g.ln_stats && stats_pending && g.A == stats_src && g.lda == D && g.K == D && g.alpha == 1.0f) {
          stats_pending = false;
          float2* sp = stats;
          pl.add("row_stats_split", 0, 8.0 * g.M * g.K, [=](hipStream_t st) {
            return row_stats_split(g.A, g.M, g.K, ln_eps, sp, g.ln_shift, g.ln_scale, g.ln_pitch, g.ln_rows, g.split_ea,
                                   buf, g.range_flag, st);
          });
        } else {
          flush_stats();
          pl.add("linear_presplit_a", 0, 8.0 * g.M * g.K, [=](hipStream_t st) { return linear_presplit_a(g, buf, st); });
        }
        add_gemm(g2);
        return;
      }
    }
    flush_stats();
    add_gemm(g);
  };
  // fp16x2 operand exponents (ExecNet::split_gemm): weights by max |w|, activations fixed (2^6 for
  // LayerNorm-modulated tokens, q, k, v, attention and MLP outputs; 2^14 for softmax rows)
  // cover: a GEMM DM_MATH_FP16 covers (every static-weight token GEMM but the adaLN one)
  auto split = [&](GemmArgs& g, int ea, size_t w, size_t wn, int eb_act, bool cover = true) {
    split_gemm(g, ea, wn ? P(w) : nullptr, wn, eb_act);
    if (conv_math != 2) return;
    // static weight [N][K]: pre-split once for linear_k32 (the gemm.hip path stays the fallback)
    if (wn && linear_k32_on && g.K % 64 == 0 && g.N % 4 == 0) {
      const auto key = std::make_pair((const float*)P(w), 2);
      auto it = split_w.find(key);
      if (it == split_w.end()) {
        void* buf = nullptr;
        const size_t nb = split_conv_weights_bytes(1, g.N, g.K, 2);
        if (hipMalloc(&buf, nb) != hipSuccess) {
          (void)hipGetLastError();
          return;
        }
        if (split_conv_weights(key.first, 1, g.N, g.K, g.K, 1, 2, buf, nullptr) != DM_OK ||
            hipDeviceSynchronize() != hipSuccess) {
          (void)hipFree(buf);
          return;
        }
        it = split_w.emplace(key, buf).first;
        split_bytes += nb;
      }
      g.ws = it->second;
      g.ws_rowscale = split_conv_rowscale(it->second, 1, g.N, g.K);
      if (sk_on) {
        g.sk_ws = sk_ws;
        g.sk_cnt = sk_cnt;
        g.sk_cap = sk_cap;
      }
      if (h16 && cover) {  // the launch form: the image in `as`, the prologue done by the image pass
        GemmArgs ph = g;
        ph.h16 = 1;
        ph.ln_stats = nullptr;
        ph.pro_scale = ph.pro_shift = nullptr;
        ph.as = reinterpret_cast<const _Float16*>(uintptr_t(256));  // only its alignment is checked
        if (linear_h16_ok(ph)) {
          g.h16 = 1;
          g.sk_ws = nullptr;  // (no split-K tail in this arithmetic)
          g.sk_cnt = nullptr;
          return;
        }
      }
      // with the pre-split A image (add_token_gemm) the GEMM takes no prologue: check that form
      GemmArgs probe = g;
      if (presplit_on && g.pick_M >= 4096 && !probe.c_split) {
        probe.ln_stats = nullptr;
        probe.pro_scale = probe.pro_shift = nullptr;
        probe.as = reinterpret_cast<const _Float16*>(uintptr_t(256));  // only its alignment is checked
      }
      if (!linear_k32_ok(probe)) {
        g.ws = nullptr;
        g.ws_rowscale = nullptr;
      }
    }
  };
  auto linear = [&](const float* A, int lda, long rows, size_t w, size_t bias, int N, int K, float* out, int ldc) {
    GemmArgs g{};
    g.M = (int)rows; g.N = N; g.K = K; g.Z1 = 1; g.Z2 = 1; g.pick_M = rows / B * kPickBatch;  // rows = B or B*T
    g.A = A; g.lda = lda; g.Bm = P(w); g.ldb = K; g.C = out; g.ldc = ldc; g.alpha = 1.f;
    g.bias = bias != (size_t)-1 ? P(bias) : nullptr;
    return g;
  };

  // --- conditioning: t_embedder (dit/model.py:40-64), y_embedder, c = t + y, SiLU for every adaLN
  pl.add("timestep_embed", 0, 4.0 * B * 256, [=](hipStream_t st) {
    return timestep_embed(P_->t, B, 256, 1, self->freqs_set ? self->P(self->freqs) : nullptr, e0, st);
  });
  {
    GemmArgs g = linear(e0, 256, B, tw1, tb1, D, 256, e1, D);
    g.act = 1;
    add_gemm(g);
    add_gemm(linear(e1, D, B, tw2, tb2, D, D, temb, D));
  }
  {
    const float* table = P(ytab);
    const int null_row = a.null_class ? a.num_classes : -1;
    pl.add("class_embed_silu", 0, 8.0 * B * D, [=](hipStream_t st) {
      return embed_add_silu(temb, P_->y, table, B, D, se, st, null_row);
    });
  }
  // every block's (and the final layer's) adaLN modulation in one GEMM: [B][depth * 6D + 2D]. A weight stream
  // (902 MB for DiT-XL/2 against 2B = 64 rows): on linear_k32 with the weights pre-split once, one block per
  // 128 columns streaming its K x 128 slice (the fp32 gemm_kernel took 558 us, 1.6 TB/s)
  {
    GemmArgs g = linear(se, D, B, ada_w, ada_b, ada_total, D, mods, ada_total);
    // (DM_MATH_FP16 leaves it on linear_k32: M = B rows against the whole weight stream is bandwidth bound, and a
    // 128-row tile of one product per MAC has nothing to win on B rows)
    split(g, 6, ada_w, (size_t)ada_total * D, 6, false);
    add_gemm(g);
  }

  // --- patch embedding + pos_embed (dit/model.py:244)
  pl.add("patchify", 0, 8.0 * M * C * p * p,
         [=](hipStream_t st) { return patchify(P_->x, B, C, S, S, p, a0, st); });
  {
    GemmArgs g = linear(a0, C * p * p, M, xw, xb, D, C * p * p, x, D);
    g.res = P(pos); g.ld_res = D; g.res_mod = T;
    add_gemm(g);
  }

  auto stats_op = [&](const float* src) { stats_pending = true; stats_src = src; };
  // One transformer block (DiT's and MDT's alike): reads xin, writes x + gate_msa * attn(..) to xmid and
  // xmid + gate_mlp * mlp(..) to xout. DiT runs it in place (xin = xmid = xout = x); MDT's en_inblocks keep xin.
  // bp.bias_l2 set: the attention adds the block's relative-position bias.
  auto emit_block = [&](const BlockP& bp, int b, const float* xin, float* xmid, float* xout) {
    const float* mb = mods + (size_t)b * 6 * D;  // shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
    const bool biased = bp.bias_l2 != kNone;
    // attention branch
    stats_op(xin);
    GemmArgs gq = linear(xin, D, M, bp.qkv_w, bp.qkv_b, 3 * D, D, qkv, 3 * D);
    gq.ln_stats = stats; gq.ln_shift = mb; gq.ln_scale = mb + D; gq.ln_pitch = ada_total; gq.ln_rows = T;
    split(gq, 6, bp.qkv_w, (size_t)3 * D * D, 0);
    // flash attention (attention.hip attn_flash_kernel): the qkv GEMM's epilogue writes q * d^-1/2, k, v as
    // the fp16x2 operand planes (over the qkv buffer: same bytes), S never leaves the CU
    const bool flash = conv_math == 2 && gq.ws && attn_flash_ok(T, Dh) && toggles().attn != kAttnUnfused &&
                       (!biased || attn_flash_bias_ok(T, W));
    _Float16* planes = reinterpret_cast<_Float16*>(qkv);
    const size_t plane_n = (size_t)M * D * 2;   // fp16 elements of one operand's two planes
    if (flash) {
      gq.ap_q = planes; gq.ap_k = planes + plane_n; gq.ap_v = planes + 2 * plane_n;
      gq.ap_L = T; gq.ap_heads = heads; gq.ap_Dh = Dh; gq.ap_legacy = 0;
      gq.ap_alpha = (float)std::pow((double)Dh, -0.5); gq.ap_bscale = 0.f;
      gq.ap_ea = 6; gq.ap_eb = 6; gq.ap_ev = 6;
    }
    add_token_gemm(gq);
    // the proj GEMM, built before the attention op: the flash kernel writes O as the proj's pre-split A image
    // only when this GEMM is the one that will read it (same predicate), else O as fp32 rows
    GemmArgs gpj = linear(Ob, D, M, bp.proj_w, bp.proj_b, D, D, xmid, D);
    gpj.res = xin; gpj.ld_res = D; gpj.gate = mb + 2 * D; gpj.gate_pitch = ada_total; gpj.gate_rows = T;
    split(gpj, 6, bp.proj_w, (size_t)D * D, 0);
    GemmArgs gpj_as = gpj;
    gpj_as.as = reinterpret_cast<const _Float16*>(Ob);
    const bool o_presplit = flash && !gpj.h16 && presplit_on && D % 32 == 0 && gpj.ws && gpj.split_ea == 6 && linear_k32_ok(gpj_as);
    if (flash) {
      AttnArgs at{};
      at.pq = planes; at.pk = planes + plane_n; at.pv = planes + 2 * plane_n;
      at.L = T; at.Dh = Dh; at.heads = heads; at.B = B;
      at.out = Ob; at.ldo = D;
      at.ea = 6; at.eb = 6; at.ep = 14; at.ev = 6;
      at.range_flag = range_flag;
      if (o_presplit) {   // O straight into the proj GEMM's pre-split A image (over Ob)
        at.o_split = reinterpret_cast<_Float16*>(Ob);
        at.o_split_ea = 6;
        at.o_ld = D;
      }
      if (biased) {
        at.bias = P(bp.bias_l2);
        at.bias_W = W;
        at.bias_hs = bias_hs;
      }
      pl.add(std::string(biased ? "attn_flash_bias_kernel<" : "attn_flash_kernel<") + std::to_string(Dh) + ">",
             4.0 * B * heads * (double)T * T * Dh, 4.0 * M * (3.0 * D + D),
             [=](hipStream_t st) { return attn_flash(at, st); });
    } else {
      if (!Sb) Sb = pl.alloc((size_t)B * heads * T * T * 4);
      // timm Attention: qkv.reshape(B, N, 3, heads, d): q / k / v of head h at columns h*d, D + h*d, 2D + h*d
      GemmArgs gs{};
      gs.M = T; gs.N = T; gs.K = Dh; gs.Z1 = B; gs.Z2 = heads; gs.pick_Z = (long)kPickBatch * heads;
      gs.A = qkv; gs.a_s1 = (long)T * 3 * D; gs.a_s2 = Dh; gs.lda = 3 * D;
      gs.Bm = qkv + D; gs.b_s1 = (long)T * 3 * D; gs.b_s2 = Dh; gs.ldb = 3 * D;
      gs.C = Sb; gs.c_s1 = (long)heads * T * T; gs.c_s2 = (long)T * T; gs.ldc = T;
      gs.alpha = (float)std::pow((double)Dh, -0.5);
      split(gs, 6, 0, 0, 6);
      add_gemm(gs);
      const long rows = (long)B * heads * T;
      const int L = T;
      float* Sb_ = Sb;
      if (biased) {
        const float* tab = P(bp.bias_nat);
        const int W_ = W, hs_ = bias_hs;
        pl.add("softmax_rows_bias", 0, 8.0 * rows * L, [=](hipStream_t st) {
          return softmax_rows_bias(Sb_, rows, L, L, tab, W_, hs_, heads, st);
        });
      } else {
        pl.add("softmax_rows", 0, 8.0 * rows * L, [=](hipStream_t st) { return softmax_rows(Sb_, rows, L, L, st); });
      }
      GemmArgs go{};
      go.M = T; go.N = Dh; go.K = T; go.Z1 = B; go.Z2 = heads; go.pick_Z = (long)kPickBatch * heads;
      go.A = Sb; go.a_s1 = (long)heads * T * T; go.a_s2 = (long)T * T; go.lda = T;
      go.Bm = qkv + 2 * D; go.b_s1 = (long)T * 3 * D; go.b_s2 = Dh; go.ldb = 3 * D; go.b_kn = 1;
      go.C = Ob; go.c_s1 = (long)T * D; go.c_s2 = Dh; go.ldc = D;
      go.alpha = 1.f;
      split(go, 14, 0, 0, 6);
      add_gemm(go);
    }
    if (o_presplit)
      add_gemm(gpj_as);   // A = the flash kernel's pre-split O image
    else
      add_token_gemm(gpj);
    // MLP branch
    stats_op(xmid);
    {
      GemmArgs g = linear(xmid, D, M, bp.fc1_w, bp.fc1_b, Hm, D, hb, Hm);
      g.ln_stats = stats; g.ln_shift = mb + 3 * D; g.ln_scale = mb + 4 * D; g.ln_pitch = ada_total; g.ln_rows = T;
      g.act = 2;
      split(g, 6, bp.fc1_w, (size_t)Hm * D, 0);
      GemmArgs g2 = linear(hb, Hm, M, bp.fc2_w, bp.fc2_b, D, Hm, xout, D);
      g2.res = xmid; g2.ld_res = D; g2.gate = mb + 5 * D; g2.gate_pitch = ada_total; g2.gate_rows = T;
      split(g2, 6, bp.fc2_w, (size_t)D * Hm, 0);
      // fc1's epilogue writes GELU(h) as fc2's pre-split A image (over hb: same bytes), no split pass for fc2
      GemmArgs g1s = g, g2s = g2;
      g1s.c_split = reinterpret_cast<_Float16*>(hb);
      g1s.c_split_ea = g2.split_ea;
      g2s.as = reinterpret_cast<const _Float16*>(hb);
      GemmArgs h1 = g1s, h2 = g2s;   // DM_MATH_FP16: the launch forms (fc1's prologue goes to its image pass)
      h1.ln_stats = nullptr;
      h1.as = h2.as;
      if (g.h16 && g2.h16 && linear_h16_ok(h1) && linear_h16_ok(h2)) {
        add_token_gemm(g1s);   // GELU(h) * 2^ea rounded once, as fc2's image (one fp16 plane over hb)
        add_token_gemm(g2s);
      } else if (g.h16 || g2.h16) {
        add_token_gemm(g);
        add_token_gemm(g2);
      } else if (presplit_on && g.ws && g2.ws && linear_k32_ok(g1s) && linear_k32_ok(g2s)) {
        add_token_gemm(g1s);
        add_gemm(g2s);
      } else {
        add_token_gemm(g);
        add_token_gemm(g2);
      }
    }
  };
  // MDT: out = skip_linear(cat[cur, skip]) (mdt/model.py:211-212), no residual; out may be cur. On linear_k32 the A
  // pre-split pass does the concat (linear_presplit_cat) and one K = 2 D GEMM runs against the weight pre-split
  // as [D][2D]; otherwise two chained GEMMs over the weight's column halves, through Ob (free between blocks).
  auto emit_skip = [&](const BlockP& bp, const float* cur, const float* skip, float* out) {
    flush_stats();
    {
      GemmArgs g = linear(cur, 2 * D, M, bp.skip_w, bp.skip_b, D, 2 * D, out, D);
      split(g, 6, bp.skip_w, (size_t)D * 2 * D, 0);
      if (g.h16 && D % 32 == 0) {   // DM_MATH_FP16: the image pass does the concat
        const size_t need = (size_t)M * 2 * D * 2;
        if (need > as_bytes) {
          as_buf = reinterpret_cast<_Float16*>(pl.alloc(need));
          as_bytes = need;
        }
        g.as = as_buf;
        if (as_buf && linear_h16_ok(g)) {
          _Float16* buf = as_buf;
          int* rf = g.range_flag;
          const int D_ = D;
          pl.add("linear_h16_image_cat", 0, 12.0 * M * D, [=](hipStream_t st) {
            return linear_h16_image_cat(cur, skip, M, D_, 6, buf, rf, st);
          });
          add_gemm(g);
          return;
        }
        g.as = nullptr;
      }
      g.h16 = 0;   // (refused: as in fp16x2)
      if (g.ws && presplit_on && g.pick_M >= 4096 && D % 32 == 0) {
        const size_t need = (size_t)M * 2 * D * 4;
        if (need > as_bytes) {
          as_buf = reinterpret_cast<_Float16*>(pl.alloc(need));
          as_bytes = need;
        }
        g.as = as_buf;
        if (as_buf && linear_k32_ok(g)) {
          _Float16* buf = as_buf;
          int* rf = g.range_flag;
          const int D_ = D;
          pl.add("linear_presplit_cat", 0, 16.0 * M * D, [=](hipStream_t st) {
            return linear_presplit_cat(cur, skip, M, D_, 6, buf, rf, st);
          });
          add_gemm(g);
          return;
        }
      }
    }
    auto half = [&](const float* A, size_t woff, bool bias, float* res, float* C) {
      GemmArgs g = linear(A, D, M, bp.skip_w + woff, bias ? bp.skip_b : kNone, D, D, C, D);
      g.ldb = 2 * D;
      g.res = res; g.ld_res = D;
      split_gemm(g, 6, P(bp.skip_w), (size_t)D * 2 * D);  // one exponent for both halves: the whole [D][2D] matrix's
      add_gemm(g);
    };
    half(cur, 0, true, nullptr, Ob);
    half(skip, D, false, Ob, out);
  };
  float* xf = x;   // the final layer's input
  if (!mdt) {
    for (int b = 0; b < a.depth; ++b) emit_block(blocks[b], b, x, x, x);
  } else {
    // mdt/model.py:473-497: en_inblocks (outputs kept as skips), en_outblocks (skips popped last in, first out),
    // + decoder_pos_embed, de_blocks (each with the embedded input as its skip)
    const int hd = half_depth;
    for (int i = 0; i < hd; ++i) emit_block(blocks[i], i, xs[i], xw_, xs[i + 1]);
    const float* cur = xs[hd];
    for (int j = 0; j < hd; ++j) {
      emit_skip(blocks[hd + j], cur, xs[hd - j], xw_);
      emit_block(blocks[hd + j], hd + j, xw_, xw_, xw_);
      cur = xw_;
    }
    {
      const float* tab = P(dpos);
      float* xd = xw_;
      const int D_ = D, T_ = T;
      pl.add("add_rows_mod", 0, 8.0 * M * D, [=](hipStream_t st) { return add_rows_mod(xd, tab, M, D_, T_, st); });
    }
    for (int d = 0; d < decode_layer; ++d) {
      emit_skip(blocks[2 * hd + d], xw_, xs[0], xw_);
      emit_block(blocks[2 * hd + d], 2 * hd + d, xw_, xw_, xw_);
    }
    xf = xw_;
  }
  // --- final layer (dit/model.py:138-142) + unpatchify
  stats_op(xf);
  {
    const float* mf = mods + (size_t)blocks.size() * 6 * D;  // shift, scale
    GemmArgs g = linear(xf, D, M, fin_w, fin_b, PP * OC, D, lin, PP * OC);
    g.ln_stats = stats; g.ln_shift = mf; g.ln_scale = mf + D; g.ln_pitch = ada_total; g.ln_rows = T;
    split(g, 6, fin_w, (size_t)PP * OC * D, 0);
    add_token_gemm(g);
  }
  if (pl.alloc_failed) { set_error("workspace allocation failed"); return DM_ERR_HIP; }
  const int oc = OC;
  pl.add("unpatchify", 0, 8.0 * M * PP * OC,
         [=](hipStream_t st) { return unpatchify(lin, B, oc, S, S, p, P_->out, st); });
  return DM_OK;
}

}  // namespace dm

// ===========================================================================
// C ABI
// ===========================================================================
struct dm_dit {
  dm::DiTModel* m;
};

extern "C" int dm_dit_param_count(const dm_dit_arch* arch, int* n_params) {
  int rc = dm::dit_validate(arch);
  if (rc) return rc;
  if (!n_params) { dm::set_error("n_params is null"); return DM_ERR_ARG; }
  *n_params = dm::dit_count(*arch);
  return DM_OK;
}

extern "C" int dm_dit_create(const dm_dit_arch* arch, const float* const* params, const int64_t* numels,
                             int n_params, void* stream, dm_dit** out) {
  if (!out || !params || !numels) { dm::set_error("null argument"); return DM_ERR_ARG; }
  dm::DiTModel* m = nullptr;
  int rc = dm::dit_create(arch, nullptr, params, numels, n_params, (hipStream_t)stream, &m);
  if (rc) return rc;
  *out = new dm_dit{m};
  return DM_OK;
}

// dm_dit_forward and dm_mdt_forward
static int dit_forward(dm::DiTModel* m, const float* x, const int64_t* t, const int64_t* y, int B, float* out,
                       hipStream_t st) {
  DM_ABI_MODEL(m);
  if (!x || !t || !out) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  if (B <= 0) { dm::set_error("empty batch"); return DM_ERR_ARG; }
  if (static_cast<const void*>(out) == static_cast<const void*>(x)) {
    dm::set_error("out must not alias x");
    return DM_ERR_ARG;
  }
  const int S = m->arch.input_size;
  const size_t nx = (size_t)B * m->arch.in_channels * S * S, no = (size_t)B * m->OC * S * S;
  using Plan = dm::DiTModel::Plan;
  return dm::run_forward(
      *m, st, [&](int math, Plan** pl) { return m->get_plan(B, math, pl); },
      [&](Plan& pl) {
        DM_CHECK_HIP(hipMemcpyAsync(pl.x, x, nx * sizeof(float), hipMemcpyDeviceToDevice, st));
        DM_CHECK_HIP(hipMemcpyAsync(pl.t, t, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        if (y)
          DM_CHECK_HIP(hipMemcpyAsync(pl.y, y, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        else
          DM_CHECK_HIP(hipMemsetAsync(pl.y, 0xff, (size_t)B * sizeof(int64_t), st));  // -1: the null class
        return DM_OK;
      },
      [&](Plan& pl) {
        DM_CHECK_HIP(hipMemcpyAsync(out, pl.out, no * sizeof(float), hipMemcpyDeviceToDevice, st));
        return DM_OK;
      });
}

extern "C" int dm_dit_forward(dm_dit* h, const float* x, const int64_t* t, const int64_t* y, int B, float* out,
                              void* stream) {
  return dit_forward(dm::model_of(h), x, t, y, B, out, (hipStream_t)stream);
}
extern "C" int dm_dit_set_range_deferred(dm_dit* h, int deferred) {
  return dm::abi_set_range_deferred(dm::model_of(h), deferred);
}
extern "C" int dm_dit_range_poll(dm_dit* h, void* stream, int* flagged) {
  return dm::abi_range_poll(dm::model_of(h), (hipStream_t)stream, flagged);
}
extern "C" int dm_dit_range_fallback(dm_dit* h, int on) { return dm::abi_range_fallback(dm::model_of(h), on); }
extern "C" int dm_dit_range_stats(const dm_dit* h, int64_t* fallbacks, int* active) {
  return dm::abi_range_stats(dm::model_of(h), fallbacks, active);
}
extern "C" int dm_dit_set_math(dm_dit* h, int kind) { return dm::abi_set_math(dm::model_of(h), kind, false, true); }
extern "C" int dm_dit_get_math(const dm_dit* h, int* kind) { return dm::abi_get_math(dm::model_of(h), kind); }
extern "C" int dm_dit_set_time_freqs(dm_dit* h, const float* freqs, int n, void* stream) {
  return dm::abi_set_time_freqs(dm::model_of(h), freqs, n, (hipStream_t)stream);
}
extern "C" int dm_dit_profile(dm_dit* h, int enable) { return dm::abi_profile(dm::model_of(h), enable); }
extern "C" int dm_dit_profile_count(dm_dit* h, int* n_ops) { return dm::abi_profile_count(dm::model_of(h), n_ops); }
extern "C" int dm_dit_profile_get(dm_dit* h, int i, char* label, int label_len, double* flops, double* bytes,
                                  double* ms_total, int64_t* launches) {
  return dm::abi_profile_get(dm::model_of(h), i, label, label_len, flops, bytes, ms_total, launches);
}
extern "C" int dm_dit_memory(const dm_dit* h, int64_t* weight_bytes, int64_t* workspace_bytes) {
  return dm::abi_memory(dm::model_of(h), weight_bytes, workspace_bytes);
}
extern "C" int dm_dit_plan_stats(const dm_dit* h, int64_t* builds, int* cached) {
  return dm::abi_plan_stats(dm::model_of(h), builds, cached);
}
extern "C" void dm_dit_destroy(dm_dit* h) { dm::abi_destroy(h); }

// ===========================================================================
// C ABI: MDTv2 (the same model object and the same calls as dm_dit_*)
// ===========================================================================
struct dm_mdt {
  dm::DiTModel* m;
};

extern "C" int dm_mdt_param_count(const dm_mdt_arch* arch, int* n_params) {
  int rc = dm::mdt_validate(arch);
  if (rc) return rc;
  if (!n_params) { dm::set_error("n_params is null"); return DM_ERR_ARG; }
  *n_params = dm::mdt_count(*arch);
  return DM_OK;
}

extern "C" int dm_mdt_create(const dm_mdt_arch* arch, const float* const* params, const int64_t* numels,
                             int n_params, void* stream, dm_mdt** out) {
  if (!out || !params || !numels || !arch) { dm::set_error("null argument"); return DM_ERR_ARG; }
  const dm_dit_arch base = dm::mdt_base(*arch);
  dm::DiTModel* m = nullptr;
  int rc = dm::dit_create(&base, arch, params, numels, n_params, (hipStream_t)stream, &m);
  if (rc) return rc;
  *out = new dm_mdt{m};
  return DM_OK;
}

extern "C" int dm_mdt_forward(dm_mdt* h, const float* x, const int64_t* t, const int64_t* y, int B, float* out,
                              void* stream) {
  return dit_forward(dm::model_of(h), x, t, y, B, out, (hipStream_t)stream);
}
extern "C" int dm_mdt_set_range_deferred(dm_mdt* h, int deferred) {
  return dm::abi_set_range_deferred(dm::model_of(h), deferred);
}
extern "C" int dm_mdt_range_poll(dm_mdt* h, void* stream, int* flagged) {
  return dm::abi_range_poll(dm::model_of(h), (hipStream_t)stream, flagged);
}
extern "C" int dm_mdt_range_fallback(dm_mdt* h, int on) { return dm::abi_range_fallback(dm::model_of(h), on); }
extern "C" int dm_mdt_range_stats(const dm_mdt* h, int64_t* fallbacks, int* active) {
  return dm::abi_range_stats(dm::model_of(h), fallbacks, active);
}
extern "C" int dm_mdt_set_math(dm_mdt* h, int kind) { return dm::abi_set_math(dm::model_of(h), kind, false, true); }
extern "C" int dm_mdt_get_math(const dm_mdt* h, int* kind) { return dm::abi_get_math(dm::model_of(h), kind); }
extern "C" int dm_mdt_set_time_freqs(dm_mdt* h, const float* freqs, int n, void* stream) {
  return dm::abi_set_time_freqs(dm::model_of(h), freqs, n, (hipStream_t)stream);
}
extern "C" int dm_mdt_profile(dm_mdt* h, int enable) { return dm::abi_profile(dm::model_of(h), enable); }
extern "C" int dm_mdt_profile_count(dm_mdt* h, int* n_ops) { return dm::abi_profile_count(dm::model_of(h), n_ops); }
extern "C" int dm_mdt_profile_get(dm_mdt* h, int i, char* label, int label_len, double* flops, double* bytes,
                                  double* ms_total, int64_t* launches) {
  return dm::abi_profile_get(dm::model_of(h), i, label, label_len, flops, bytes, ms_total, launches);
}
extern "C" int dm_mdt_memory(const dm_mdt* h, int64_t* weight_bytes, int64_t* workspace_bytes) {
  return dm::abi_memory(dm::model_of(h), weight_bytes, workspace_bytes);
}
extern "C" int dm_mdt_plan_stats(const dm_mdt* h, int64_t* builds, int* cached) {
  return dm::abi_plan_stats(dm::model_of(h), builds, cached);
}
extern "C" void dm_mdt_destroy(dm_mdt* h) { dm::abi_destroy(h); }
