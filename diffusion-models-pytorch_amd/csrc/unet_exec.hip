// Native executor for the DDPM UNet denoiser (models/unet.py:46-152).
//
// Build time (dm_unet_create): the reference state_dict tensors are consumed
// in registration order, checked against the expected element counts, and
// packed into one library-owned device arena:
//   - 3x3 / 1x1 conv weights -> implicit-GEMM layout [Cout][K] (k = tap*Cin + c);
//     a ResBlock's 1x1 shortcut is appended to its second conv's K
//     (W2 | Wsc, bias b2 + bsc) so the shortcut is one more K segment;
//   - q, k, v 1x1 convs -> one [3C][C] weight (single QKV GEMM);
//   - every ResBlock's time projection -> one [sum Cout][4*dim] weight, so the
//     per-step projections of all blocks are a single GEMM.
// Forward (dm_unet_forward): a flat list of launches on one stream over a
// per-batch workspace. Activations are NHWC; skip tensors are written by
// their producer directly into the channel slice of the up-path block that
// concatenates them (models/unet.py:145), so torch.cat never materialises.
#include <memory>
#include <vector>
#include <functional>
#include <cmath>
#include <map>
#include <set>

#include "dm_common.h"
#include "dm_kernels.h"
#include "plan.h"
#include "exec_pack.h"
#include "exec_core.h"

namespace dm {

namespace {

struct GnP { size_t g, b; int C; };
struct ConvP {
  size_t w, bias;
  int Cout, Cin, taps, K;
  size_t w_sub = 0;  // sub-pixel weights [4][Cout][4 Cin] of an upsample conv (0 = none)
  size_t w_subw = 0;  // sub-pixel Winograd U matrices [6][Cout][2 Cin] of an Upsample conv (0 = none)
  bool has_subw = false;
};

struct ResBlockP {
  int cin, cout;
  GnP gn1, gn2;
  ConvP conv1, conv2;  // conv2 carries the shortcut segment when cin != cout
  int proj_col;        // column offset of this block's projection in the fused proj output
                       // (variant 0: temb add [cout]; variant 1: AdaGN [ys | yb], 2 * cout)
  bool adagn = false;  // variant 1: AdaGN before conv2 instead of the temb add after conv1
  int updown = 0;      // variant 1: 0 none, 1 nearest-2x up, 2 avg-pool down (unet_categorial_adagn.py:24-27)
};

struct AttnP {
  int C, heads;
  bool legacy = false;  // ADM QKVAttentionLegacy: head h owns qkv channels [h*3d, (h+1)*3d) = [q; k; v]
  float sa = 1.f, sb = 0.f;  // scale applied to q (and to k when sb != 0) elements
  GnP gn;
  size_t wqkv, bqkv, wproj, bproj;
};

enum NodeKind { N_RES, N_ATTN, N_DOWN, N_UP };

}  // namespace

namespace {

struct Node {
  NodeKind kind;
  int idx;        // index into res/attn/conv vectors
  int cin, cout;  // channels in/out
  int h_in;       // input resolution (relative to image H; H / 2^level)
  int level_in, level_out;
  bool skip_producer = false;
  int skip_id = -1;       // id of the skip this node produces
  int pops_skip = -1;     // for up-RBs: id of the skip consumed
  int concat_cx = 0;      // for up-RBs: channels of the X part
};

}  // namespace

// (the weight arena, the arithmetic -- fallback bf16x3 -- and the split / Winograd weights: ExecNet, exec_core.h)
struct UNetModel : ExecNet {
  dm_unet_arch arch;
  // packed parameters (offsets into arena)
  size_t te_w1, te_b1, te_w2, te_b2;
  size_t freqs;            // [n_freqs = dim/2] sinusoid frequencies
  int n_freqs = 0;
  bool freqs_set = false;  // host table installed (else computed on device)
  size_t class_embed = 0;     // variants 1, 2: [num_classes][4 dim]
  bool has_class = false;
  size_t first_w, first_b;
  size_t proj_w, proj_b;
  int proj_total = 0;
  GnP last_gn;
  size_t last_w, last_b;
  std::vector<ResBlockP> res;
  std::vector<AttnP> attn;
  std::vector<ConvP> convs;  // down / up sample convs
  std::vector<Node> nodes;
  std::vector<int> skip_C, skip_level;  // per skip id
  int n_levels = 0;
  float norm_eps = 1e-5f;  // every GroupNorm's eps: nn.GroupNorm's default; variant 3: 1e-6 (pesser/model.py:33)

  // plan cache (LRU over (B, H, W)), scratch from a pool shared with dm_unet_share_workspace peers
  struct Plan : PlanBase {
    int B = 0, H = 0, W = 0;
    int math = 0;   // the arithmetic the plan was built with (conv_math at build time)
    bool half = false;  // built with the conv-half option in effect (an fp16x2 plan of a model with conv_half set)
    // plan-owned staging of the caller's tensors (every launch reads fixed pointers: graph replay)
    float* x = nullptr;
    int64_t* t = nullptr;
    int64_t* y = nullptr;  // class labels; all -1 when the caller passes none
    float* out = nullptr;
  };
  PlanCache<Plan> plans;
  float* last_packed = nullptr;  // last conv weights as [9][Cin][CO] (small_out_pack), made at the first build
  // folded single-head attention blocks (attn_block.hip): per block's qkv weights, the fp32 products At, w,
  // Wg, cb and the fp16x2 fragment images of At and Wg' (Wg with permuted columns), made at the first fp16x2
  // plan build
  using FoldW = AttnFoldW;  // (attn_fold_all, attn_block.hip)
  std::map<size_t, FoldW> folds;
  std::vector<void*> fold_mem;
  const FoldW* fold_for(const AttnP& p);

  UNetModel() { wino_small = true; }
  ~UNetModel() {
    for (void* q : fold_mem) (void)hipFree(q);
    if (last_packed) (void)hipFree(last_packed);
  }
  int build_plan(Plan& pl, int B, int H, int W);
  int get_plan(int B, int H, int W, int math, Plan** out) {
    conv_math = math;
    const bool half = half_active();
    return plans.get([&](const Plan& p) { return p.B == B && p.H == H && p.W == W && p.math == math && p.half == half; },
                     [&](Plan& p) { return build_plan(p, B, H, W); }, out);
  }
};

// The folded weights of a single-head attention block (attn_fold, float64 products of the block's own
// weights) and their fp16x2 images; null if an allocation or launch fails (the block then runs unfolded).
const UNetModel::FoldW* UNetModel::fold_for(const AttnP& p) {
  auto it = folds.find(p.wqkv);
  if (it != folds.end()) return it->second.at ? &it->second : nullptr;  // a failed fold stays failed
  const int C = p.C;
  FoldW f;
  void* mem = nullptr;
  const size_t nb = attn_fold_bytes(C);
  if (hipMalloc(&mem, nb) != hipSuccess) {
    (void)hipGetLastError();
    folds[p.wqkv] = FoldW{};  // plan builds stay deterministic: every later build sees the same failure
    return nullptr;
  }
  fold_mem.push_back(mem);
  const double s = (double)p.sa * (p.sb != 0.f ? (double)p.sb : 1.0);
  if (attn_fold_all(P(p.wqkv), P(p.bqkv), P(p.wproj), P(p.bproj), C, s, mem, &f, nullptr) != DM_OK ||
      hipDeviceSynchronize() != hipSuccess) {
    folds[p.wqkv] = FoldW{};
    return nullptr;
  }
  split_bytes += nb - 64;  // (the fold results and images; not the allocation's 64 bytes of alignment slack)
  return &(folds[p.wqkv] = f);
}

// Channels of the first conv / last conv input: dim (models/unet.py:72) or
// channel_mult[0] * model_channels (models/adm/unet.py:499).
static int first_channels(const dm_unet_arch& a) { return a.variant == 2 ? a.dim * a.dim_mults[0] : a.dim; }

// Heads of an attention block with C channels; where: 0 down path, 1 bottleneck, 2 up path.
static int attn_heads(const dm_unet_arch& a, int C, int where) {
  if (a.variant == 3) return 1;  // AttnBlock: one head of C channels (pesser/model.py:171-176)
  if (a.variant == 2) {  // models/adm/unet.py:296-302, 470-471, 606
    if (a.attn_head_dims > 0) return C / a.attn_head_dims;
    return where == 2 ? a.n_heads_up : a.n_heads;
  }
  if (where == 1) return 1;  // SelfAttentionBlock(cur_dim) default n_heads (unet.py:95)
  return a.variant == 1 ? C / a.attn_head_dims : a.n_heads;
}

static int count_params(const dm_unet_arch& a) {
  // mirrors the registration order of models/unet.py:47-119 (variant 1:
  // models/unet_categorial_adagn.py:77-163; variant 2: models/adm/unet.py:489-635; variant 3:
  // models/pesser/model.py:203-285, the same tensors as variant 0 in another order: walk_order below)
  int n = 4 + 2;  // time_embed (2 linears), first conv
  if (a.variant >= 1 && a.num_classes > 0) n += 1;  // class_embed.weight / label_emb.weight
  auto rb = [](int cin, int cout) { return 10 + (cin != cout ? 2 : 0); };
  const int attn = a.variant == 2 ? 6 : 10;  // norm, qkv, proj_out  |  norm, q, k, v, proj
  const bool rb_updown = a.variant >= 1 && a.resblock_updown;
  const int resample = (a.variant == 2 && a.pool_resample) ? 0 : 2;  // conv down/up-sample parameters
  int cur = first_channels(a);
  std::vector<int> dims{cur};
  for (int i = 0; i < a.n_stages; ++i) {
    int out = a.dim * a.dim_mults[i];
    for (int j = 0; j < a.num_res_blocks; ++j) {
      n += rb(cur, out);
      if (a.use_attn[i]) n += attn;
      dims.push_back(out);
      cur = out;
    }
    if (i < a.n_stages - 1) {
      n += rb_updown ? rb(out, out) : resample;  // ResBlock(down) or Downsample
      dims.push_back(out);
    }
  }
  n += rb(cur, cur) * 2 + attn;
  for (int i = a.n_stages - 1; i >= 0; --i) {
    int out = a.dim * a.dim_mults[i];
    for (int j = 0; j < a.num_res_blocks + 1; ++j) {
      int s = dims.back();
      dims.pop_back();
      n += rb(s + cur, out);
      if (a.use_attn[i]) n += attn;
      cur = out;
    }
    if (i > 0) n += rb_updown ? rb(out, out) : resample;  // ResBlock(up) or Upsample
  }
  n += 4;  // last GN + conv
  return n;
}

static int validate_arch(const dm_unet_arch* a) {
  DM_REQUIRE(a != nullptr, "arch is null");
  DM_REQUIRE(a->n_stages >= 1 && a->n_stages <= DM_MAX_STAGES, "n_stages out of range");
  DM_REQUIRE(a->dim >= 32 && a->dim % 32 == 0, "dim must be a positive multiple of 32");
  DM_REQUIRE(a->in_channels >= 1 && a->in_channels <= 4, "in_channels out of range (1..4)");
  DM_REQUIRE(a->out_channels >= 1 && a->out_channels <= 8, "out_channels out of range (1..8)");
  DM_REQUIRE(a->num_res_blocks >= 1, "num_res_blocks must be >= 1");
  DM_REQUIRE(a->variant >= 0 && a->variant <= 3,
             "variant must be 0 (UNet), 1 (UNetCategorialAdaGN), 2 (ADM UNetModel) or 3 (pesser Model)");
  if (a->variant == 0) DM_REQUIRE(a->n_heads >= 1, "n_heads must be >= 1");
  if (a->variant == 1) DM_REQUIRE(a->attn_head_dims >= 1, "attn_head_dims must be >= 1");
  if (a->variant == 2 && a->attn_head_dims <= 0)
    DM_REQUIRE(a->n_heads >= 1 && a->n_heads_up >= 1, "num_heads / num_heads_upsample must be >= 1");
  DM_REQUIRE(a->num_classes >= 0, "num_classes must be >= 0");
  for (int i = 0; i < a->n_stages; ++i) {
    DM_REQUIRE(a->dim_mults[i] >= 1, "dim_mults must be >= 1");
    const int c = a->dim * a->dim_mults[i];
    DM_REQUIRE(c % 32 == 0, "stage channels must be multiples of 32 (GroupNorm(32) / MFMA tiles)");
    if (a->use_attn[i]) {
      for (int where : {0, 2}) {
        const int h = attn_heads(*a, c, where);
        DM_REQUIRE(h >= 1 && c % h == 0 && (c / h) % 4 == 0, "attention channels not divisible by heads");
      }
    }
  }
  const int cb = a->dim * a->dim_mults[a->n_stages - 1];
  const int hb = attn_heads(*a, cb, 1);
  DM_REQUIRE(hb >= 1 && cb % hb == 0 && (cb / hb) % 4 == 0, "bottleneck channels not divisible by heads");
  return DM_OK;
}

// Variant 3 (models/pesser/model.py) registers a level's ResnetBlocks, then its AttnBlocks, then its Downsample
// (:220-240), and stores `up` by level (self.up.insert(0, ...), :277) although the forward runs it from the deepest
// level (:314). order[i] = the state_dict index of the i-th tensor of the executor's walk (block, its attention,
// ..., resample; up path deepest level first), which is variant 0's registration order.
static std::vector<int> walk_order(const dm_unet_arch& a) {
  auto rb = [](int cin, int cout) { return 10 + (cin != cout ? 2 : 0); };
  const int attn = 10, L = a.n_stages, R = a.num_res_blocks;
  std::vector<int> order;
  auto run = [&](int first, int n) {
    for (int i = 0; i < n; ++i) order.push_back(first + i);
  };
  int pos = 0;
  run(pos, 6);  // temb.dense.{0,1}, conv_in
  pos += 6;
  int cur = a.dim;
  std::vector<int> dims{cur};
  for (int i = 0; i < L; ++i) {
    const int out = a.dim * a.dim_mults[i];
    std::vector<int> blk;  // first index of each block
    int p = pos;
    for (int j = 0; j < R; ++j) {
      blk.push_back(p);
      p += rb(j == 0 ? cur : out, out);
    }
    const int attn0 = p;
    if (a.use_attn[i]) p += attn * R;
    for (int j = 0; j < R; ++j) {
      run(blk[j], rb(j == 0 ? cur : out, out));
      if (a.use_attn[i]) run(attn0 + attn * j, attn);
      dims.push_back(out);
    }
    cur = out;
    if (i < L - 1) {
      run(p, 2);
      p += 2;
      dims.push_back(out);
    }
    pos = p;
  }
  const int mid = rb(cur, cur) * 2 + attn;
  run(pos, mid);
  pos += mid;
  // up levels as the forward meets them (deepest first): their block input widths, then their state_dict offsets
  std::vector<std::vector<int>> cin(L);
  for (int i = L - 1; i >= 0; --i) {
    const int out = a.dim * a.dim_mults[i];
    for (int j = 0; j < R + 1; ++j) {
      cin[i].push_back(dims.back() + cur);
      dims.pop_back();
      cur = out;
    }
  }
  std::vector<int> first(L);
  for (int i = 0; i < L; ++i) {
    first[i] = pos;
    for (int j = 0; j < R + 1; ++j) pos += rb(cin[i][j], a.dim * a.dim_mults[i]);
    if (a.use_attn[i]) pos += attn * (R + 1);
    if (i > 0) pos += 2;
  }
  for (int i = L - 1; i >= 0; --i) {
    const int out = a.dim * a.dim_mults[i];
    int p = first[i];
    std::vector<int> blk;
    for (int j = 0; j < R + 1; ++j) {
      blk.push_back(p);
      p += rb(cin[i][j], out);
    }
    for (int j = 0; j < R + 1; ++j) {
      run(blk[j], rb(cin[i][j], out));
      if (a.use_attn[i]) run(p + attn * j, attn);
    }
    if (a.use_attn[i]) p += attn * (R + 1);
    if (i > 0) run(p, 2);
  }
  run(pos, 4);  // norm_out, conv_out
  return order;
}

// ---------------------------------------------------------------------------
// create
// ---------------------------------------------------------------------------
static int unet_create(const dm_unet_arch* arch, const float* const* params, const int64_t* numels, int n_params,
                       hipStream_t st, UNetModel** out) {
  int rc = validate_arch(arch);
  if (rc) return rc;
  const dm_unet_arch a = *arch;
  const int expect = count_params(a);
  DM_REQUIRE(n_params == expect, "expected " + std::to_string(expect) + " parameter tensors, got " +
                                     std::to_string(n_params));
  refresh_toggles();  // the model's arithmetic and range check (member initialisers) from this snapshot
  auto m = std::make_unique<UNetModel>();
  m->arch = a;
  if (a.variant == 3) m->norm_eps = 1e-6f;
  // variant 3: the caller's tensors re-ordered into the walk's order
  std::vector<const float*> wparams;
  std::vector<int64_t> wnumels;
  if (a.variant == 3) {
    const std::vector<int> order = walk_order(a);
    DM_REQUIRE((int)order.size() == n_params, "variant 3: parameter order table does not cover the state_dict");
    std::vector<char> seen(n_params, 0);
    for (int idx : order) {
      DM_REQUIRE(idx >= 0 && idx < n_params && !seen[idx], "variant 3: parameter order table is not a permutation");
      seen[idx] = 1;
      wparams.push_back(params[idx]);
      wnumels.push_back(numels[idx]);
    }
    params = wparams.data();
    numels = wnumels.data();
  }
  ParamReader rd{params, numels, n_params};
  Packer pk;
  const int D = a.dim, TD = 4 * a.dim, C0 = first_channels(a);
  const bool adm = a.variant == 2;

  // time embedding MLP: Linear(D, 4D) -> SiLU -> Linear(4D, 4D)
  m->te_w1 = pk.raw(rd.take((int64_t)TD * D, "time_embed Linear 1 weight"), (int64_t)TD * D);
  m->te_b1 = pk.raw(rd.take(TD, "time_embed Linear 1 bias"), TD);
  m->te_w2 = pk.raw(rd.take((int64_t)TD * TD, "time_embed Linear 2 weight"), (int64_t)TD * TD);
  m->te_b2 = pk.raw(rd.take(TD, "time_embed Linear 2 bias"), TD);
  m->freqs = pk.reserve(D / 2);
  m->n_freqs = D / 2;
  if (a.variant >= 1 && a.num_classes > 0) {  // unet_categorial_adagn.py:104, adm/unet.py:496-497
    m->class_embed = pk.raw(rd.take((int64_t)a.num_classes * TD, "class_embed / label_emb weight"),
                            (int64_t)a.num_classes * TD);
    m->has_class = true;
  }
  m->first_w = pk.raw(rd.take((int64_t)C0 * a.in_channels * 9, "first conv weight"), (int64_t)C0 * a.in_channels * 9);
  m->first_b = pk.raw(rd.take(C0, "first conv bias"), C0);

  // Projections are collected then packed into one matrix after the walk.
  struct ProjSrc { const float* w; const float* b; int cout; };
  std::vector<ProjSrc> projs;

  auto gn = [&](int C, const char* what) {
    GnP g;
    g.C = C;
    g.g = pk.raw(rd.take(C, what), C);
    g.b = pk.raw(rd.take(C, what), C);
    return g;
  };
  // variant 0 (models/unet.py:14-44): blk1 (GN, conv), proj, blk2 (GN, conv), shortcut
  // variant 1 (models/unet_categorial_adagn.py:31-42): blk1 (GN, conv), adagn (gn, proj -> 2 cout),
  //           blk2 conv, shortcut
  // variant 2 (models/adm/unet.py:201-241): in_layers (GN, conv), emb_layers (Linear -> cout or 2 cout
  //           with use_scale_shift_norm), out_layers (GN, conv), skip_connection
  auto resblock = [&](int cin, int cout, int updown) {
    ResBlockP r;
    r.cin = cin;
    r.cout = cout;
    r.adagn = a.variant == 1 || (adm && a.scale_shift_norm);
    r.updown = updown;
    r.gn1 = gn(cin, "ResBlock.blk1.0 (GroupNorm)");
    const float* w1 = rd.take((int64_t)cout * cin * 9, "ResBlock.blk1.2.weight");
    const float* b1 = rd.take(cout, "ResBlock.blk1.2.bias");
    r.conv1 = {0, 0, cout, cin, 9, 9 * cin};
    r.conv1.w = pk.reserve((int64_t)cout * 9 * cin);
    pk.conv_at(w1, cout, cin, 9, 9 * cin, 0, r.conv1.w);
    r.conv1.bias = pk.raw(b1, cout);
    if (updown == 1) r.conv1.w_sub = pk.subpix(w1, cout, cin);  // nearest-2x folded into conv1
    const int pn = r.adagn ? 2 * cout : cout;
    const bool gn2_first = a.variant == 1;  // AdaGN registers its gn before its proj
    if (gn2_first) r.gn2 = gn(cout, "ResBlock.adagn.gn");
    const float* pw = rd.take((int64_t)pn * TD, r.adagn ? "ResBlock.adagn.proj.1.weight" : "ResBlock.proj.1.weight");
    const float* pb = rd.take(pn, r.adagn ? "ResBlock.adagn.proj.1.bias" : "ResBlock.proj.1.bias");
    r.proj_col = m->proj_total;
    m->proj_total += pn;
    projs.push_back({pw, pb, pn});
    if (!gn2_first) r.gn2 = gn(cout, "ResBlock second GroupNorm");
    const float* w2 = rd.take((int64_t)cout * cout * 9, "ResBlock.blk2 conv weight");
    const float* b2 = rd.take(cout, "ResBlock.blk2 conv bias");
    const int K2 = 9 * cout + (cin != cout ? cin : 0);
    r.conv2 = {0, 0, cout, cout, 9, K2};
    r.conv2.w = pk.reserve((int64_t)cout * K2);
    pk.conv_at(w2, cout, cout, 9, K2, 0, r.conv2.w);
    if (cin != cout) {
      const float* ws = rd.take((int64_t)cout * cin, "ResBlock.shortcut.weight");
      const float* bs = rd.take(cout, "ResBlock.shortcut.bias");
      pk.conv_at(ws, cout, cin, 1, K2, 9 * cout, r.conv2.w);
      r.conv2.bias = pk.reserve(cout);
      pk.add_at(b2, bs, cout, r.conv2.bias);
    } else {
      r.conv2.bias = pk.raw(b2, cout);
    }
    m->res.push_back(r);
    return (int)m->res.size() - 1;
  };
  auto attnblock = [&](int C, int heads) {
    AttnP p;
    p.C = C;
    p.heads = heads;
    const int Dh = C / heads;
    if (adm) {
      // AttentionBlock (adm/unet.py:304-313): norm, qkv Conv1d [3C][C], proj_out Conv1d [C][C];
      // q and k each scaled by ch^-1/4 (adm/unet.py:367-370)
      p.legacy = a.attn_legacy != 0;
      p.sa = p.sb = (float)(1.0 / std::sqrt(std::sqrt((double)Dh)));
      p.gn = gn(C, "AttentionBlock.norm");
      p.wqkv = pk.raw(rd.take((int64_t)3 * C * C, "AttentionBlock.qkv.weight"), (int64_t)3 * C * C);
      p.bqkv = pk.raw(rd.take(3 * C, "AttentionBlock.qkv.bias"), 3 * C);
      p.wproj = pk.raw(rd.take((int64_t)C * C, "AttentionBlock.proj_out.weight"), (int64_t)C * C);
      p.bproj = pk.raw(rd.take(C, "AttentionBlock.proj_out.bias"), C);
      m->attn.push_back(p);
      return (int)m->attn.size() - 1;
    }
    // SelfAttentionBlock (modules.py:78-87): q * (C/heads)^-1/2 (modules.py:95)
    p.sa = (float)std::pow((double)Dh, -0.5);
    p.sb = 0.f;
    p.gn = gn(C, "SelfAttentionBlock.norm");
    p.wqkv = pk.reserve((int64_t)3 * C * C);
    p.bqkv = pk.reserve(3 * C);
    for (int i = 0; i < 3; ++i) {
      const float* w = rd.take((int64_t)C * C, "SelfAttentionBlock.{q,k,v}.weight");
      const float* b = rd.take(C, "SelfAttentionBlock.{q,k,v}.bias");
      pk.raw_at(w, (int64_t)C * C, p.wqkv + (size_t)i * C * C);
      pk.raw_at(b, C, p.bqkv + (size_t)i * C);
    }
    p.wproj = pk.raw(rd.take((int64_t)C * C, "SelfAttentionBlock.proj.weight"), (int64_t)C * C);
    p.bproj = pk.raw(rd.take(C, "SelfAttentionBlock.proj.bias"), C);
    m->attn.push_back(p);
    return (int)m->attn.size() - 1;
  };
  auto sampleconv = [&](int C, const char* what) {
    if (adm && a.pool_resample) return -1;  // avg-pool / nearest only (adm/unet.py:126-128, 153-155)
    ConvP c{0, 0, C, C, 9, 9 * C};
    const float* w = rd.take((int64_t)C * C * 9, what);
    const float* b = rd.take(C, what);
    c.w = pk.reserve((int64_t)C * 9 * C);
    pk.conv_at(w, C, C, 9, 9 * C, 0, c.w);
    c.bias = pk.raw(b, C);
    if (std::string(what) == "Upsample") {
      c.w_sub = pk.subpix(w, C, C);
      if (C % 128 == 0) {  // (the channel counts conv_subwino takes)
        c.w_subw = pk.subwino(w, C, C);
        c.has_subw = true;
      }
    }
    m->convs.push_back(c);
    return (int)m->convs.size() - 1;
  };

  const bool rb_updown = a.variant >= 1 && a.resblock_updown;
  // ---- down path (models/unet.py:77-90, forward :126-136; adm/unet.py:506-556, forward :674-676)
  int cur = C0, level = 0, n_skips = 0;
  std::vector<int> skip_stack;  // skip ids
  auto push_skip = [&](int C, int lvl) {
    m->skip_C.push_back(C);
    m->skip_level.push_back(lvl);
    skip_stack.push_back(n_skips);
    return n_skips++;
  };
  const int s0 = push_skip(C0, 0);  // first conv output
  (void)s0;
  for (int i = 0; i < a.n_stages; ++i) {
    const int out = D * a.dim_mults[i];
    for (int j = 0; j < a.num_res_blocks; ++j) {
      Node n{N_RES, resblock(cur, out, 0), cur, out, 0, level, level};
      m->nodes.push_back(n);
      if (a.use_attn[i]) {
        Node na{N_ATTN, attnblock(out, attn_heads(a, out, 0)), out, out, 0, level, level};
        m->nodes.push_back(na);
      }
      m->nodes.back().skip_producer = true;
      m->nodes.back().skip_id = push_skip(out, level);
      cur = out;
    }
    if (i < a.n_stages - 1) {
      if (rb_updown)
        m->nodes.push_back(Node{N_RES, resblock(out, out, 2), out, out, 0, level, level + 1});
      else
        m->nodes.push_back(Node{N_DOWN, sampleconv(out, "Downsample"), out, out, 0, level, level + 1});
      ++level;
      m->nodes.back().skip_producer = true;
      m->nodes.back().skip_id = push_skip(out, level);
    }
  }
  m->n_levels = level + 1;
  // ---- bottleneck (models/unet.py:93-97; adm/unet.py:558-582)
  m->nodes.push_back(Node{N_RES, resblock(cur, cur, 0), cur, cur, 0, level, level});
  m->nodes.push_back(Node{N_ATTN, attnblock(cur, attn_heads(a, cur, 1)), cur, cur, 0, level, level});
  m->nodes.push_back(Node{N_RES, resblock(cur, cur, 0), cur, cur, 0, level, level});
  // ---- up path (models/unet.py:101-112, forward :142-149)
  for (int i = a.n_stages - 1; i >= 0; --i) {
    const int out = D * a.dim_mults[i];
    for (int j = 0; j < a.num_res_blocks + 1; ++j) {
      const int sid = skip_stack.back();
      skip_stack.pop_back();
      const int cin = cur + m->skip_C[sid];
      Node n{N_RES, resblock(cin, out, 0), cin, out, 0, level, level};
      n.pops_skip = sid;
      n.concat_cx = cur;
      m->nodes.push_back(n);
      if (a.use_attn[i])
        m->nodes.push_back(Node{N_ATTN, attnblock(out, attn_heads(a, out, 2)), out, out, 0, level, level});
      cur = out;
    }
    if (i > 0) {
      if (rb_updown)
        m->nodes.push_back(Node{N_RES, resblock(out, out, 1), out, out, 0, level, level - 1});
      else
        m->nodes.push_back(Node{N_UP, sampleconv(out, "Upsample"), out, out, 0, level, level - 1});
      --level;
    }
  }
  // ---- last conv (models/unet.py:115-119; adm/unet.py:631-635 `out`)
  m->last_gn = gn(cur, "last_conv.0 (GroupNorm)");
  m->last_w = pk.raw(rd.take((int64_t)a.out_channels * cur * 9, "last_conv.2.weight"), (int64_t)a.out_channels * cur * 9);
  m->last_b = pk.raw(rd.take(a.out_channels, "last_conv.2.bias"), a.out_channels);
  if (!rd.err.empty()) {
    set_error(rd.err);
    return DM_ERR_ARG;
  }
  DM_REQUIRE(rd.pos == n_params, "parameter count mismatch after walk");

  // fused projection matrix [proj_total][TD]
  m->proj_w = pk.reserve((int64_t)m->proj_total * TD);
  m->proj_b = pk.reserve(m->proj_total);
  {
    int row = 0;
    for (auto& p : projs) {
      pk.raw_at(p.w, (int64_t)p.cout * TD, m->proj_w + (size_t)row * TD);
      pk.raw_at(p.b, p.cout, m->proj_b + row);
      row += p.cout;
    }
  }

  // allocate + run the pack jobs
  m->arena_floats = pk.size;
  DM_CHECK_HIP(hipMalloc(&m->arena, pk.size * sizeof(float)));
  rc = run_pack_jobs(pk, m->arena, st);
  if (rc) return rc;
  *out = m.release();
  return DM_OK;
}

// ---------------------------------------------------------------------------
// plan (per batch size / resolution)
// ---------------------------------------------------------------------------
int UNetModel::build_plan(Plan& pl, int B, int H, int W) {
  refresh_toggles();
  pl.toggles = toggles();
  ToggleScope scope(pl.toggles);
  pl.graph_enabled = toggles().graph;
  pl.B = B;
  pl.math = conv_math;
  pl.half = half_active();
  pl.H = H;
  pl.W = W;
  if (const int rcf = ensure_range_flag()) return rcf;
  DM_REQUIRE(H % (1 << (n_levels - 1)) == 0 && W % (1 << (n_levels - 1)) == 0,
             "image size must be divisible by 2^(n_stages-1)");
  bool& alloc_failed = pl.alloc_failed;
  auto alloc = [&](size_t bytes) -> float* { return pl.alloc(bytes); };
  auto Hl = [&](int lvl) { return H >> lvl; };
  auto Wl = [&](int lvl) { return W >> lvl; };
  const int D = arch.dim, TD = 4 * arch.dim, G = 32, C0 = skip_C[0];
  const float gn_eps = norm_eps;

  // --- staging of x / t / y / out
  pl.x = alloc((size_t)B * arch.in_channels * H * W * 4);
  pl.t = (int64_t*)alloc((size_t)B * 8);
  pl.y = (int64_t*)alloc((size_t)B * 8);
  pl.out = alloc((size_t)B * arch.out_channels * H * W * 4);
  // --- temb workspace
  float* e0 = alloc((size_t)B * D * 4);
  float* e1 = alloc((size_t)B * TD * 4);
  float* se = alloc((size_t)B * TD * 4);
  float* e2 = has_class ? alloc((size_t)B * TD * 4) : nullptr;
  float* projs = alloc((size_t)B * proj_total * 4);

  // --- scratch sizes
  size_t max_a1 = 0, max_h = 0, max_attn = 0, max_qkv = 0, max_S = 0, max_xr = 0;
  int max_chunks = 1;
  for (auto& n : nodes) {
    const size_t hw = (size_t)Hl(n.level_in) * Wl(n.level_in);
    max_chunks = std::max(max_chunks, gn_num_chunks((int)hw));
    if (n.kind == N_RES) {
      // up/down ResBlocks convolve at the output resolution
      const size_t hw_o = (size_t)Hl(n.level_out) * Wl(n.level_out);
      max_chunks = std::max(max_chunks, gn_num_chunks((int)hw_o));
      max_a1 = std::max(max_a1, (size_t)B * std::max(hw, hw_o) * n.cin);
      max_h = std::max(max_h, (size_t)B * hw_o * n.cout);
      if (res[n.idx].updown) max_xr = std::max(max_xr, (size_t)B * hw_o * n.cin);
    } else if (n.kind == N_ATTN) {
      max_attn = std::max(max_attn, (size_t)B * hw * n.cin);
      max_qkv = std::max(max_qkv, (size_t)B * hw * 3 * n.cin);
      const int heads = attn[n.idx].heads;
      max_S = std::max(max_S, (size_t)B * heads * hw * hw);
    }
  }
  max_chunks = std::max(max_chunks, gn_num_chunks(H * W));
  float* a1 = alloc(std::max(max_a1, (size_t)B * H * W * C0) * 4);
  float* hbuf = alloc(max_h * 4);
  float* a2 = alloc(max_h * 4);
  float* an = alloc(std::max<size_t>(max_attn, 1) * 4);
  float* qkv = alloc(std::max<size_t>(max_qkv, 1) * 4);
  float* Sb = alloc(std::max<size_t>(max_S, 1) * 4);
  float* Ob = alloc(std::max<size_t>(max_attn, 1) * 4);
  float* xr = alloc(std::max<size_t>(max_xr, 1) * 4);  // resampled residual of up/down ResBlocks
  double2* part = (double2*)alloc((size_t)B * max_chunks * G * sizeof(double2));
  // per-(image, channel) GroupNorm affine for the fused conv prologues
  size_t max_c = (size_t)C0;
  for (auto& n : nodes) max_c = std::max(max_c, (size_t)std::max(n.cin, n.cout));
  float* gsc = alloc((size_t)B * max_c * 4);
  float* gsh = alloc((size_t)B * max_c * 4);
  // conv-half plans: the fp16 image planes of the covered convs' two segments (conv_h16_image), the largest once.
  // Only ResBlock convs can be covered (conv1: Cin1 = cin; conv2: Cin1 = cout, Cin2 = cin where the widths differ), at
  // the block's output resolution and on maps of >= 64 pixels: sized from those. add_conv checks every use against it.
  _Float16* h16_p1 = nullptr;
  _Float16* h16_p2 = nullptr;
  size_t h16_cap1 = 0, h16_cap2 = 0;  // fp16 elements
  bool h16_overflow = false;
  if (pl.half) {
    for (auto& n : nodes) {
      const size_t hw_o = (size_t)Hl(n.level_out) * Wl(n.level_out);
      if (n.kind != N_RES || hw_o < 64) continue;
      h16_cap1 = std::max(h16_cap1, (size_t)B * hw_o * std::max(n.cin, n.cout));
      if (n.cin != n.cout) h16_cap2 = std::max(h16_cap2, (size_t)B * hw_o * n.cin);
    }
    if (h16_cap1) h16_p1 = (_Float16*)alloc(h16_cap1 * 2);
    if (h16_cap2) h16_p2 = (_Float16*)alloc(h16_cap2 * 2);
  }

  // --- concat buffers for up-RBs and skip slot views
  std::vector<View> skip_view(skip_C.size());
  std::vector<View> concat_x(nodes.size());
  for (size_t i = 0; i < nodes.size(); ++i) {
    const Node& n = nodes[i];
    if (n.kind == N_RES && n.pops_skip >= 0) {
      const int lvl = n.level_in;
      float* buf = alloc((size_t)B * Hl(lvl) * Wl(lvl) * n.cin * 4);
      concat_x[i] = View{buf, B, Hl(lvl), Wl(lvl), n.concat_cx, n.cin};
      skip_view[n.pops_skip] = View{buf + n.concat_cx, B, Hl(lvl), Wl(lvl), skip_C[n.pops_skip], n.cin};
    }
  }
  if (alloc_failed) { set_error("workspace allocation failed"); return DM_ERR_HIP; }

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
  // Split-K for convs on maps of <= 16 pixels (e.g. the 4x4 level at CIFAR size): without it a
  // B=256 launch has only 256 tiles for 256 CUs. The split depends on the layer shape only, never on
  // B, so every image's result is the same at any batch size.
  float* kpart_ws = nullptr;
  size_t kpart_floats = 0;
  auto maybe_split = [&](ConvArgs& c) {
    if (c.upsample == 2 || c.taps != 9 || c.stride != 1 || c.Hout * c.Wout > 16) return;
    // the Winograd kernel on 4 x 4 maps (conv_wino.hip, fp16x2): 4 splits (64 tiles x 4 = 256 blocks at B = 256),
    // reduced by conv_splitk_reduce, where a split has >= 12 K steps of 32 channels (B = 256: 512 -> 256 33.2 us vs
    // conv_k32s 39.8 us; at 256 -> 256, 6 steps, 26.6 vs 22.8 us: the per-block prologue / epilogue and the
    // reduction pass dominate); else the K32 small-map kernel (conv_k32.hip): 2 splits inside the block (4x4
    // maps, B = 256: 32.5 us vs 37.8 us with 4, the reduction included); conv_patch3's 16-channel chunks: 4
    int ks = 0;
    if (conv_math == 2 && toggles().wino && wino_small_ks(c)) {
      ConvArgs w = c;
      w.ksplit = wino_small_ks(c);
      w.kpart = conv_standin<float>();
      if (conv_wino_shape_ok(w)) ks = w.ksplit;
    }
    if (!ks) {
      if (!conv_choose(c).takes_prologue) return;
      ks = std::min(2, c.Cin1 / 32);
      if (ks < 2) return;
    }
    const size_t need = (size_t)ks * c.B * c.Hout * c.Wout * c.Cout;
    if (need > kpart_floats) {
      kpart_ws = alloc(need * 4);
      kpart_floats = need;
    }
    c.ksplit = ks;
    c.kpart = kpart_ws;
  };
  auto add_conv = [&](ConvArgs c) {
    maybe_split(c);
    split_for(c);
    if (c.h16) {  // conv-half: the image pass (prologue, one rounding), then conv_h16_kernel
      const size_t need1 = (size_t)c.B * c.Hin * c.Win * c.Cin1, need2 = (size_t)c.B * c.Hout * c.Wout * c.Cin2;
      if (c.gin_part || need1 > h16_cap1 || need2 > h16_cap2) {  // (gn_prologue keeps gin_* off a marked conv)
        h16_overflow = true;
        return;
      }
      c.h16_a1 = h16_p1;
      c.h16_a2 = c.Cin2 ? h16_p2 : nullptr;
      double fl, by;
      conv_cost(c, fl, by);
      const double npix = (double)c.B * c.Hin * c.Win;
      add("conv_h16_image", 0, 6.0 * npix * (c.Cin1 + c.Cin2), [=](hipStream_t st) {
        return conv_h16_image(c, const_cast<_Float16*>(c.h16_a1), const_cast<_Float16*>(c.h16_a2), st);
      });
      add(conv_label(c), fl, by - 2.0 * npix * (c.Cin1 + c.Cin2), [=](hipStream_t st) { return conv2d_h16(c, st); });
      return;
    }
    const ConvChoice ch = conv_choose(c);  // one decision for the launch and the label
    double fl, by;
    conv_cost(c, fl, by);
    add(conv_label(c, ch), fl, by, [=](hipStream_t st) { return conv2d_run(c, ch, st); });
  };
  auto add_gemm = [&](const GemmArgs& g) {
    double fl, by;
    gemm_cost(g, fl, by);
    add(gemm_label(g), fl, by, [=](hipStream_t st) { return gemm_batched(g, st); });
  };
  auto gn_bytes = [](const View& v, bool apply) {
    const double n = (double)v.B * v.H * v.W * v.C;
    return apply ? 8.0 * n : 4.0 * n;
  };
  Plan* P_ = &pl;
  UNetModel* self = this;

  // temb
  add("timestep_embed", 0, 4.0 * B * D, [=](hipStream_t st) {
    // [sin, cos] (modules.py:56) or ADM [cos, sin] (adm/nn.py:118)
    return timestep_embed(P_->t, B, D, self->arch.variant == 2 ? 1 : 0,
                          self->freqs_set ? self->P(self->freqs) : nullptr, e0, st);
  });
  // the time MLP and the temb projections: M = B rows, skinny. linear_rows where gemm_kernel's 64 x 64 tiles would
  // not fill one round of the CUs (the 512-wide time MLP: 9.7 vs 15 / 24 us at B = 256); the 4992-wide temb projection
  // stays on gemm_kernel (33 us vs 59 us on linear_rows). DM_LIN_ROWS=0: gemm_kernel for all three.
  auto add_rows = [&](const GemmArgs& g) {
    const long tiles64 = (long)ceil_div(kPickBatch, 64) * ceil_div(g.N, 64);
    if (!toggles().lin_rows || !linear_rows_ok(g) || tiles64 >= 256) return add_gemm(g);
    double fl, by;
    gemm_cost(g, fl, by);
    add("linear_rows_kernel", fl, by, [=](hipStream_t st) { return linear_rows(g, st); });
  };
  {
    GemmArgs g{};
    g.M = B; g.N = TD; g.K = D; g.Z1 = 1; g.Z2 = 1; g.pick_M = kPickBatch;
    g.A = e0; g.lda = D; g.Bm = P(te_w1); g.ldb = D; g.C = e1; g.ldc = TD; g.alpha = 1.f;
    g.bias = P(te_b1); g.act = 1;
    add_rows(g);
    GemmArgs g2 = g;
    g2.K = TD; g2.A = e1; g2.lda = TD; g2.Bm = P(te_w2); g2.ldb = TD; g2.C = se; g2.bias = P(te_b2);
    g2.act = 1;  // only SiLU(temb) is ever consumed (ResBlock.proj / AdaGN.proj = SiLU -> Linear)
    if (has_class) {
      // temb + class_embed(y) before the SiLU (unet_categorial_adagn.py:172-174, adm/unet.py:669-671)
      g2.act = 0;
      g2.C = e2;
      add_rows(g2);
      const float* table = P(class_embed);
      add("class_embed_silu", 0, 8.0 * B * TD, [=](hipStream_t st) {
        return embed_add_silu(e2, P_->y, table, B, TD, se, st);
      });
    } else {
      add_rows(g2);
    }
    GemmArgs g3 = g;
    g3.N = proj_total; g3.K = TD; g3.A = se; g3.lda = TD; g3.Bm = P(proj_w); g3.ldb = TD; g3.C = projs;
    g3.ldc = proj_total; g3.bias = P(proj_b); g3.act = 0;
    add_rows(g3);
  }

  // output view of node i (and of first_conv, i = -1)
  auto out_view_for = [&](int i, int C, int lvl) -> View {
    if (i >= 0 && nodes[i].skip_producer) return skip_view[nodes[i].skip_id];
    const int nx = i + 1;
    if (nx < (int)nodes.size() && nodes[nx].kind == N_RES && nodes[nx].pops_skip >= 0) return concat_x[nx];
    float* buf = alloc((size_t)B * Hl(lvl) * Wl(lvl) * C * 4);
    return View{buf, B, Hl(lvl), Wl(lvl), C, C};
  };

  // GroupNorm statistics emitted by producers (conv / GEMM epilogues): view pointer -> partials.
  // A consumer whose input view has them skips its gn_partial pass; every other write to a view
  // drops its entry.
  struct GnReady {
    double2* p;
    int C, G;  // the view's channels, the partials' group count over them
  };
  std::map<const float*, GnReady> gn_ready;
  _Float16* qkv_as = nullptr;  // pre-split qkv input (linear_presplit_a), shared by the attention blocks
  size_t qkv_as_bytes = 0;
  std::map<const float*, std::pair<double2*, int>> gn_bufs;  // view pointer -> partials buffer, its group capacity
  auto gn_buf_for = [&](const View& v, int Gv) -> double2* {
    auto it = gn_bufs.find(v.p);
    if (it != gn_bufs.end() && it->second.second >= Gv) return it->second.first;
    double2* b = (double2*)alloc((size_t)B * gn_num_chunks(v.H * v.W) * Gv * sizeof(double2));
    gn_bufs[v.p] = {b, Gv};
    return b;
  };
  // the h slice of an up-path concat [h | skip] whose GroupNorm groups straddle the slice boundary (CIFAR's
  // 384 = 256 + 128): its producer emits 4-channel units, which gn_concat_stats sums into the concat's groups
  std::set<const float*> concat_base;
  for (const View& cx : concat_x)
    if (cx.p) concat_base.insert(cx.p);
  auto emit_groups = [&](const View& v) -> int {
    if (!toggles().gn_fusion || !concat_base.count(v.p) || v.pitch == v.C || v.pitch % G != 0) return G;
    const int cpg = v.pitch / G;
    return (v.C % cpg != 0 && cpg % 4 == 0 && v.C % 4 == 0) ? v.C / 4 : G;
  };
  auto emit_conv = [&](ConvArgs& c, const View& v) {
    gn_ready.erase(v.p);
    for (const int Gv : {emit_groups(v), G}) {
      ConvArgs sk = c;
      sk.gn_part = conv_standin<double2>();
      sk.gn_G = Gv;
      maybe_split(sk);  // split-K is shape-determined; its reduction emits the statistics
      split_for(sk);    // the kernel add_conv will launch (Winograd or direct: their statistics rules differ)
      if (!conv_can_emit_gn(sk)) continue;
      c.gn_part = gn_buf_for(v, Gv);
      c.gn_G = Gv;
      gn_ready[v.p] = {c.gn_part, v.C, Gv};
      return;
    }
    c.gn_part = nullptr;
  };
  auto emit_gemm = [&](GemmArgs& g, const View& v) {
    gn_ready.erase(v.p);
    const int hw = v.H * v.W, cpg = v.C / G;
    if (gemm_pick(g) != 0 || hw % 64 != 0 || v.C % G != 0 || 32 % cpg != 0) return;
    g.gn_part = gn_buf_for(v, G);
    g.gn_G = G;
    g.gn_hw = hw;
    gn_ready[v.p] = {g.gn_part, v.C, G};
  };
  auto gn_stats = [&](const View& v) -> const double2* {
    auto it = gn_ready.find(v.p);
    if (it != gn_ready.end() && it->second.C == v.C && it->second.G == G) return it->second.p;
    add("gn_partial", 0, gn_bytes(v, false), [=](hipStream_t st) { return gn_partial(v, G, part, st); });
    return part;
  };
  // the concat input [h | skip] of an up-path ResBlock: when both slices' producers emitted their statistics
  // in groups that tile the concat's (gn_concat_ok), combine the slices' partials instead of a gn_partial pass
  auto gn_stats_concat = [&](const View& v, const View& sk) -> const double2* {
    const int Ch = v.C - sk.C;
    auto ih = gn_ready.find(v.p), is = gn_ready.find(sk.p);
    if (toggles().gn_fusion && ih != gn_ready.end() && ih->second.C == Ch && is != gn_ready.end() &&
        is->second.C == sk.C && gn_concat_ok(Ch, ih->second.G, sk.C, is->second.G, G)) {
      const double2* ph = ih->second.p;
      const double2* ps = is->second.p;
      const int Cs = sk.C, HW = v.H * v.W, Gh = ih->second.G, Gs = is->second.G;
      add("gn_concat_stats", 0, 32.0 * B * gn_num_chunks(HW) * G, [=](hipStream_t st) {
        return gn_concat_stats(ph, Ch, Gh, ps, Cs, Gs, B, HW, G, part, st);
      });
      return part;
    }
    return gn_stats(v);
  };
  // GroupNorm(G) of v feeding conv c's prologue (tables gsc / gsh): either the conv finalizes the
  // statistics itself into its LDS tables (ConvChoice::lds_tables: no gn_finalize launch) or gn_finalize runs.
  auto gn_prologue = [&](ConvArgs& c, const View& v, const double2* stp, size_t gamma, size_t beta,
                         const float* ms, const float* mb, int mp) {
    c.pro_scale = gsc;
    c.pro_shift = gsh;
    split_for(c);
    const ConvChoice ch = conv_choose(c);
    const long imgs = c.taps == 1 ? 127 / ((long)c.Hout * c.Wout) + 2 : (long)ch.geom.TB;
    // in-kernel finalize: every block re-reduces its images' chunk partials, so only for small maps
    // (CIFAR: <= 16 chunks per image); the 256^2 maps of ADM have 1024 and take the finalize launch
    if (!c.h16 && ch.lds_tables && imgs * G <= 512 && v.C == c.Cin1 && gn_num_chunks(v.H * v.W) <= 64) {
      c.gin_part = stp; c.gin_G = G; c.gin_nchunk = gn_num_chunks(v.H * v.W);
      c.gin_n = (double)v.H * v.W * (v.C / G); c.gin_eps = gn_eps;
      c.gin_gamma = P(gamma); c.gin_beta = P(beta); c.gin_ms = ms; c.gin_mb = mb; c.gin_mp = mp;
      return;
    }
    add("gn_finalize", 0, 8.0 * B * v.C, [=](hipStream_t st) {
      return gn_finalize(v, G, stp, gn_eps, self->P(gamma), self->P(beta), gsc, gsh, st, ms, mb, mp);
    });
  };

  // first conv -> skip 0
  View x_cur = skip_view[0];
  {
    View y = x_cur;
    const float* w = P(first_w);
    const float* bb = P(first_b);
    const int cin = arch.in_channels;
    // the first ResBlock's GroupNorm statistics (and the last up-path concat's skip slice: skip 0 is never
    // rewritten) from the conv's epilogue
    double2* gp = nullptr;
    if (conv3x3_small_in_can_emit(H, W, C0, G) && toggles().gn_fusion) {
      gp = gn_buf_for(y, G);
      gn_ready[y.p] = {gp, C0, G};
    }
    add("conv3x3_small_in", 2.0 * B * H * W * C0 * 9 * cin, 4.0 * B * H * W * (cin + C0),
        [=](hipStream_t st) { return conv3x3_small_in(P_->x, B, cin, H, W, w, bb, C0, y, st, gp, G); });
  }

  for (size_t i = 0; i < nodes.size(); ++i) {
    const Node& n = nodes[i];
    View xin = (n.kind == N_RES && n.pops_skip >= 0)
                   ? View{concat_x[i].p, B, concat_x[i].H, concat_x[i].W, n.cin, n.cin}
                   : x_cur;
    View y = out_view_for((int)i, n.cout, n.level_out);
    if (!y.p || alloc_failed) { set_error("workspace allocation failed"); return DM_ERR_HIP; }
    const int Hi = Hl(n.level_in), Wi = Wl(n.level_in);
    const int hw = Hi * Wi;
    const int nchunk = gn_num_chunks(hw);
    if (n.kind == N_RES) {
      const ResBlockP r = res[n.idx];
      // conv resolution: the block's output resolution (differs from the input for up/down blocks)
      const int Ho = Hl(n.level_out), Wo = Wl(n.level_out);
      const int nchunk_o = gn_num_chunks(Ho * Wo);
      View va1{a1, B, Ho, Wo, r.cin, r.cin};
      View vh{hbuf, B, Ho, Wo, r.cout, r.cout};
      View va2{a2, B, Ho, Wo, r.cout, r.cout};
      // residual / shortcut operand at conv resolution: X, or updown(X) (unet_categorial_adagn.py:52-57)
      View xres = xin;
      if (r.updown) {
        xres = View{xr, B, Ho, Wo, r.cin, r.cin};
        const bool down = r.updown == 2;
        add("resample2x", 0, 4.0 * B * ((double)Hi * Wi + (double)Ho * Wo) * r.cin,
            [=](hipStream_t st) { return resample2x(xin, xres, down, nullptr, nullptr, st); });
      }
      ConvArgs c1{};
      c1.x1_pitch = r.cin; c1.Cin1 = r.cin; c1.Hin = Ho; c1.Win = Wo;
      c1.taps = 9; c1.stride = 1; c1.upsample = 0;
      c1.w = P(r.conv1.w); c1.K = r.conv1.K;
      c1.y = hbuf; c1.y_pitch = r.cout; c1.Cout = r.cout; c1.B = B; c1.pick_B = kPickBatch; c1.Hout = Ho; c1.Wout = Wo;
      c1.bias = P(r.conv1.bias);
      if (!r.adagn) { c1.rowvec = projs + r.proj_col; c1.rowvec_pitch = proj_total; }
      if (r.updown == 1) { c1.upsample = 1; c1.Hin = Hi; c1.Win = Wi; }
      // sub-pixel form of the upsample conv (4/9 of the MFMA work) when its low-res shape tiles
      auto try_subpix = [&](ConvArgs& c, size_t w_sub) {
        if (!c.upsample || !w_sub) return;
        ConvArgs s = c;
        s.upsample = 2; s.w = P(w_sub); s.K = 4 * c.Cin1;
        split_for(s);  // the tile choice depends on the split copy (fp16x2-only tiles)
        if (conv_choose(s).takes_prologue) c = s;
      };
      ConvArgs c2{};
      c2.x1 = a2; c2.x1_pitch = r.cout; c2.Cin1 = r.cout; c2.Hin = Ho; c2.Win = Wo;
      c2.taps = 9; c2.stride = 1;
      c2.w = P(r.conv2.w); c2.K = r.conv2.K;
      c2.y = y.p; c2.y_pitch = y.pitch; c2.Cout = r.cout; c2.B = B; c2.pick_B = kPickBatch; c2.Hout = Ho; c2.Wout = Wo;
      c2.bias = P(r.conv2.bias);
      if (r.cin != r.cout) {
        c2.x2 = xres.p; c2.x2_pitch = xres.pitch; c2.Cin2 = r.cin;
      } else {
        c2.res = xres.p; c2.res_pitch = xres.pitch;
      }
      split_for(c1);
      split_for(c2);
      try_subpix(c1, r.conv1.w_sub);
      const bool fuse1 = r.updown != 2 && conv_choose(c1).takes_prologue, fuse2 = conv_choose(c2).takes_prologue;
      // AdaGN modulation gn(h) * (1 + ys) + yb, [ys | yb] from the fused projection (modules.py:114-123)
      const float* ms = r.adagn ? projs + r.proj_col : nullptr;
      const float* mb = r.adagn ? projs + r.proj_col + r.cout : nullptr;
      const int mp = r.adagn ? proj_total : 0;
      const double2* st1 = n.pops_skip >= 0 ? gn_stats_concat(xin, skip_view[n.pops_skip]) : gn_stats(xin);
      if (r.updown && !fuse1) {
        // normalise + SiLU + resample into a1, then a plain conv at the output resolution
        add("gn_finalize", 0, 8.0 * B * r.cin, [=](hipStream_t st) {
          return gn_finalize(xin, G, st1, gn_eps, self->P(r.gn1.g), self->P(r.gn1.b), gsc, gsh, st);
        });
        const bool down = r.updown == 2;
        add("resample2x", 0, 4.0 * B * ((double)Hi * Wi + (double)Ho * Wo) * r.cin,
            [=](hipStream_t st) { return resample2x(xin, va1, down, gsc, gsh, st); });
        c1.x1 = a1; c1.upsample = 0; c1.Hin = Ho; c1.Win = Wo;
        c1.w = P(r.conv1.w); c1.K = r.conv1.K;
      } else if (fuse1) {
        // GroupNorm + SiLU folded into conv1's patch load: x read once, normalised tensor never stored
        c1.x1 = xin.p; c1.x1_pitch = xin.pitch;
        gn_prologue(c1, xin, st1, r.gn1.g, r.gn1.b, nullptr, nullptr, 0);
      } else {
        add("gn_apply", 0, gn_bytes(xin, true), [=](hipStream_t st) {
          return gn_apply(xin, G, st1, nchunk, gn_eps, self->P(r.gn1.g), self->P(r.gn1.b), nullptr, nullptr, 0, 1,
                          va1, st);
        });
        c1.x1 = a1;
      }
      emit_conv(c1, vh);
      add_conv(c1);
      const double2* st2 = gn_stats(vh);
      if (fuse2) {
        c2.x1 = hbuf;
        gn_prologue(c2, vh, st2, r.gn2.g, r.gn2.b, ms, mb, mp);
      } else {
        add("gn_apply", 0, gn_bytes(vh, true), [=](hipStream_t st) {
          return gn_apply(vh, G, st2, nchunk_o, gn_eps, self->P(r.gn2.g), self->P(r.gn2.b), ms, mb, mp, 1, va2, st);
        });
      }
      emit_conv(c2, y);
      add_conv(c2);
    } else if (n.kind == N_ATTN) {
      const AttnP p = attn[n.idx];
      const int C = p.C, heads = p.heads, Dh = C / heads;
      // GroupNorm folded into the QKV projection's A load (modules.py:91-94): one pass over x
      const double2* sta = gn_stats(xin);
      // One head of 256 channels on a 16 x 16 map (the CIFAR UNet's stage-1 blocks): the folded block
      // (attn_block.hip): T, S, softmax, P xn, the folded projection Wg' and the residual in one kernel, no q / k /
      // v planes. Variant 4 (default): 8 waves of 16 queries (attn_block4_kernel); DM_ATTN=3: the 4-wave form
      // (attn_block3_kernel, bit-identical); DM_ATTN=0 / unfused / ...: the unfolded path below.
      const int av = toggles().attn;
      const FoldW* fw = nullptr;
      if (conv_math == 2 && arch.variant != 2 && (av == 3 || av == 4) && attn_block_ok(hw, C, heads) && y.p != xin.p)
        fw = fold_for(p);
      if (fw) {
        AttnBlockArgs ab{};
        ab.x = xin.p; ab.x_pitch = xin.pitch; ab.gsc = gsc; ab.gsh = gsh;
        ab.at_img = static_cast<const _Float16*>(fw->at_img); ab.at_rowscale = fw->at_rs; ab.w = fw->w;
        ab.y = y.p; ab.y_pitch = y.pitch; ab.B = B; ab.ex = 6; ab.eg = 6;
        ab.range_flag = range_flag;
        ab.variant = av;
        ab.wg_img = static_cast<const _Float16*>(fw->wgp_img); ab.wg_rowscale = fw->wgp_rs; ab.cb = fw->cb;
        // variant 4 finalizes the block's GroupNorm statistics itself (DM_ATTN_GNFIN=1: gn_finalize)
        const bool infin = av == 4 && C % G == 0 && !toggles().attn_gn_launch;
        if (infin) {
          ab.gin_part = sta; ab.gin_G = G; ab.gin_nchunk = gn_num_chunks(hw);
          ab.gin_gamma = P(p.gn.g); ab.gin_beta = P(p.gn.b); ab.gin_eps = gn_eps;
        } else {
          add("gn_finalize", 0, 8.0 * B * C, [=](hipStream_t st) {
            return gn_finalize(xin, G, sta, gn_eps, self->P(p.gn.g), self->P(p.gn.b), gsc, gsh, st);
          });
        }
        gn_ready.erase(y.p);
        const int cpg = C / G;
        if (C % G == 0 && cpg >= 4 && cpg <= 32 && (cpg & (cpg - 1)) == 0) {
          ab.gn_part = gn_buf_for(y, G);
          ab.gn_G = G;
          gn_ready[y.p] = {ab.gn_part, y.C, G};
        }
        // T (2 L C^2), S (2 L^2 C), P xn (2 L^2 C), Wg' O (2 L C^2) per image; x read, y written
        const double fl = 2.0 * B * (2.0 * hw * C * C + 2.0 * hw * hw * C);
        const double by = 4.0 * B * hw * C * 2.0;
        add(av == 4 ? "attn_block4_kernel<8>" : "attn_block3_kernel", fl, by,
            [=](hipStream_t st) { return attn_block(ab, st); });
        x_cur = y;
        continue;
      }
      // The 4 x 4 middle block (16 tokens): the same folded form on the fp32 vector ALUs, one work-group per
      // image, GroupNorm finalize and the consumer's statistics in the kernel (attn_small; DM_ATTN_SMALL=0 or an
      // oracle DM_ATTN mode: the unfolded launches below)
      if (conv_math == 2 && arch.variant != 2 && (av == 3 || av == 4) && toggles().attn_small && attn_small_ok(hw, C, heads) &&
          y.p != xin.p && C % G == 0 && (C / G) >= 4 && ((C / G) & (C / G - 1)) == 0) {
        if (const FoldW* fs = fold_for(p)) {
          AttnBlockArgs ab{};
          ab.x = xin.p; ab.x_pitch = xin.pitch; ab.y = y.p; ab.y_pitch = y.pitch; ab.B = B;
          ab.at_t = fs->at_t; ab.w = fs->w; ab.wg_t = fs->wg_t; ab.cb = fs->cb;
          ab.gin_part = sta; ab.gin_G = G; ab.gin_nchunk = gn_num_chunks(hw);
          ab.gin_gamma = P(p.gn.g); ab.gin_beta = P(p.gn.b); ab.gin_eps = gn_eps;
          ab.gn_part = gn_buf_for(y, G);
          ab.gn_G = G;
          gn_ready.erase(y.p);
          gn_ready[y.p] = {ab.gn_part, y.C, G};
          const double fl = 2.0 * B * (2.0 * hw * C * C + 2.0 * hw * hw * C);
          const double by = 4.0 * B * hw * C * 2.0;
          add("attn_small_kernel", fl, by, [=](hipStream_t st) { return attn_small(ab, st); });
          x_cur = y;
          continue;
        }
      }
      GemmArgs gq{};
      gq.M = B * hw; gq.N = 3 * C; gq.K = C; gq.Z1 = 1; gq.Z2 = 1; gq.pick_M = (long)kPickBatch * hw;
      gq.A = xin.p; gq.lda = xin.pitch; gq.Bm = P(p.wqkv); gq.ldb = C; gq.C = qkv; gq.ldc = 3 * C;
      gq.alpha = 1.f; gq.bias = P(p.bqkv);
      gq.pro_scale = gsc; gq.pro_shift = gsh; gq.pro_rows = hw;
      // fp16x2: qkv = 1x1 conv of GroupNorm(x) on the split conv kernel (MODE 3, pre-split weights)
      ConvArgs cq{};
      cq.x1 = xin.p; cq.x1_pitch = xin.pitch; cq.Cin1 = C; cq.Hin = Hi; cq.Win = Wi; cq.taps = 1; cq.stride = 1;
      cq.w = P(p.wqkv); cq.K = C; cq.y = qkv; cq.y_pitch = 3 * C; cq.Cout = 3 * C; cq.B = B; cq.pick_B = kPickBatch; cq.Hout = Hi;
      cq.Wout = Wi; cq.bias = P(p.bqkv); cq.pro_scale = gsc; cq.pro_shift = gsh; cq.pro_nosilu = 1;
      split_for(cq);
      // Fused attention (attention.hip) on 16 x 16 maps; with the qkv conv on the split kernel, its epilogue
      // writes q / k / v as the fp16x2 operand planes the fused kernel reads (over the qkv buffer: same bytes)
      // other shapes (ADM's 32^2 and 8^2 blocks): flash attention on the pre-split planes (attn_flash)
      // (DM_ATTN oracle modes, Toggles::attn: no flash kernel outside the defaults 3 / 4; "fused": no pre-split
      // planes; "unfused": S GEMM, softmax_rows, PV GEMM; "noproj": proj as its own launch)
      const bool l256 = attn_fused_ok(hw, Dh);
      const bool attn_default = av == 3 || av == 4;
      const bool flash = !l256 && attn_flash_ok(hw, Dh) && attn_default;
      bool fuse_attn = conv_math == 2 && (l256 || flash) && av != kAttnUnfused;
      const bool presplit = fuse_attn && conv_pw_ok(cq) && av != kAttnFused;
      if (flash && !presplit) fuse_attn = false;   // the flash kernel reads the planes only
      _Float16* planes = reinterpret_cast<_Float16*>(qkv);
      const size_t plane_n = (size_t)B * hw * C * 2;  // fp16 elements of one operand's two planes
      if (presplit) {
        cq.ap_q = planes; cq.ap_k = planes + plane_n; cq.ap_v = planes + 2 * plane_n;
        cq.ap_L = hw; cq.ap_heads = heads; cq.ap_Dh = Dh; cq.ap_legacy = p.legacy ? 1 : 0;
        cq.ap_alpha = p.sa; cq.ap_bscale = p.sb;
        cq.ap_ea = 6; cq.ap_eb = 6; cq.ap_ev = 6;
      }
      // the qkv projection on linear_k32 (pre-split weights = the MODE 3 conv's split copy, K = 32 MFMA steps,
      // GroupNorm tables from gn_finalize): the plane or fp32 epilogue of the same values in every attention mode
      GemmArgs gl{};
      gl.M = B * hw; gl.N = 3 * C; gl.K = C; gl.Z1 = 1; gl.Z2 = 1;
      gl.A = xin.p; gl.lda = xin.pitch; gl.Bm = P(p.wqkv); gl.ldb = C; gl.C = qkv; gl.ldc = 3 * C;
      gl.alpha = 1.f; gl.bias = P(p.bqkv);
      gl.pro_scale = gsc; gl.pro_shift = gsh; gl.pro_rows = hw;
      gl.split = 2; gl.split_ea = 0; gl.range_flag = range_flag;
      gl.ws = cq.ws; gl.ws_rowscale = cq.ws_rowscale;
      if (presplit) {
        gl.ap_q = cq.ap_q; gl.ap_k = cq.ap_k; gl.ap_v = cq.ap_v;
        gl.ap_L = cq.ap_L; gl.ap_heads = cq.ap_heads; gl.ap_Dh = cq.ap_Dh; gl.ap_legacy = cq.ap_legacy;
        gl.ap_alpha = cq.ap_alpha; gl.ap_bscale = cq.ap_bscale;
        gl.ap_ea = cq.ap_ea; gl.ap_eb = cq.ap_eb; gl.ap_ev = cq.ap_ev;
      }
      const bool qkv_linear = conv_math == 2 && cq.ws && cq.ws_np == 2 && linear_k32_ok(gl);
      if (qkv_linear) {
        add("gn_finalize", 0, 8.0 * B * C, [=](hipStream_t st) {
          return gn_finalize(xin, G, sta, gn_eps, self->P(p.gn.g), self->P(p.gn.b), gsc, gsh, st);
        });
        // GroupNorm + split of the input once (linear_presplit_a) instead of once per 128-column tile inside
        // the GEMM: one buffer shared by the attention blocks (the plan's launches are stream-ordered)
        const size_t need = (size_t)gl.M * gl.K * 4;
        if (need > qkv_as_bytes) {
          qkv_as = reinterpret_cast<_Float16*>(alloc(need));
          qkv_as_bytes = need;
        }
        _Float16* asb = qkv_as;
        add("linear_presplit_a", 0, 8.0 * gl.M * gl.K, [=](hipStream_t st) { return linear_presplit_a(gl, asb, st); });
        GemmArgs g2 = gl;
        g2.as = asb;
        g2.pro_scale = g2.pro_shift = nullptr;
        add_gemm(g2);
      } else if (conv_pw_ok(cq)) {
        gn_prologue(cq, xin, sta, p.gn.g, p.gn.b, nullptr, nullptr, 0);
        add_conv(cq);
      } else {
        add("gn_finalize", 0, 8.0 * B * C, [=](hipStream_t st) {
          return gn_finalize(xin, G, sta, gn_eps, self->P(p.gn.g), self->P(p.gn.b), gsc, gsh, st);
        });
        split_gemm(gq, 6, gq.Bm, (size_t)3 * C * C);
        add_gemm(gq);
      }
      // head h of q / k / v: columns q0 + h * hs, k0 + h * hs, v0 + h * hs of the qkv rows
      // (q | k | v blocks: modules.py:92-94 and ADM QKVAttention; per-head [q; k; v]: QKVAttentionLegacy)
      const int hs = p.legacy ? 3 * Dh : Dh;
      const int k0 = p.legacy ? Dh : C, v0 = p.legacy ? 2 * Dh : 2 * C;
      // proj (1x1 conv, + bias + residual x): built here so that the fused kernel can apply it
      GemmArgs gp{};
      gp.M = B * hw; gp.N = C; gp.K = C; gp.Z1 = 1; gp.Z2 = 1; gp.pick_M = (long)kPickBatch * hw;
      gp.A = Ob; gp.lda = C; gp.Bm = P(p.wproj); gp.ldb = C; gp.C = y.p; gp.ldc = y.pitch;
      gp.alpha = 1.f; gp.bias = P(p.bproj); gp.res = xin.p; gp.ld_res = xin.pitch;
      ConvArgs cp{};
      cp.x1 = Ob; cp.x1_pitch = C; cp.Cin1 = C; cp.Hin = Hi; cp.Win = Wi; cp.taps = 1; cp.stride = 1;
      cp.w = P(p.wproj); cp.K = C; cp.y = y.p; cp.y_pitch = y.pitch; cp.Cout = C; cp.B = B; cp.pick_B = kPickBatch; cp.Hout = Hi;
      cp.Wout = Wi; cp.bias = P(p.bproj); cp.res = xin.p; cp.res_pitch = xin.pitch;
      split_for(cp);
      const bool proj_conv = conv_pw_ok(cp);
      if (proj_conv) emit_conv(cp, y);
      // one head of 256 channels (the CIFAR UNet's 16 x 16 attention): proj runs inside the fused kernel on
      // its O rows (O never goes to HBM), same MFMA sequence and epilogue as the MODE 3 launch
      const bool fuse_proj = presplit && proj_conv && heads == 1 && Dh == 256 && av != kAttnNoProj;
      if (fuse_attn) {
        // S, softmax and PV in one kernel (attention.hip), bit-identical to the three launches below
        AttnArgs at{};
        if (fuse_proj) {
          at.fuse_proj = 1;
          at.proj = cp;
        }
        if (presplit) {
          at.pq = planes; at.pk = planes + plane_n; at.pv = planes + 2 * plane_n;
        }
        at.qkv = qkv; at.ld = 3 * C; at.L = hw; at.Dh = Dh; at.heads = heads; at.B = B;
        at.q0 = 0; at.k0 = k0; at.v0 = v0; at.hs = hs;
        at.alpha = p.sa; at.b_scale = p.sb;
        at.out = Ob; at.ldo = C;
        at.ea = 6; at.eb = 6; at.ep = 14; at.ev = 6;
        at.range_flag = range_flag;
        double fl = 4.0 * B * heads * (double)hw * hw * Dh;
        double by = 4.0 * B * hw * (3.0 * C + C);
        if (fuse_proj) {  // + the proj GEMM; reads x (residual) and the weights, writes y instead of O
          fl += 2.0 * B * hw * (double)C * C;
          by += 4.0 * B * hw * C + 4.0 * C * C;
        }
        add((flash ? "attn_flash_kernel<" : presplit ? "attn_presplit_kernel<" : "attn_fused_kernel<") + std::to_string(Dh) +
                (fuse_proj ? ",proj>" : ">"),
            fl, by, [=](hipStream_t st) { return attn_fused(at, st); });
      } else {
      GemmArgs gs{};
      gs.M = hw; gs.N = hw; gs.K = Dh; gs.Z1 = B; gs.Z2 = heads; gs.pick_Z = (long)kPickBatch * heads;
      gs.A = qkv; gs.a_s1 = (long)hw * 3 * C; gs.a_s2 = hs; gs.lda = 3 * C;
      gs.Bm = qkv + k0; gs.b_s1 = (long)hw * 3 * C; gs.b_s2 = hs; gs.ldb = 3 * C;
      gs.C = Sb; gs.c_s1 = (long)heads * hw * hw; gs.c_s2 = (long)hw * hw; gs.ldc = hw;
      gs.alpha = p.sa;
      gs.b_scale = p.sb;
      split_gemm(gs, 6, nullptr, 0, 6);
      add_gemm(gs);
      const long rows = (long)B * heads * hw;
      add("softmax_rows", 0, 8.0 * rows * hw, [=](hipStream_t st) { return softmax_rows(Sb, rows, hw, hw, st); });
      GemmArgs go{};
      go.M = hw; go.N = Dh; go.K = hw; go.Z1 = B; go.Z2 = heads; go.pick_Z = (long)kPickBatch * heads;
      go.A = Sb; go.a_s1 = (long)heads * hw * hw; go.a_s2 = (long)hw * hw; go.lda = hw;
      go.Bm = qkv + v0; go.b_s1 = (long)hw * 3 * C; go.b_s2 = hs; go.ldb = 3 * C; go.b_kn = 1;
      go.C = Ob; go.c_s1 = (long)hw * C; go.c_s2 = Dh; go.ldc = C;
      go.alpha = 1.f;
      split_gemm(go, 14, nullptr, 0, 6);
      add_gemm(go);
      }
      if (fuse_proj) {
      } else if (proj_conv) {
        add_conv(cp);
      } else {
        split_gemm(gp, 6, gp.Bm, (size_t)C * C);
        emit_gemm(gp, y);
        add_gemm(gp);
      }
    } else if (n.idx < 0) {
      // resampling without a conv (adm/unet.py:126-128 nearest-2x, :153-155 avg-pool)
      const bool down = n.kind == N_DOWN;
      gn_ready.erase(y.p);
      add("resample2x", 0, 4.0 * B * ((double)Hi * Wi + (double)y.H * y.W) * n.cin,
          [=](hipStream_t st) { return resample2x(xin, y, down, nullptr, nullptr, st); });
    } else {
      const ConvP cv = convs[n.idx];
      ConvArgs c{};
      c.x1 = xin.p; c.x1_pitch = xin.pitch; c.Cin1 = n.cin; c.Hin = Hi; c.Win = Wi;
      c.taps = 9; c.stride = n.kind == N_DOWN ? 2 : 1; c.upsample = n.kind == N_UP;
      // variant 3's Downsample pads (0, 1, 0, 1) and convolves with padding 0 (pesser/model.py:66-70): taps from 2o
      if (n.kind == N_DOWN && arch.variant == 3) c.s2_pad0 = 1;
      c.w = P(cv.w); c.K = cv.K;
      c.y = y.p; c.y_pitch = y.pitch; c.Cout = n.cout; c.B = B; c.pick_B = kPickBatch;
      c.Hout = Hl(n.level_out); c.Wout = Wl(n.level_out);
      c.bias = P(cv.bias);
      if (c.upsample && cv.w_sub) {
        ConvArgs s = c;
        s.upsample = 2; s.w = P(cv.w_sub); s.K = 4 * c.Cin1;
        split_for(s);
        if (conv_choose(s).takes_prologue) c = s;
        // whole-row low-res maps of 4 / 8 / 16 columns: the sub-pixel Winograd kernel (3/4 of the MFMA products)
        if (c.upsample == 2 && cv.has_subw) subwino_for(c, P(cv.w_subw));
      }
      if (c.upsample == 2) {
        emit_conv(c, y);  // the K32 sub-pixel conv's epilogue emits the consumer's GroupNorm partials
      } else if (c.stride == 2) {
        // the K32 stride-2 tiles emit them too. Only those take the split weights here: attached earlier to a
        // 4x4-output downsample they made maybe_split() put it on conv_patch3 MODE 4 with split-K, a path the
        // plan never takes otherwise (reference-fixture forwards off by 0.14)
        ConvArgs s = c;
        split_for(s);
        const K32Form v = conv_choose(s).k32;
        if (v == K32Form::S2 || (c.s2_pad0 && v == K32Form::S2Seg)) {  // (the row-segment form: bottom/right-padded only)
          c = s;
          emit_conv(c, y);
        } else {
          gn_ready.erase(y.p);
        }
      } else {
        gn_ready.erase(y.p);
      }
      add_conv(c);
    }
    x_cur = y;
  }
  // last conv: GN -> SiLU -> conv(cur -> out_channels), NCHW output
  {
    const int C = x_cur.C;
    View xin = x_cur;
    View va{a1, B, H, W, C, C};
    const int nchunk = gn_num_chunks(H * W);
    const GnP lg = last_gn;
    const float* lw = P(last_w);
    const float* lb = P(last_b);
    const int oc = arch.out_channels;
    const double2* stl = gn_stats(xin);
    // the GroupNorm affine finalized in the last conv's blocks (one image each) from the partials, the serial chunk
    // sums of gn_finalize_kernel (maps of <= 64 chunks: 64^2 and below); DM_GN_FUSION=0, wider maps or more than 512
    // channels: the gn_finalize launch
    GnFin fin;
    if (toggles().gn_fusion && C <= 512 && C % G == 0 && nchunk <= 64) {
      fin.part = stl; fin.G = G; fin.nchunk = nchunk; fin.n = (double)H * W * (C / G); fin.eps = gn_eps;
      fin.gamma = P(lg.g); fin.beta = P(lg.b);
    } else {
      add("gn_finalize", 0, 8.0 * B * C, [=](hipStream_t st) {
        return gn_finalize(xin, G, stl, gn_eps, self->P(lg.g), self->P(lg.b), gsc, gsh, st);
      });
    }
    (void)va;
    if (!last_packed) {  // packed [9][C][CO] copy of the last conv weight (model-owned, built once)
      DM_CHECK_HIP(hipMalloc(&last_packed, (size_t)9 * C * 8 * sizeof(float)));
      DM_REQUIRE(small_out_pack(lw, oc, C, last_packed, nullptr) == DM_OK, "last conv: weight packing failed");
      DM_CHECK_HIP(hipDeviceSynchronize());
    }
    lw = last_packed;
    add("conv3x3_small_out", 2.0 * B * H * W * oc * 9 * C, 4.0 * B * H * W * (C + oc),
        [=](hipStream_t st) {
          return fin.part ? conv3x3_small_out(xin, lw, lb, oc, P_->out, st, nullptr, nullptr, fin)
                          : conv3x3_small_out(xin, lw, lb, oc, P_->out, st, gsc, gsh);
        });
  }
  DM_REQUIRE(!h16_overflow, "conv-half plan: a covered conv with in-kernel GroupNorm tables, or beyond the image planes");
  return DM_OK;
}

}  // namespace dm

// ===========================================================================
// C ABI
// ===========================================================================
struct dm_unet {
  dm::UNetModel* m;
};

extern "C" int dm_unet_param_count(const dm_unet_arch* arch, int* n_params) {
  int rc = dm::validate_arch(arch);
  if (rc) return rc;
  if (!n_params) { dm::set_error("n_params is null"); return DM_ERR_ARG; }
  *n_params = dm::count_params(*arch);
  return DM_OK;
}

/* Test hook (tests/test_pesser_host.py; host only): the state_dict index of every tensor in the order the executor
 * consumes them. Variant 3: dm::walk_order(); the other variants read the state_dict as it is registered. */
extern "C" int dm_debug_unet_param_order(const dm_unet_arch* arch, int* order, int n) {
  int rc = dm::validate_arch(arch);
  if (rc) return rc;
  if (!order || n != dm::count_params(*arch)) { dm::set_error("order: one slot per parameter tensor"); return DM_ERR_ARG; }
  if (arch->variant == 3) {
    const std::vector<int> w = dm::walk_order(*arch);
    if ((int)w.size() != n) { dm::set_error("variant 3: parameter order table does not cover the state_dict"); return DM_ERR_STATE; }
    for (int i = 0; i < n; ++i) order[i] = w[i];
  } else {
    for (int i = 0; i < n; ++i) order[i] = i;
  }
  return DM_OK;
}

extern "C" int dm_unet_create(const dm_unet_arch* arch, const float* const* params, const int64_t* numels,
                              int n_params, void* stream, dm_unet** out) {
  if (!out || !params || !numels) { dm::set_error("null argument"); return DM_ERR_ARG; }
  dm::UNetModel* m = nullptr;
  int rc = dm::unet_create(arch, params, numels, n_params, (hipStream_t)stream, &m);
  if (rc) return rc;
  *out = new dm_unet{m};
  return DM_OK;
}

extern "C" int dm_unet_forward(dm_unet* h, const float* x, const int64_t* t, const int64_t* y, int B, int H, int W,
                               float* out, void* stream) {
  dm::UNetModel* m = dm::model_of(h);
  DM_ABI_MODEL(m);
  if (!x || !t || !out) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  if (B <= 0 || H <= 0 || W <= 0) { dm::set_error("empty batch or image"); return DM_ERR_ARG; }
  if (static_cast<const void*>(out) == static_cast<const void*>(x)) {
    dm::set_error("out must not alias x");
    return DM_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t nx = (size_t)B * m->arch.in_channels * H * W, no = (size_t)B * m->arch.out_channels * H * W;
  using Plan = dm::UNetModel::Plan;
  return dm::run_forward(
      *m, st, [&](int math, Plan** pl) { return m->get_plan(B, H, W, math, pl); },
      [&](Plan& pl) {
        DM_CHECK_HIP(hipMemcpyAsync(pl.x, x, nx * sizeof(float), hipMemcpyDeviceToDevice, st));
        DM_CHECK_HIP(hipMemcpyAsync(pl.t, t, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        // the labels are read only by the class embedding (class_embed_silu); without one the staging is skipped
        if (m->has_class) {
          if (y)
            DM_CHECK_HIP(hipMemcpyAsync(pl.y, y, (size_t)B * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
          else
            DM_CHECK_HIP(hipMemsetAsync(pl.y, 0xff, (size_t)B * sizeof(int64_t), st));  // -1: no label
        }
        return DM_OK;
      },
      [&](Plan& pl) {
        DM_CHECK_HIP(hipMemcpyAsync(out, pl.out, no * sizeof(float), hipMemcpyDeviceToDevice, st));
        return DM_OK;
      });
}

extern "C" int dm_unet_set_range_deferred(dm_unet* h, int deferred) {
  return dm::abi_set_range_deferred(dm::model_of(h), deferred);
}
extern "C" int dm_unet_range_poll(dm_unet* h, void* stream, int* flagged) {
  return dm::abi_range_poll(dm::model_of(h), (hipStream_t)stream, flagged);
}
extern "C" int dm_unet_range_fallback(dm_unet* h, int on) { return dm::abi_range_fallback(dm::model_of(h), on); }
extern "C" int dm_unet_range_stats(const dm_unet* h, int64_t* fallbacks, int* active) {
  return dm::abi_range_stats(dm::model_of(h), fallbacks, active);
}
extern "C" int dm_unet_memory(const dm_unet* h, int64_t* weight_bytes, int64_t* workspace_bytes) {
  return dm::abi_memory(dm::model_of(h), weight_bytes, workspace_bytes);
}

extern "C" int dm_unet_share_workspace(dm_unet* a, dm_unet* b) {
  if (!a || !a->m || !b || !b->m) { dm::set_error("null model"); return DM_ERR_STATE; }
  if (a->m->plans.pool != b->m->plans.pool) b->m->plans.share(a->m->plans.pool);
  return DM_OK;
}

extern "C" int dm_unet_plan_stats(const dm_unet* h, int64_t* builds, int* cached) {
  return dm::abi_plan_stats(dm::model_of(h), builds, cached);
}
extern "C" int dm_unet_set_conv_math(dm_unet* h, int kind) { return dm::abi_set_math(dm::model_of(h), kind, true); }
extern "C" int dm_unet_get_conv_math(const dm_unet* h, int* kind) { return dm::abi_get_math(dm::model_of(h), kind); }

extern "C" int dm_unet_set_conv_half(dm_unet* h, int on) {
  auto* m = dm::model_of(h);
  DM_ABI_MODEL(m);
  if (on != 0 && on != 1) { dm::set_error("conv_half must be 0 or 1"); return DM_ERR_ARG; }
  if ((on != 0) != m->conv_half) {
    m->conv_half = on != 0;
    m->plans.clear();
  }
  return DM_OK;
}
extern "C" int dm_unet_get_conv_half(const dm_unet* h, int* on) {
  auto* m = dm::model_of(h);
  DM_ABI_MODEL(m && on);
  *on = m->conv_half ? 1 : 0;
  return DM_OK;
}
extern "C" int dm_unet_set_time_freqs(dm_unet* h, const float* freqs, int n, void* stream) {
  return dm::abi_set_time_freqs(dm::model_of(h), freqs, n, (hipStream_t)stream);
}
extern "C" int dm_unet_profile(dm_unet* h, int enable) { return dm::abi_profile(dm::model_of(h), enable); }
extern "C" int dm_unet_profile_count(dm_unet* h, int* n_ops) { return dm::abi_profile_count(dm::model_of(h), n_ops); }
extern "C" int dm_unet_profile_get(dm_unet* h, int i, char* label, int label_len, double* flops, double* bytes,
                                   double* ms_total, int64_t* launches) {
  return dm::abi_profile_get(dm::model_of(h), i, label, label_len, flops, bytes, ms_total, launches);
}
extern "C" void dm_unet_destroy(dm_unet* h) { dm::abi_destroy(h); }
