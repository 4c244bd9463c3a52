// Building blocks shared by the KL autoencoder's two executors (vae_exec.hip: the decoder, vae_enc_exec.hip: the
// encoder; reference models/stablediffusion/autoencoder.py): the packed weights of a ResnetBlock (:69-130) and of
// the single-head AttnBlock (:133-182), and the plan builders of the two blocks over an ExecNet (exec_core.h: the
// weight arena, split weights, the fp16 range flag) -- GroupNorm statistics emitted by the producer conv and
// consumed in the next conv's prologue, the unfused middle attention.
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "dm_common.h"
#include "dm_kernels.h"
#include "plan.h"
#include "exec_pack.h"
#include "exec_core.h"

namespace dm {
namespace vaeb {

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

// Create time: the blocks' state_dict tensors in registration order -> pack jobs into the weight arena
struct BlockReader {
  ParamReader& rd;
  Packer& pk;
  GnW gn(int C, const char* what) {
    GnW g;
    g.g = pk.raw(rd.take(C, what), C);
    g.b = pk.raw(rd.take(C, what), C);
    return g;
  }
  // a 3x3 conv as [Cout][9 Cin]
  ConvW conv3x3(int cin, int cout, const char* wname, const char* bname) {
    ConvW c;
    const float* w = rd.take((int64_t)cout * cin * 9, wname);
    const float* b = rd.take(cout, bname);
    c.Cout = cout; c.Cin = cin; c.K = 9 * cin;
    c.w = pk.reserve((int64_t)cout * 9 * cin);
    pk.conv_at(w, cout, cin, 9, 9 * cin, 0, c.w);
    c.bias = pk.raw(b, cout);
    return c;
  }
  ResW resblock(int cin, int cout) {
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
  }
  AttnW attn(int C) {
    AttnW p;
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
    return p;
  }
};

// Plan-build time: the activation buffers of one plan and the builders of the two blocks over them. Lives for one
// build_plan call; every launch closure copies what it reads (no closure keeps a pointer to the planner).
struct BlockPlanner {
  ExecNet* net;
  PlanBase& pl;
  int B, G;
  float eps;
  float* bufs[3] = {nullptr, nullptr, nullptr};
  float* hbuf = nullptr;   // conv1 output of a ResnetBlock
  float* abuf = nullptr;   // GroupNorm + SiLU output where a conv has no fused prologue
  double2* part = nullptr;
  double2* emit_parts[2] = {nullptr, nullptr};  // producer-emitted statistics alternate between two buffers
  float *gsc = nullptr, *gsh = nullptr;
  // attention scratch: qkv rows, O rows, and the scores of `sb` images at a time (bounded score scratch)
  float *qkv = nullptr, *Ob = nullptr, *Sb = nullptr;
  int sb = 1;
  // GroupNorm statistics a producer's epilogue emitted for a view (pointer -> partials)
  struct Ready { const double2* p; int C; };
  std::map<const float*, Ready> gn_ready;
  int emit_next = 0;
  int cur_buf = 0;

  BlockPlanner(ExecNet* n, PlanBase& p, int B_, int G_, float eps_) : net(n), pl(p), B(B_), G(G_), eps(eps_) {}

  // three rotating activation buffers + hbuf + abuf of max_t floats per image, the statistics and table buffers, and
  // the attention scratch for hw0 tokens of Ca channels
  void alloc(size_t max_t, int max_chunks, int max_c, int hw0, int Ca) {
    for (auto& b : bufs) b = pl.alloc((size_t)B * max_t * 4);
    hbuf = pl.alloc((size_t)B * max_t * 4);
    abuf = pl.alloc((size_t)B * max_t * 4);
    part = (double2*)pl.alloc((size_t)B * max_chunks * G * sizeof(double2));
    for (auto& e : emit_parts) e = (double2*)pl.alloc((size_t)B * max_chunks * G * sizeof(double2));
    gsc = pl.alloc((size_t)B * max_c * 4);
    gsh = pl.alloc((size_t)B * max_c * 4);
    const size_t kScoreBudget = (size_t)256 << 20;
    sb = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, kScoreBudget / ((size_t)hw0 * hw0 * 4)));
    qkv = pl.alloc((size_t)B * hw0 * 3 * Ca * 4);
    Ob = pl.alloc((size_t)B * hw0 * Ca * 4);
    Sb = pl.alloc((size_t)sb * hw0 * hw0 * 4);
  }

  void add(std::string label, double flops, double bytes, std::function<int(hipStream_t)> fn) {
    pl.add(std::move(label), flops, bytes, std::move(fn));
  }
  static void conv_cost(const ConvArgs& c, double& fl, double& by) {
    const double M = (double)c.B * c.Hout * c.Wout;
    fl = 2.0 * M * c.Cout * c.K;
    by = 4.0 * ((double)c.B * c.Hin * c.Win * c.Cin1 + M * c.Cin2 + (double)c.Cout * c.K + M * c.Cout +
                (c.res ? M * c.Cout : 0.0));
  }
  static void gemm_cost(const GemmArgs& g, double& fl, double& by) {
    const double Z = (double)g.Z1 * g.Z2;
    fl = 2.0 * Z * g.M * g.N * g.K;
    by = 4.0 * Z * ((double)g.M * g.K + (double)g.N * g.K + (double)g.M * g.N) + (g.res ? 4.0 * g.M * g.N : 0.0);
  }
  void add_conv(ConvArgs c) {
    net->split_for(c);
    const ConvChoice ch = conv_choose(c);  // one decision for the launch and the label
    double fl, by;
    conv_cost(c, fl, by);
    add(conv_label(c, ch), fl, by, [c, ch](hipStream_t st) { return conv2d_run(c, ch, st); });
  }
  void add_gemm(const GemmArgs& g) {
    double fl, by;
    gemm_cost(g, fl, by);
    add(gemm_label(g), fl, by, [g](hipStream_t st) { return gemm_batched(g, st); });
  }

  // have conv c emit the GroupNorm statistics of its output view v where its kernel can
  void emit_conv(ConvArgs& c, const View& v) {
    gn_ready.erase(v.p);
    c.gn_part = nullptr;
    c.gn_G = 0;
    if (!toggles().gn_fusion) return;
    ConvArgs sk = c;
    sk.gn_part = conv_standin<double2>();
    sk.gn_G = G;
    net->split_for(sk);
    if (!conv_can_emit_gn(sk)) return;
    c.gn_part = emit_parts[emit_next];
    emit_next ^= 1;
    c.gn_G = G;
    // the buffer's previous owner (two producers ago) has been consumed; drop a stale entry that points at it
    for (auto it = gn_ready.begin(); it != gn_ready.end();)
      it = it->second.p == c.gn_part ? gn_ready.erase(it) : std::next(it);
    gn_ready[v.p] = {c.gn_part, v.C};
  }
  const double2* gn_stats(const View& v) {
    auto it = gn_ready.find(v.p);
    if (it != gn_ready.end() && it->second.C == v.C) return it->second.p;
    const int G_ = G;
    double2* part_ = part;
    add("gn_partial", 0, 4.0 * v.B * v.H * v.W * v.C, [=](hipStream_t st) { return gn_partial(v, G_, part_, st); });
    return part;
  }
  // GroupNorm(G) + SiLU of v as conv c's prologue: in-kernel finalize where the conv keeps its tables in LDS and the
  // map is small, else a gn_finalize launch (as the UNet plan's gn_prologue, at this network's eps)
  void gn_prologue(ConvArgs& c, const View& v, const double2* stp, const GnW& gw) {
    c.pro_scale = gsc;
    c.pro_shift = gsh;
    net->split_for(c);
    const ConvChoice ch = conv_choose(c);
    const long imgs = c.taps == 1 ? 127 / ((long)c.Hout * c.Wout) + 2 : (long)ch.geom.TB;
    const float* gamma = net->P(gw.g);
    const float* beta = net->P(gw.b);
    if (ch.lds_tables && imgs * G <= 512 && v.C == c.Cin1 && gn_num_chunks(v.H * v.W) <= 64) {
      c.gin_part = stp; c.gin_G = G; c.gin_nchunk = gn_num_chunks(v.H * v.W);
      c.gin_n = (double)v.H * v.W * (v.C / G); c.gin_eps = eps;
      c.gin_gamma = gamma; c.gin_beta = beta; c.gin_ms = nullptr; c.gin_mb = nullptr; c.gin_mp = 0;
      return;
    }
    const int G_ = G;
    const float eps_ = eps;
    float *gsc_ = gsc, *gsh_ = gsh;
    add("gn_finalize", 0, 8.0 * B * v.C,
        [=](hipStream_t st) { return gn_finalize(v, G_, stp, eps_, gamma, beta, gsc_, gsh_, st); });
  }

  float* next_buf() {
    cur_buf = (cur_buf + 1) % 3;
    return bufs[cur_buf];
  }

  // ResnetBlock (autoencoder.py:69-130, temb_channels = 0): norm1 -> SiLU -> conv1 -> norm2 -> SiLU -> conv2, plus x
  // or nin_shortcut(x) (the second K segment of conv2)
  View resblock(const ResW& r, const View& xin) {
    const int Ho = xin.H, Wo = xin.W;
    View y{next_buf(), B, Ho, Wo, r.cout, r.cout};
    View va{abuf, B, Ho, Wo, r.cin, r.cin};
    View vh{hbuf, B, Ho, Wo, r.cout, r.cout};
    View va2{abuf, B, Ho, Wo, r.cout, r.cout};
    const int nchunk = gn_num_chunks(Ho * Wo);
    ConvArgs c1{};
    c1.x1 = xin.p; c1.x1_pitch = xin.pitch; c1.Cin1 = r.cin; c1.Hin = Ho; c1.Win = Wo;
    c1.taps = 9; c1.stride = 1;
    c1.w = net->P(r.conv1.w); c1.K = r.conv1.K;
    c1.y = hbuf; c1.y_pitch = r.cout; c1.Cout = r.cout; c1.B = B; c1.pick_B = kPickBatch; c1.Hout = Ho; c1.Wout = Wo;
    c1.bias = net->P(r.conv1.bias);
    ConvArgs c2{};
    c2.x1 = hbuf; c2.x1_pitch = r.cout; c2.Cin1 = r.cout; c2.Hin = Ho; c2.Win = Wo;
    c2.taps = 9; c2.stride = 1;
    c2.w = net->P(r.conv2.w); c2.K = r.conv2.K;
    c2.y = y.p; c2.y_pitch = y.pitch; c2.Cout = r.cout; c2.B = B; c2.pick_B = kPickBatch; c2.Hout = Ho; c2.Wout = Wo;
    c2.bias = net->P(r.conv2.bias);
    if (r.cin != r.cout) {
      c2.x2 = xin.p; c2.x2_pitch = xin.pitch; c2.Cin2 = r.cin;
    } else {
      c2.res = xin.p; c2.res_pitch = xin.pitch;
    }
    net->split_for(c1);
    net->split_for(c2);
    const bool fuse1 = conv_choose(c1).takes_prologue, fuse2 = conv_choose(c2).takes_prologue;
    const double2* st1 = gn_stats(xin);
    const GnW g1 = r.gn1, g2 = r.gn2;
    const int G_ = G;
    const float eps_ = eps;
    if (fuse1) {
      gn_prologue(c1, xin, st1, g1);
    } else {
      const float *ga = net->P(g1.g), *be = net->P(g1.b);
      add("gn_apply", 0, 8.0 * B * Ho * Wo * r.cin, [=](hipStream_t st) {
        return gn_apply(xin, G_, st1, nchunk, eps_, ga, be, nullptr, nullptr, 0, 1, va, st);
      });
      c1.x1 = abuf; c1.x1_pitch = r.cin;
    }
    emit_conv(c1, vh);
    add_conv(c1);
    const double2* st2 = gn_stats(vh);
    if (fuse2) {
      gn_prologue(c2, vh, st2, g2);
    } else {
      const float *ga = net->P(g2.g), *be = net->P(g2.b);
      add("gn_apply", 0, 8.0 * B * Ho * Wo * r.cout, [=](hipStream_t st) {
        return gn_apply(vh, G_, st2, nchunk, eps_, ga, be, nullptr, nullptr, 0, 1, va2, st);
      });
      c2.x1 = abuf;
    }
    emit_conv(c2, y);
    add_conv(c2);
    return y;
  }

  // AttnBlock (autoencoder.py:158-182): one head of C channels over L = H W tokens, scores scaled by C^-1/2.
  // Unfused: qkv (GroupNorm folded into its A load), per image S = (s q) k^T, softmax rows, O = P v, then proj_out
  // + residual. attn_flash / attn_fused stop at head dims 80 / L = 256 and do not take this shape.
  View attn_block(const AttnW& p, const View& xin) {
    const int H = xin.H, W = xin.W;
    const int C = p.C, hw = H * W;
    View y{next_buf(), B, H, W, C, C};
    const double2* sta = gn_stats(xin);
    const float sa = (float)std::pow((double)C, -0.5);
    const int G_ = G;
    const float eps_ = eps;
    float *gsc_ = gsc, *gsh_ = gsh;
    ConvArgs cq{};
    cq.x1 = xin.p; cq.x1_pitch = xin.pitch; cq.Cin1 = C; cq.Hin = H; cq.Win = W; cq.taps = 1; cq.stride = 1;
    cq.w = net->P(p.wqkv); cq.K = C; cq.y = qkv; cq.y_pitch = 3 * C; cq.Cout = 3 * C; cq.B = B; cq.pick_B = kPickBatch;
    cq.Hout = H; cq.Wout = W; cq.bias = net->P(p.bqkv); cq.pro_scale = gsc; cq.pro_shift = gsh; cq.pro_nosilu = 1;
    net->split_for(cq);
    if (conv_pw_ok(cq)) {
      gn_prologue(cq, xin, sta, p.gn);
      add_conv(cq);
    } else {
      const float *ga = net->P(p.gn.g), *be = net->P(p.gn.b);
      add("gn_finalize", 0, 8.0 * B * C,
          [=](hipStream_t st) { return gn_finalize(xin, G_, sta, eps_, ga, be, gsc_, gsh_, st); });
      GemmArgs gq{};
      gq.M = B * hw; gq.N = 3 * C; gq.K = C; gq.Z1 = 1; gq.Z2 = 1; gq.pick_M = (long)kPickBatch * hw;
      gq.A = xin.p; gq.lda = xin.pitch; gq.Bm = net->P(p.wqkv); gq.ldb = C; gq.C = qkv; gq.ldc = 3 * C;
      gq.alpha = 1.f; gq.bias = net->P(p.bqkv);
      gq.pro_scale = gsc; gq.pro_shift = gsh; gq.pro_rows = hw;
      net->split_gemm(gq, 6, gq.Bm, (size_t)3 * C * C, 0);
      add_gemm(gq);
    }
    for (int b0 = 0; b0 < B; b0 += sb) {
      const int nb = std::min(sb, B - b0);
      const float* q0 = qkv + (size_t)b0 * hw * 3 * C;
      float* Sb_ = Sb;
      GemmArgs gs{};
      gs.M = hw; gs.N = hw; gs.K = C; gs.Z1 = nb; gs.Z2 = 1; gs.pick_Z = kPickBatch;
      gs.A = q0; gs.a_s1 = (long)hw * 3 * C; gs.lda = 3 * C;
      gs.Bm = q0 + C; gs.b_s1 = (long)hw * 3 * C; gs.ldb = 3 * C;
      gs.C = Sb; gs.c_s1 = (long)hw * hw; gs.ldc = hw;
      gs.alpha = sa;
      net->split_gemm(gs, 6, nullptr, 0, 6);
      add_gemm(gs);
      const long rows = (long)nb * hw;
      add("softmax_rows", 0, 8.0 * rows * hw, [=](hipStream_t st) { return softmax_rows(Sb_, rows, hw, hw, st); });
      GemmArgs go{};
      go.M = hw; go.N = C; go.K = hw; go.Z1 = nb; go.Z2 = 1; go.pick_Z = kPickBatch;
      go.A = Sb; go.a_s1 = (long)hw * hw; go.lda = hw;
      go.Bm = q0 + 2 * C; go.b_s1 = (long)hw * 3 * C; go.ldb = 3 * C; go.b_kn = 1;
      go.C = Ob + (size_t)b0 * hw * C; go.c_s1 = (long)hw * C; go.ldc = C;
      go.alpha = 1.f;
      net->split_gemm(go, 14, nullptr, 0, 6);
      add_gemm(go);
    }
    ConvArgs cp{};
    cp.x1 = Ob; cp.x1_pitch = C; cp.Cin1 = C; cp.Hin = H; cp.Win = W; cp.taps = 1; cp.stride = 1;
    cp.w = net->P(p.wproj); cp.K = C; cp.y = y.p; cp.y_pitch = y.pitch; cp.Cout = C; cp.B = B; cp.pick_B = kPickBatch;
    cp.Hout = H; cp.Wout = W; cp.bias = net->P(p.bproj); cp.res = xin.p; cp.res_pitch = xin.pitch;
    net->split_for(cp);
    if (conv_pw_ok(cp)) {
      emit_conv(cp, y);
      add_conv(cp);
    } else {
      GemmArgs gp{};
      gp.M = B * hw; gp.N = C; gp.K = C; gp.Z1 = 1; gp.Z2 = 1; gp.pick_M = (long)kPickBatch * hw;
      gp.A = Ob; gp.lda = C; gp.Bm = net->P(p.wproj); gp.ldb = C; gp.C = y.p; gp.ldc = y.pitch;
      gp.alpha = 1.f; gp.bias = net->P(p.bproj); gp.res = xin.p; gp.ld_res = xin.pitch;
      net->split_gemm(gp, 6, gp.Bm, (size_t)C * C, 0);
      gn_ready.erase(y.p);
      add_gemm(gp);
    }
    return y;
  }
};

}  // namespace vaeb
}  // namespace dm
