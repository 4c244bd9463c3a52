// C-ABI wrappers over the kernel launchers (include/dm_hip.h).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include "dm_common.h"
#include "dm_kernels.h"

namespace dm {
namespace {
thread_local std::string g_last_error;
}
void set_error(const std::string& msg) { g_last_error = msg; }
const char* last_error() { return g_last_error.c_str(); }

namespace {
thread_local Toggles t_toggles;                  // this thread's last refresh_toggles()
thread_local const Toggles* t_scope = nullptr;   // the innermost ToggleScope
bool env_is(const char* name, char c) {
  const char* e = std::getenv(name);
  return e && e[0] == c;
}
bool g_launch_log_on = false;
bool g_launch_log_convs = false;  // dm_debug_launch_log(2): every dm_conv2d_nhwc* entry logs its conv_label too
std::string g_launch_log;
}  // namespace
const Toggles& toggles() { return t_scope ? *t_scope : t_toggles; }
const Toggles* toggle_scope_swap(const Toggles* t) {
  const Toggles* prev = t_scope;
  t_scope = t;
  return prev;
}
// every environment switch of the library, read here and nowhere else (DESIGN.md §6 toggle table)
void refresh_toggles() {
  Toggles t;
  if (const char* m = std::getenv("DM_CONV_MATH")) {
    const std::string v(m);
    t.conv_math = v == "fp32" ? 0 : v == "bf16x3" ? 3 : 2;
  }
  t.range_check = !env_is("DM_RANGE_CHECK", '0');
  t.graph = std::getenv("DM_NO_GRAPH") == nullptr;
  t.wino = !env_is("DM_CONV_WINO", '0');
  t.subwino = !env_is("DM_CONV_SUBWINO", '0');
  t.k32s_w4 = env_is("DM_K32S_W4", '1');
  t.k32_small = !env_is("DM_CONV_K32S", '0');
  t.k32_s2 = !env_is("DM_CONV_K32S2", '0');
  t.k32_t2d = !env_is("DM_CONV_K32T2", '0');
  t.k32_8x = !env_is("DM_K32_8X", '0');
  t.gn_fusion = !env_is("DM_GN_FUSION", '0');
  if (const char* e = std::getenv("DM_ATTN")) {
    const std::string v(e);
    t.attn = v == "3" ? 3 : v == "0" || v == "presplit" ? 0 : v == "noproj" ? kAttnNoProj : v == "fused" ? kAttnFused
           : v == "unfused" ? kAttnUnfused : 4;
  }
  t.attn_gn_launch = env_is("DM_ATTN_GNFIN", '1');
  t.attn_small = !env_is("DM_ATTN_SMALL", '0');
  t.dit_presplit = !env_is("DM_DIT_PRESPLIT", '0');
  t.lin_sk = !env_is("DM_LIN_SK", '0');
  t.lin_rows = !env_is("DM_LIN_ROWS", '0');
  t_toggles = t;
}
void note_launch(const char* name) {
  if (!g_launch_log_on) return;
  g_launch_log += name;
  g_launch_log += '\n';
}
}  // namespace dm

/* Test hook: enable (1, clearing it) / disable (0) the launch log; read copies it NUL-terminated into buf.
   enable = 2: as 1, and every conv entry (dm_conv2d_nhwc, dm_conv2d_nhwc_s2pad0) logs conv_label of its descriptor
   after the launchers' own lines, as dm_debug_conv2d_gn does -- so a test that forces a tile sees the kernel the
   dispatcher took for it (a forced tile that does not fit falls back without an error). */
extern "C" int dm_debug_launch_log(int enable) {
  dm::g_launch_log_on = enable != 0;
  dm::g_launch_log_convs = enable == 2;
  if (enable) dm::g_launch_log.clear();
  return DM_OK;
}
extern "C" int dm_debug_launch_log_read(char* buf, int len) {
  if (!buf || len <= 0) { dm::set_error("launch log: null buffer"); return DM_ERR_ARG; }
  const size_t n = std::min(dm::g_launch_log.size(), (size_t)len - 1);
  memcpy(buf, dm::g_launch_log.data(), n);
  buf[n] = 0;
  return (int)n;
}

using dm::View;

extern "C" int dm_abi_version(void) { return DM_ABI_VERSION; }

extern "C" const char* dm_last_error(void) { return dm::last_error(); }

#ifndef DM_SRC_HASH
#define DM_SRC_HASH "unknown"
#endif
extern "C" const char* dm_build_info(void) { return "src=" DM_SRC_HASH " arch=gfx950"; }

// dm_step_desc -> StepArgs, with the descriptor's argument checks
static int step_args_from_desc(const dm_step_desc* d, dm::StepArgs& s) {
  if (!d) { dm::set_error("null step descriptor"); return DM_ERR_ARG; }
  s.B = d->B; s.C = d->C; s.HW = d->HW; s.Cm = d->Cm;
  s.xt = d->xt; s.out_c = d->model_out; s.out_u = d->model_out_uncond;
  s.w_u = d->w_uncond; s.w_c = d->w_cond;
  s.objective = d->objective; s.clip = d->clip_denoised;
  s.c_recip = d->sqrt_recip_ac; s.c_recipm1 = d->sqrt_recipm1_ac;
  s.c_sa = d->sqrt_ac; s.c_s1ma = d->sqrt_one_minus_ac;
  s.kind = d->kind; s.m1 = d->coef1; s.m2 = d->coef2;
  s.var_mode = d->var_mode; s.std = d->std;
  s.min_logvar = d->min_logvar; s.max_logvar = d->max_logvar;
  s.add_noise = d->add_noise; s.noise = d->noise;
  s.sample = d->sample; s.mean_out = d->mean; s.x0_out = d->pred_x0; s.eps_out = d->pred_eps;
  s.var_out = d->var;
  s.euler = d->euler; s.e_st1 = d->e_st1; s.e_sig_t = d->e_sig_t; s.e_dsig = d->e_dsig; s.e_sp1 = d->e_sp1;
  s.e_sig_p = d->e_sig_p; s.e_d1 = d->e_d1; s.e_x1 = d->e_x1; s.e_dout = d->e_dout;
  if (s.euler < 0 || s.euler > 2) { dm::set_error("invalid euler mode"); return DM_ERR_ARG; }
  if (s.euler == 2 && (!s.e_d1 || !s.e_x1)) { dm::set_error("Heun second order needs e_d1 and e_x1"); return DM_ERR_ARG; }
  if (s.objective < 0 || s.objective > 2) { dm::set_error("invalid objective"); return DM_ERR_ARG; }
  if (s.kind < 0 || s.kind > 1) { dm::set_error("invalid sampler kind"); return DM_ERR_ARG; }
  if (s.B < 0 || s.C <= 0 || s.HW <= 0) { dm::set_error("invalid shape"); return DM_ERR_ARG; }
  return DM_OK;
}

extern "C" int dm_sampler_step(const dm_step_desc* d, void* stream) {
  dm::StepArgs s{};
  if (const int rc = step_args_from_desc(d, s); rc != DM_OK) return rc;
  return dm::sampler_step(s, (hipStream_t)stream);
}

struct dm_lowpass {
  dm::Lowpass lp;
};

extern "C" int dm_lowpass_create(int H, int W, int N, const float* const* weights, const int32_t* const* left,
                                 const int* taps, void* stream, dm_lowpass** out) {
  if (!weights || !left || !taps || !out) { dm::set_error("low-pass plan: null argument"); return DM_ERR_ARG; }
  dm::Lowpass lp{};
  const int rc = dm::lowpass_create(H, W, N, weights, left, taps, (hipStream_t)stream, &lp);
  if (rc != DM_OK) return rc;
  *out = new dm_lowpass{lp};
  return DM_OK;
}

extern "C" int64_t dm_lowpass_scratch_bytes(const dm_lowpass* p, int64_t planes) {
  if (!p || planes < 0) return -1;
  return (int64_t)dm::lowpass_scratch_floats(p->lp, (long)planes) * (int64_t)sizeof(float);
}

extern "C" int dm_lowpass_apply(const dm_lowpass* p, const float* x, float* y, int64_t planes, void* scratch,
                                void* stream) {
  if (!p) { dm::set_error("low-pass filter: null plan"); return DM_ERR_ARG; }
  return dm::lowpass_apply(p->lp, x, y, (long)planes, (float*)scratch, (hipStream_t)stream);
}

extern "C" void dm_lowpass_destroy(dm_lowpass* p) {
  if (!p) return;
  dm::lowpass_destroy(&p->lp);
  delete p;
}

extern "C" int dm_guided_step(const dm_step_desc* d, const dm_guide_desc* g, void* stream) {
  dm::StepArgs s{};
  if (const int rc = step_args_from_desc(d, s); rc != DM_OK) return rc;
  if (!g) { dm::set_error("null guide descriptor"); return DM_ERR_ARG; }
  dm::GuideArgs a{};
  a.kind = g->kind;
  a.known = g->known; a.eps_k = g->noise_known_eps; a.noise_known = g->noise_known;
  a.c_a = g->sqrt_ac_prev; a.c_b = g->sqrt_one_minus_ac_prev;
  a.mask = g->mask; a.mask_c = g->mask_channels;
  a.lp = g->lowpass ? &g->lowpass->lp : nullptr;
  a.scratch = (float*)g->scratch;
  return dm::guided_step(s, a, (hipStream_t)stream);
}

extern "C" int dm_lincomb(int mode, const float* a, const float* b, float* out, int64_t n, int64_t row_elems,
                          const float* c1_rows, const float* c2_rows, float c1, float c2, void* stream) {
  if (!a || !b || !out) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  if (mode < 0 || mode > 3) { dm::set_error("lincomb mode must be 0 .. 3"); return DM_ERR_ARG; }
  if (n < 0 || row_elems <= 0) { dm::set_error("invalid shape"); return DM_ERR_ARG; }
  return dm::lincomb(mode, a, b, out, (long)n, (long)row_elems, c1_rows, c2_rows, c1, c2, (hipStream_t)stream);
}

extern "C" int64_t dm_groupnorm_scratch_bytes(int B, int HW, int G) {
  return (int64_t)B * dm::gn_num_chunks(HW) * G * (int64_t)sizeof(double2);
}

extern "C" int dm_groupnorm_nhwc(const float* x, int x_pitch, float* y, int y_pitch, int B, int HW, int C, int G,
                                 float eps, const float* gamma, const float* beta, const float* mod_scale,
                                 const float* mod_shift, int mod_pitch, int silu, void* scratch, void* stream) {
  if (!x || !y || !scratch) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  if (B <= 0 || HW <= 0 || C <= 0 || G <= 0) { dm::set_error("invalid shape"); return DM_ERR_ARG; }
  View vx{const_cast<float*>(x), B, HW, 1, C, x_pitch};
  View vy{y, B, HW, 1, C, y_pitch};
  hipStream_t st = (hipStream_t)stream;
  int rc = dm::gn_partial(vx, G, (double2*)scratch, st);
  if (rc) return rc;
  return dm::gn_apply(vx, G, (const double2*)scratch, dm::gn_num_chunks(HW), eps, gamma, beta, mod_scale,
                      mod_shift, mod_pitch, silu ? 1 : 0, vy, st);
}

extern "C" int dm_groupnorm_affine(const float* x, int x_pitch, int B, int HW, int C, int G, float eps,
                                   const float* gamma, const float* beta, float* scale, float* shift, void* scratch,
                                   void* stream) {
  if (!x || !scale || !shift || !scratch) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  if (B <= 0 || HW <= 0 || C <= 0 || G <= 0) { dm::set_error("invalid shape"); return DM_ERR_ARG; }
  View vx{const_cast<float*>(x), B, HW, 1, C, x_pitch};
  hipStream_t st = (hipStream_t)stream;
  int rc = dm::gn_partial(vx, G, (double2*)scratch, st);
  if (rc) return rc;
  return dm::gn_finalize(vx, G, (const double2*)scratch, eps, gamma, beta, scale, shift, st);
}

extern "C" int dm_pack_conv_weight(const float* w, int Cout, int Cin, int taps, float* out, int ldw, int col0,
                                   void* stream) {
  if (!w || !out) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  if (Cout <= 0 || Cin <= 0 || (taps != 1 && taps != 9) || col0 + taps * Cin > ldw) {
    dm::set_error("invalid conv weight shape");
    return DM_ERR_ARG;
  }
  return dm::repack_conv(w, Cout, Cin, taps, out, ldw, col0, (hipStream_t)stream);
}

// dm_conv2d_nhwc and its variants: s2_pad0 (dm_conv2d_nhwc_s2pad0), GroupNorm(gn_G) statistics of the stored output
// from the epilogue into gn_part (dm_debug_conv2d_gn)
// (gin: dm_debug_conv2d_gin's in-kernel GroupNorm finalize of the prologue, ConvArgs::gin_*)
struct GinHook {
  const double2* part;
  int G, nchunk;
  float eps;
  const float *gamma, *beta, *ms, *mb;
  int mp;
};
// the ConvArgs of a descriptor (no HIP call, no tensor read: dm_debug_conv_choice builds its ConvArgs here too)
static int conv_args_from_desc(const dm_conv_desc* d, int s2_pad0, double2* gn_part, int gn_G, const GinHook* gin,
                               dm::ConvArgs& a) {
  dm::refresh_toggles();
  if (!d || !d->x || !d->w || !d->y) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  a = dm::ConvArgs{};
  a.s2_pad0 = s2_pad0;
  a.gn_part = gn_part;
  a.gn_G = gn_G;
  a.x1 = d->x; a.x1_pitch = d->x_pitch; a.Cin1 = d->Cin; a.Hin = d->Hin; a.Win = d->Win;
  a.taps = d->taps; a.stride = d->stride; a.upsample = d->upsample;
  a.x2 = d->x2; a.x2_pitch = d->x2_pitch; a.Cin2 = d->Cin2;
  a.w = d->w; a.K = d->K;
  a.y = d->y; a.y_pitch = d->y_pitch; a.Cout = d->Cout; a.B = d->B; a.Hout = d->Hout; a.Wout = d->Wout;
  a.bias = d->bias; a.rowvec = d->rowvec; a.rowvec_pitch = d->rowvec_pitch;
  a.res = d->res; a.res_pitch = d->res_pitch;
  a.tile = d->tile;
  a.pro_scale = d->pro_scale;
  a.pro_shift = d->pro_shift;
  a.pro_nosilu = d->pro_nosilu;
  a.ksplit = d->ksplit;
  a.kpart = d->kpart;
  a.ws = d->w_split;
  if (a.ws) {
    if (d->w_split_kind != DM_SPLIT_BF16X3 && d->w_split_kind != DM_SPLIT_FP16X2) {
      dm::set_error("conv: w_split_kind must be DM_SPLIT_BF16X3 or DM_SPLIT_FP16X2");
      return DM_ERR_ARG;
    }
    a.ws_np = d->w_split_kind;
    if (a.ws_np == DM_SPLIT_FP16X2)
      a.ws_rowscale = dm::split_conv_rowscale(a.ws, a.upsample == 2 ? 4 : 1, a.Cout, a.K);
    a.range_flag = d->range_flag;
  }
  if (d->w_wino) {
    if (!a.ws || a.ws_np != DM_SPLIT_FP16X2) {
      dm::set_error("conv: w_wino needs w_split of kind DM_SPLIT_FP16X2");
      return DM_ERR_ARG;
    }
    if (a.upsample == 2) {  // the sub-pixel form: w_wino is dm_pack_conv_weight_subwino's image
      a.subwino_ws = d->w_wino;
      a.subwino_rowscale = dm::subwino_rowscale(d->w_wino, a.Cout, a.Cin1);
    } else {
      a.wino_ws = d->w_wino;
      a.wino_rowscale = dm::wino_rowscale(d->w_wino, a.Cout, a.Cin1, a.Cin2);
      a.wino_fold = d->w_wino_fold;
    }
  }
  if (gin) {
    if (a.pro_scale || !gin->part || gin->G <= 0 || a.Cin1 <= 0 || a.Cin1 % gin->G != 0 || gin->nchunk <= 0 ||
        (gin->ms != nullptr) != (gin->mb != nullptr)) {
      dm::set_error("dm_debug_conv2d_gin: arguments");
      return DM_ERR_ARG;
    }
    // the plans leave their (then unread) table pointers in pro_scale / pro_shift: the kernels take the presence of
    // a prologue from them and read the partials instead. Here the partials' own address stands in.
    a.pro_scale = a.pro_shift = reinterpret_cast<const float*>(gin->part);
    a.gin_part = gin->part; a.gin_G = gin->G; a.gin_nchunk = gin->nchunk;
    a.gin_n = (double)a.Hin * a.Win * (a.Cin1 / gin->G);
    a.gin_eps = gin->eps; a.gin_gamma = gin->gamma; a.gin_beta = gin->beta;
    a.gin_ms = gin->ms; a.gin_mb = gin->mb; a.gin_mp = gin->mp;
    if (!dm::conv_choose(a).lds_tables) {
      dm::set_error("dm_debug_conv2d_gin: the conv does not stage its GroupNorm tables in LDS (ConvChoice::lds_tables)");
      return DM_ERR_UNSUPPORTED;
    }
  }
  return DM_OK;
}

static int conv2d_from_desc(const dm_conv_desc* d, int s2_pad0, double2* gn_part, int gn_G, void* stream,
                            const GinHook* gin = nullptr) {
  dm::ConvArgs a;
  if (const int rc0 = conv_args_from_desc(d, s2_pad0, gn_part, gn_G, gin, a)) return rc0;
  const dm::ConvChoice ch = dm::conv_choose(a);
  const int rc = dm::conv2d_run(a, ch, (hipStream_t)stream);
  // dm_debug_conv2d_gn / dm_debug_conv2d_gin (null on every other entry) and dm_debug_launch_log(2): the label of the
  // choice that was launched goes to the launch log after the launchers' own lines
  if ((gn_part || gin || dm::g_launch_log_convs) && rc == DM_OK) dm::note_launch(dm::conv_label(a, ch).c_str());
  return rc;
}

extern "C" int dm_conv2d_nhwc(const dm_conv_desc* d, void* stream) { return conv2d_from_desc(d, 0, nullptr, 0, stream); }

extern "C" int dm_conv2d_nhwc_s2pad0(const dm_conv_desc* d, void* stream) {
  if (d && !(d->taps == 9 && d->stride == 2 && d->upsample == 0)) {
    dm::set_error("dm_conv2d_nhwc_s2pad0: the bottom/right-padded form is for 3x3 stride-2 convs");
    return DM_ERR_ARG;
  }
  return conv2d_from_desc(d, 1, nullptr, 0, stream);
}

// Operator tests of the producer epilogues' GroupNorm statistics: the conv of `d` (s2_pad0 as above) with the
// statistics of its stored output for GroupNorm(G) written to part ([B][ceil(Hout Wout / 64)][G] {sum, sum of
// squares}, the layout dm_groupnorm_affine leaves in its scratch). Fails where the chosen kernel cannot emit them.
// With the launch log on, the conv's kernel instantiation (conv_label) is logged after the launchers' own lines.
extern "C" int dm_debug_conv2d_gn(const dm_conv_desc* d, int s2_pad0, int G, void* part, void* stream) {
  if (!part || G <= 0 || (s2_pad0 != 0 && s2_pad0 != 1)) { dm::set_error("dm_debug_conv2d_gn: arguments"); return DM_ERR_ARG; }
  return conv2d_from_desc(d, s2_pad0, (double2*)part, G, stream);
}

// Operator tests of the convs' in-kernel GroupNorm finalize (tests/test_gpu_norm_ops.py): the conv of `d` (pro_scale
// null, pro_nosilu honoured) with its prologue tables built in the kernel from the chunk partials gin_part
// [B][gin_nchunk][gin_G] of x, gin_n = Hin Win Cin / gin_G. DM_ERR_UNSUPPORTED where ConvChoice::lds_tables is false;
// gin_ms and gin_mb come together or not at all (the plans' AdaGN form).
extern "C" int dm_debug_conv2d_gin(const dm_conv_desc* d, int s2_pad0, const void* gin_part, int gin_G, int gin_nchunk,
                                   float gin_eps, const float* gin_gamma, const float* gin_beta, const float* gin_ms,
                                   const float* gin_mb, int gin_mp, void* stream) {
  if (s2_pad0 != 0 && s2_pad0 != 1) { dm::set_error("dm_debug_conv2d_gin: arguments"); return DM_ERR_ARG; }
  const GinHook gin{(const double2*)gin_part, gin_G, gin_nchunk, gin_eps, gin_gamma, gin_beta, gin_ms, gin_mb, gin_mp};
  const int rc = conv2d_from_desc(d, s2_pad0, nullptr, 0, stream, &gin);
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == DM_OK) { dm::set_error("sync"); return DM_ERR_HIP; }
  return rc;
}

// Host-only window onto the conv dispatch (tests/test_conv_dispatch_host.py): which kernel the conv of `d` would run,
// without a HIP call or a tensor read. The ConvArgs are conv2d_from_desc's, plus what the plans set beside a
// descriptor: pick_B, a split-K workspace (ksplit_has_part: a stand-in address where d->kpart is null), the conv-half
// mark with stand-in planes (h16), statistics requested from the epilogue (gn_emit: gn_part set, GroupNorm(gn_G)) and
// the in-kernel GroupNorm finalize (gin_G > 0). Everything reported is conv_choose's: label, launched ("family:variant",
// or "refused"), lds_tables; emits_gn from the choice of the same conv with gn_part set, as the plans ask (0 where
// gn_G <= 0).
extern "C" int dm_debug_conv_choice(const dm_conv_desc* d, int s2_pad0, int gn_G, int gn_emit, int pick_B,
                                    int ksplit_has_part, int h16, int gin_G, int gin_nchunk, char* label, int label_len,
                                    int* emits_gn, int* lds_tables, char* launched, int launched_len) {
  if (!d || !label || label_len <= 0 || !emits_gn || !lds_tables || !launched || launched_len <= 0) {
    dm::set_error("dm_debug_conv_choice: arguments");
    return DM_ERR_ARG;
  }
  auto put = [](char* dst, int len, const std::string& s) {
    const size_t n = std::min(s.size(), (size_t)len - 1);
    memcpy(dst, s.data(), n);
    dst[n] = 0;
  };
  put(label, label_len, "");
  put(launched, launched_len, "refused");
  *emits_gn = *lds_tables = 0;
  double2* const standin = reinterpret_cast<double2*>(uintptr_t(1) << 20);  // never read
  const GinHook gin{standin, gin_G, gin_nchunk, 1e-5f, reinterpret_cast<const float*>(standin),
                    reinterpret_cast<const float*>(standin), nullptr, nullptr, 0};
  dm::ConvArgs a;
  if (conv_args_from_desc(d, s2_pad0, gn_emit ? standin : nullptr, gn_G, gin_G > 0 ? &gin : nullptr, a)) return DM_OK;
  a.pick_B = pick_B;
  if (ksplit_has_part && !a.kpart) a.kpart = reinterpret_cast<float*>(standin);
  if (h16) {
    a.h16 = 1;
    a.h16_a1 = reinterpret_cast<const _Float16*>(standin);
    if (a.Cin2 > 0) a.h16_a2 = reinterpret_cast<const _Float16*>(standin);
  }
  const dm::ConvChoice ch = dm::conv_choose(a);
  if (ch.error) return DM_OK;
  put(launched, launched_len, dm::conv_choice_name(a, ch));
  put(label, label_len, dm::conv_label(a, ch));
  if (gn_G > 0) {
    dm::ConvArgs e = a;
    e.gn_part = standin;
    *emits_gn = dm::conv_choose(e).emits_gn ? 1 : 0;
  }
  *lds_tables = ch.lds_tables ? 1 : 0;
  return DM_OK;
}

extern "C" int64_t dm_conv_weight_wino_bytes(int Cout, int Cin, int Cin2) {
  if (Cout <= 0 || Cin <= 0 || Cin % 32 != 0 || Cin2 < 0 || Cin2 % 64 != 0) return -1;
  return (int64_t)dm::wino_weights_bytes(Cout, Cin, Cin2);
}

extern "C" int dm_pack_conv_weight_wino(const float* w, int Cout, int Cin, int Cin2, int fold, void* out, void* stream) {
  return dm::wino_weights(w, Cout, Cin, Cin2, fold, out, (hipStream_t)stream);
}

extern "C" int64_t dm_conv_weight_subwino_bytes(int Cout, int Cin) {
  if (Cout <= 0 || Cin <= 0 || Cin % 32 != 0) return -1;
  return (int64_t)dm::subwino_weights_bytes(Cout, Cin);
}

extern "C" int dm_pack_conv_weight_subwino(const float* w, int Cout, int Cin, void* out, void* stream) {
  return dm::subwino_weights(w, Cout, Cin, out, (hipStream_t)stream);
}

extern "C" int64_t dm_conv_weight_split_bytes(int nmat, int Cout, int K, int kind) {
  if (nmat <= 0 || Cout <= 0 || K <= 0 || K % 16 != 0) return 0;
  if (kind != DM_SPLIT_BF16X3 && kind != DM_SPLIT_FP16X2) return 0;
  return (int64_t)dm::split_conv_weights_bytes(nmat, Cout, K, kind);
}

extern "C" int dm_pack_conv_weight_split(const float* w, int nmat, int Cout, int K, int Cin, int taps, int kind,
                                         void* out, void* stream) {
  if (!w || !out) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  return dm::split_conv_weights(w, nmat, Cout, K, Cin, taps, kind, out, (hipStream_t)stream);
}

extern "C" int dm_pack_conv_weight_subpixel(const float* w, int Cout, int Cin, float* out, void* stream) {
  if (!w || !out) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  return dm::repack_subpixel(w, Cout, Cin, out, (hipStream_t)stream);
}

// dm_gemm; with gn_part (dm_debug_gemm_gn) also the GroupNorm(gn_G) statistics of the output rows, images of gn_hw rows
static int gemm_from_desc(const dm_gemm_desc* d, double2* gn_part, int gn_G, int gn_hw, void* stream,
                          int64_t pick_M = 0, int64_t pick_Z = 0, bool log = false) {
  dm::refresh_toggles();
  if (!d || !d->A || !d->B || !d->C) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  dm::GemmArgs g{};
  g.M = d->M; g.N = d->N; g.K = d->K; g.Z1 = d->Z1; g.Z2 = d->Z2;
  g.pick_M = (long)pick_M; g.pick_Z = (long)pick_Z;
  g.A = d->A; g.a_s1 = d->a_s1; g.a_s2 = d->a_s2; g.lda = d->lda;
  g.Bm = d->B; g.b_s1 = d->b_s1; g.b_s2 = d->b_s2; g.ldb = d->ldb; g.b_kn = d->b_kn;
  g.C = d->C; g.c_s1 = d->c_s1; g.c_s2 = d->c_s2; g.ldc = d->ldc;
  g.alpha = d->alpha; g.bias = d->bias; g.res = d->res; g.ld_res = d->ld_res; g.act = d->act;
  g.b_scale = d->b_scale;
  g.split = d->split; g.split_ea = d->split_ea; g.split_eb = d->split_eb; g.range_flag = d->range_flag;
  g.gn_part = gn_part; g.gn_G = gn_G; g.gn_hw = gn_hw;
  const int rc = dm::gemm_batched(g, (hipStream_t)stream);
  if (log && rc == DM_OK) dm::note_launch(dm::gemm_label(g).c_str());
  return rc;
}

extern "C" int dm_gemm(const dm_gemm_desc* d, void* stream) { return gemm_from_desc(d, nullptr, 0, 0, stream); }

// Operator tests of the GEMM epilogue's GroupNorm statistics (GemmArgs::gn_part): dm_gemm with the statistics of its
// output for GroupNorm(G) over images of hw rows written to part [M / hw][hw / 64][G]. Synchronous.
extern "C" int dm_debug_gemm_gn(const dm_gemm_desc* d, int G, int hw, void* part, void* stream) {
  if (!part || G <= 0 || hw <= 0) { dm::set_error("dm_debug_gemm_gn: arguments"); return DM_ERR_ARG; }
  const int rc = gemm_from_desc(d, (double2*)part, G, hw, stream);
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == DM_OK) { dm::set_error("sync"); return DM_ERR_HIP; }
  return rc;
}

// Operator tests of the unfused attention chain (tests/test_gpu_unfused_attention_ops.py): dm_gemm with the tile
// heuristic's nominal M and Z1 * Z2 (GemmArgs::pick_M / pick_Z, 0: the actual ones) as the plans pass them, so the
// 128 x 128 batched instances run on a two-image buffer. Synchronous; with the launch log on, gemm_label is logged.
extern "C" int dm_debug_gemm_pick(const dm_gemm_desc* d, int64_t pick_M, int64_t pick_Z, void* stream) {
  if (pick_M < 0 || pick_Z < 0) { dm::set_error("dm_debug_gemm_pick: arguments"); return DM_ERR_ARG; }
  const int rc = gemm_from_desc(d, nullptr, 0, 0, stream, pick_M, pick_Z, true);
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess && rc == DM_OK) { dm::set_error("sync"); return DM_ERR_HIP; }
  return rc;
}

extern "C" int dm_softmax_rows(float* x, int64_t rows, int L, int ld, void* stream) {
  if (!x) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  return dm::softmax_rows(x, rows, L, ld, (hipStream_t)stream);
}

extern "C" int dm_timestep_embedding(const int64_t* t, int B, int dim, int kind, const float* freqs, float* out,
                                     void* stream) {
  if (!t || !out) { dm::set_error("null tensor"); return DM_ERR_ARG; }
  if (B <= 0) { dm::set_error("empty batch"); return DM_ERR_ARG; }
  return dm::timestep_embed(t, B, dim, kind, freqs, out, (hipStream_t)stream);
}
