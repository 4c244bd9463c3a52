// What the model executors (unet_exec.hip, dit_exec.hip, vae_exec.hip, vae_enc_exec.hip) share: the weight arena and
// the arithmetic / fp16 range state of one network (ExecNet), the forward driver with its range fallback
// (run_forward), and the bodies of the C ABI entry points every model handle has (abi_*).
#pragma once
#include <algorithm>
#include <map>
#include <string>
#include <utility>

#include "dm_common.h"
#include "dm_kernels.h"
#include "plan.h"

namespace dm {

// The split count of the Winograd kernel on a 4 x 4 map, 0 where the plan keeps the direct kernel: 4 splits when a
// split has >= 12 K steps of 32 channels (the UNet plan's maybe_split; split_for attaches the Winograd weights to
// those only)
inline int wino_small_ks(const ConvArgs& c) {
  if (c.Hout != 4 || c.Wout != 4) return 0;
  const int ks = std::min(4, c.Cin1 / 32);
  return ks >= 2 && (3 * (c.Cin1 / 32) + c.Cin2 / 64) / ks >= 12 ? ks : 0;
}

// The weight arena and the arithmetic state of one network.
// base_math: the arithmetic the caller chose -- 2 fp16x2 (default), 3 bf16x3, 0 fp32 MFMA kernels
// (DM_CONV_MATH=fp16x2|bf16x3|fp32). fp16x2 kernels raise range_flag on an operand beyond the fp16 range; that
// forward then runs again in fallback_math (3 for the conv nets, 0 for DiT / MDT) and the next one is fp16x2 again
// (not sticky: plans are cached per (shape, arithmetic)). In deferred mode (abi_set_range_deferred) forwards neither
// read the flag nor sync; the caller polls it once per sampling loop (abi_range_poll), and its re-run of a flagged
// loop runs in fallback_math while `fallback` is set (abi_range_fallback clears it). DM_RANGE_CHECK=0 skips the
// check and its sync. conv_math is the arithmetic of the plan being built (set by the model's get_plan).
// DM_MATH_FP16 (1, the token models only: dit_exec.hip) is range-checked in the same way: its operands are fp16 too.
inline bool math_range_checked(int kind) { return kind == DM_SPLIT_FP16X2 || kind == DM_MATH_FP16; }

struct ExecNet {
  float* arena = nullptr;
  size_t arena_floats = 0;
  int base_math = conv_math_from_env();
  int fallback_math = 3;
  bool fallback = false;
  int conv_math = base_math;
  bool range_check = toggles().range_check;
  int* range_flag = nullptr;       // device
  int* range_flag_host = nullptr;  // pinned
  bool range_deferred = false;
  long range_fallbacks = 0;  // forwards / loops re-run in fallback_math
  // split copies of the conv / GEMM weights per (packed weights, arithmetic), Winograd F(2,3) weights per (packed
  // weights, shortcut fold), made at the first plan build that wants them
  std::map<std::pair<const float*, int>, void*> split_w;
  std::map<std::pair<const float*, int>, void*> wino_w;
  std::map<const float*, void*> subwino_w;  // sub-pixel Winograd images per packed U matrices (subwino_for)
  size_t split_bytes = 0;
  std::map<const float*, int> w_exp;  // fp16x2 GEMMs: the weights' operand exponents (split_gemm)
  // the UNet plans put the Winograd kernel on 4 x 4 maps (a split-K form, where maybe_split chose wino_small_ks
  // splits); the other networks keep the direct kernel there
  bool wino_small = false;
  // The conv-half option of the conv UNets (dm_unet_set_conv_half), a switch beside the arithmetic, not
  // a fourth kind of it: in a plan of the fp16x2 arithmetic the 3x3 stride-1 convs conv_h16_ok takes run with one fp16
  // product per MAC (conv_h16.hip). base_math keeps governing everything else and stays the range fallback's source;
  // fp32 / bf16x3 plans (the fallback's included) are unchanged. Off by default; the other networks never set it.
  bool conv_half = false;
  bool half_active() const { return conv_half && conv_math == DM_SPLIT_FP16X2; }

  ExecNet() = default;
  ExecNet(const ExecNet&) = delete;
  ExecNet& operator=(const ExecNet&) = delete;
  ~ExecNet() {
    for (auto& kv : split_w) (void)hipFree(kv.second);
    for (auto& kv : wino_w) (void)hipFree(kv.second);
    for (auto& kv : subwino_w) (void)hipFree(kv.second);
    if (range_flag) (void)hipFree(range_flag);
    if (range_flag_host) (void)hipHostFree(range_flag_host);
    if (arena) (void)hipFree(arena);
  }
  float* P(size_t off) const { return arena + off; }
  int run_math() const { return math_range_checked(base_math) && fallback ? fallback_math : base_math; }

  int ensure_range_flag() {
    if (!range_flag) {
      DM_CHECK_HIP(hipMalloc(&range_flag, sizeof(int)));
      DM_CHECK_HIP(hipMemset(range_flag, 0, sizeof(int)));
      DM_CHECK_HIP(hipHostMalloc(&range_flag_host, sizeof(int)));
    }
    return DM_OK;
  }
  // Read the range flag back on st (one 4-byte copy and a stream sync) and clear it if it was raised
  int take_range_flag(hipStream_t st, bool* raised) {
    DM_CHECK_HIP(hipMemcpyAsync(range_flag_host, range_flag, sizeof(int), hipMemcpyDeviceToHost, st));
    DM_CHECK_HIP(hipStreamSynchronize(st));
    *raised = *range_flag_host != 0;
    if (*raised) DM_CHECK_HIP(hipMemsetAsync(range_flag, 0, sizeof(int), st));
    return DM_OK;
  }

  // Attach the split copy (and, for the shapes conv_wino takes, the Winograd weights) of a conv's packed weights;
  // none: the conv stays on the fp32 kernels. A bottom/right-padded stride-2 conv that conv_split_eligible
  // (conv_patch3 MODE 4's 384-pixel patch) turns down also gets split weights when conv_k32 itself would run it
  // given them (the KL encoder's first downsamples: the whole-row tile's 390-pixel patch at Wout = 64, the
  // row-segment tile beyond; the pesser UNet's Downsample), and only then: no split copy is made for a conv that
  // stays on im2col.
  void split_for(ConvArgs& c) {
    c.h16 = 0;
    c.ws = nullptr;
    c.ws_np = 0;
    c.ws_rowscale = nullptr;
    c.range_flag = nullptr;
    c.wino_ws = nullptr;
    c.wino_rowscale = nullptr;
    bool s2seg = false;
    if (conv_math == 2 && c.s2_pad0 && c.stride == 2 && c.taps == 9) {
      ConvArgs t = c;
      t.ws = conv_standin<const void>();
      t.ws_np = 2;
      t.ws_rowscale = conv_standin<const float>();
      s2seg = conv_choose(t).k32_stride2();
    }
    if (!conv_math || !(conv_split_eligible(c) || (conv_math == 2 && conv_seg_eligible(c)) || s2seg)) return;
    if ((c.taps == 1 || c.stride == 2) && conv_math != 2) return;  // the split 1x1 / stride-2 paths are fp16x2 only
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
    // conv-half plans: a covered conv that got its fp16x2 copy is marked for conv_h16 (conv_h16.hip) and takes no
    // Winograd weights; a conv the gate refuses runs as in fp16x2
    if (half_active()) {
      ConvArgs t = c;
      t.gn_part = nullptr;  // (the statistics rule is conv_can_emit_gn's, asked by the plan)
      if (conv_h16_ok(t)) {
        c.h16 = 1;
        return;
      }
    }
    // the Winograd F(2,3) kernel for the 3x3 convs it takes (DM_CONV_WINO=0: conv_k32, its test oracle)
    if (conv_math != 2 || !toggles().wino || !conv_wino_shape_ok(c)) return;
    if (c.Wout == 4 && !(wino_small && c.ksplit == wino_small_ks(c))) return;  // (4 x 4: the plan's split decision)
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

  // Attach the sub-pixel Winograd weights (conv_subwino.hip) to an upsample conv in its sub-pixel form that split_for
  // gave its fp16x2 copy: u = the packed U matrices [6][Cout][2 Cin] (Packer::subwino), split on first use.
  // DM_CONV_SUBWINO=0, another arithmetic, a conv-half conv or a shape the kernel does not take: the conv stays as it is.
  void subwino_for(ConvArgs& c, const float* u) {
    c.subwino_ws = nullptr;
    c.subwino_rowscale = nullptr;
    if (!u || conv_math != 2 || !toggles().subwino || c.ws_np != 2 || !c.ws || c.h16 || !conv_subwino_shape_ok(c)) return;
    auto it = subwino_w.find(u);
    void* wp = nullptr;
    if (it != subwino_w.end()) {
      wp = it->second;
    } else {
      const size_t nb = subwino_weights_bytes(c.Cout, c.Cin1);
      if (hipMalloc(&wp, nb) != hipSuccess) {
        (void)hipGetLastError();
        return;
      }
      if (split_conv_weights(u, 6, c.Cout, 2 * c.Cin1, c.Cin1, 2, 2, wp, nullptr) != DM_OK ||
          hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(wp);
        return;
      }
      subwino_w[u] = wp;
      split_bytes += nb;
    }
    c.subwino_ws = wp;
    c.subwino_rowscale = subwino_rowscale(wp, c.Cout, c.Cin1);
  }

  // fp16x2 GEMMs (gemm.hip SPLIT): A scaled by 2^ea, B by the weight's exponent (max |w| * 2^eb in [2^13, 2^14);
  // cached in w_exp) or, for an activation B, 2^eb_act. Activations use fixed exponents that keep their low fp16
  // pieces normal down to ~2^-8 while leaving headroom to 65504 / 2^e (the range flag catches the rest):
  // normalised inputs, q, k, v and the attention output 2^6, softmax rows (<= 1) 2^14.
  void split_gemm(GemmArgs& g, int ea, const float* weight, size_t weight_n, int eb_act = 0) {
    g.split = 0;
    if (conv_math != 2) return;
    int eb = eb_act;
    if (weight) {
      auto it = w_exp.find(weight);
      if (it == w_exp.end()) it = w_exp.emplace(weight, split_weight_exponent(weight, weight_n)).first;
      eb = it->second;
    }
    g.split = 2;
    g.split_ea = ea;
    g.split_eb = eb;
    g.range_flag = range_flag;
  }
};

// One forward of model m (an ExecNet with a PlanCache `plans`) on st, in at most two passes: the caller's
// arithmetic, then (an fp16x2 operand beyond the fp16 range) the same forward in m.fallback_math; the model's next
// forward is fp16x2 again. get_plan(math, &plan) finds or builds the plan, stage_in(plan) / stage_out(plan) enqueue
// the copies between the caller's tensors and the plan's. Every exit after order() records the completion event, so
// a later forward on another stream waits for whatever this one enqueued over the shared slab, even when it failed
// part way. The callables are template parameters: a graph-replay forward is host-latency-bound and allocates
// nothing here.
template <class M, class GetPlan, class StageIn, class StageOut>
int run_forward(M& m, hipStream_t st, GetPlan get_plan, StageIn stage_in, StageOut stage_out) {
  ScratchPool& pool = *m.plans.pool;
  if (const int rc = pool.order(st)) return rc;
  const int rc_body = [&]() -> int {
    for (int math = m.run_math();; math = m.fallback_math) {
      typename M::Plan* pl = nullptr;
      if (const int rc = get_plan(math, &pl)) return rc;
      if (const int rc = stage_in(*pl)) return rc;
      if (const int rc = pl->run(st)) return rc;
      if (const int rc = stage_out(*pl)) return rc;
      if (!math_range_checked(math) || !m.range_check || m.range_deferred) return DM_OK;
      bool raised = false;
      if (const int rc = m.take_range_flag(st, &raised)) return rc;
      if (!raised) return DM_OK;
      m.range_fallbacks++;
    }
  }();
  const int rc_mark = pool.mark(st);
  return rc_body ? rc_body : rc_mark;
}

// ---------------------------------------------------------------------------
// C ABI bodies: each extern "C" entry point is model_of(handle) and one of these
// ---------------------------------------------------------------------------
template <class H>
auto model_of(H* h) -> decltype(h->m) {
  return h ? h->m : nullptr;
}

#define DM_ABI_MODEL(m)          \
  if (!(m)) {                    \
    ::dm::set_error("null model"); \
    return DM_ERR_STATE;         \
  }

inline int abi_set_range_deferred(ExecNet* m, int deferred) {
  DM_ABI_MODEL(m);
  m->range_deferred = deferred != 0;
  return DM_OK;
}

inline int abi_range_poll(ExecNet* m, hipStream_t st, int* flagged) {
  DM_ABI_MODEL(m && flagged);
  *flagged = 0;
  if (!m->range_flag) return DM_OK;  // no fp16x2 plan was ever built
  bool raised = false;
  if (const int rc = m->take_range_flag(st, &raised)) return rc;
  if (raised) {
    *flagged = 1;
    if (math_range_checked(m->base_math)) {  // the caller re-runs what it computed since the last poll: in fallback_math
      m->fallback = true;
      m->range_fallbacks++;
    }
  }
  return DM_OK;
}

inline int abi_range_fallback(ExecNet* m, int on) {
  DM_ABI_MODEL(m);
  m->fallback = on != 0;
  return DM_OK;
}

inline int abi_range_stats(const ExecNet* m, int64_t* fallbacks, int* active) {
  DM_ABI_MODEL(m);
  if (fallbacks) *fallbacks = m->range_fallbacks;
  if (active) *active = m->run_math();
  return DM_OK;
}

inline int abi_get_math(const ExecNet* m, int* kind) {
  DM_ABI_MODEL(m && kind);
  *kind = m->base_math;
  return DM_OK;
}

// bf16x3_ok: the conv nets take 0, fp16x2 and bf16x3; fp16_ok: the token models take 0, fp16x2 and DM_MATH_FP16
template <class M>
int abi_set_math(M* m, int kind, bool bf16x3_ok, bool fp16_ok = false) {
  DM_ABI_MODEL(m);
  if (kind != 0 && kind != DM_SPLIT_FP16X2 && !(bf16x3_ok && kind == DM_SPLIT_BF16X3) &&
      !(fp16_ok && kind == DM_MATH_FP16)) {
    set_error(std::string("math must be 0 (fp32)") + (bf16x3_ok ? ", DM_SPLIT_BF16X3" : "") +
              (fp16_ok ? ", DM_MATH_FP16" : "") + " or DM_SPLIT_FP16X2" +
              (fp16_ok ? "" : " (DM_MATH_FP16 is for the token models, dm_dit_* / dm_mdt_*, only)"));
    return DM_ERR_ARG;
  }
  m->fallback = false;
  if (kind != m->base_math) {
    m->base_math = kind;
    m->plans.clear();
  }
  return DM_OK;
}

// the fp32 arena plus the split copies of the weights; the plan scratch
template <class M>
int abi_memory(const M* m, int64_t* weight_bytes, int64_t* workspace_bytes) {
  DM_ABI_MODEL(m);
  if (weight_bytes) *weight_bytes = (int64_t)(m->arena_floats * sizeof(float) + m->split_bytes);
  if (workspace_bytes) *workspace_bytes = (int64_t)m->plans.pool->bytes();
  return DM_OK;
}

template <class M>
int abi_plan_stats(const M* m, int64_t* builds, int* cached) {
  DM_ABI_MODEL(m);
  if (builds) *builds = m->plans.builds;
  if (cached) *cached = (int)m->plans.plans.size();
  return DM_OK;
}

// Install (freqs null: drop) the host-evaluated sinusoid frequency table of a model with a time embedding
// (members freqs: arena offset, n_freqs, freqs_set); launches read freqs_set at capture time
template <class M>
int abi_set_time_freqs(M* m, const float* freqs, int n, hipStream_t st) {
  DM_ABI_MODEL(m);
  if (freqs) {
    if (n != m->n_freqs) {
      set_error("time frequency table must have " + std::to_string(m->n_freqs) + " entries");
      return DM_ERR_ARG;
    }
    DM_CHECK_HIP(hipMemcpyAsync(m->P(m->freqs), freqs, (size_t)n * sizeof(float), hipMemcpyDefault, st));
  }
  m->freqs_set = freqs != nullptr;
  m->plans.invalidate_graphs();
  return DM_OK;
}

template <class M>
int abi_profile(M* m, int enable) {
  DM_ABI_MODEL(m);
  if (!m->plans.current()) { set_error("no plan yet: run a forward once first"); return DM_ERR_STATE; }
  m->plans.current()->profile_enable(enable);
  return DM_OK;
}

template <class M>
int abi_profile_count(M* m, int* n_ops) {
  DM_ABI_MODEL(m);
  if (!m->plans.current() || !n_ops) { set_error("no plan"); return DM_ERR_STATE; }
  *n_ops = (int)m->plans.current()->ops.size();
  return DM_OK;
}

template <class M>
int abi_profile_get(M* m, int i, char* label, int label_len, double* flops, double* bytes, double* ms_total,
                    int64_t* launches) {
  DM_ABI_MODEL(m);
  if (!m->plans.current()) { set_error("no plan"); return DM_ERR_STATE; }
  return m->plans.current()->profile_get(i, label, label_len, flops, bytes, ms_total, launches);
}

template <class H>
void abi_destroy(H* h) {
  if (!h) return;
  (void)hipDeviceSynchronize();
  delete h->m;
  delete h;
}

}  // namespace dm
