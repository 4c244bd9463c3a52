// Create-time helpers shared by the conv-net executors (the UNet and both VAE networks): reading the caller's
// state_dict tensors in registration order and packing them into one library-owned device arena (ExecNet::arena,
// exec_core.h).
#pragma once
#include <string>
#include <vector>

#include "dm_common.h"
#include "dm_kernels.h"

namespace dm {

struct ParamReader {
  const float* const* params;
  const int64_t* numels;
  int n, pos = 0;
  std::string err;
  const float* take(int64_t expect, const char* what) {
    if (pos >= n) {
      if (err.empty()) err = std::string("too few parameters at ") + what;
      return nullptr;
    }
    if (numels[pos] != expect && err.empty())
      err = "parameter " + std::to_string(pos) + " (" + what + "): expected " + std::to_string(expect) +
            " elements, got " + std::to_string(numels[pos]);
    return params[pos++];
  }
};

// A copy / repack job into the weight arena.
struct PackJob {
  int kind;  // 0 raw copy, 1 conv repack, 2 add (bias sum), 3 sub-pixel upsample repack, 4 sub-pixel Winograd U matrices
  const float* src;
  const float* src2;
  int64_t n;
  int Cout, Cin, taps, ldw, col0;
  size_t dst;  // float offset in arena
};

struct Packer {
  std::vector<PackJob> jobs;
  size_t size = 0;
  size_t reserve(int64_t n) {
    size_t off = size;
    size += ((size_t)n + 63) / 64 * 64;
    return off;
  }
  size_t raw(const float* src, int64_t n) {
    size_t off = reserve(n);
    jobs.push_back({0, src, nullptr, n, 0, 0, 0, 0, 0, off});
    return off;
  }
  void raw_at(const float* src, int64_t n, size_t off) { jobs.push_back({0, src, nullptr, n, 0, 0, 0, 0, 0, off}); }
  void conv_at(const float* w, int Cout, int Cin, int taps, int ldw, int col0, size_t off) {
    jobs.push_back({1, w, nullptr, (int64_t)Cout * Cin * taps, Cout, Cin, taps, ldw, col0, off});
  }
  void add_at(const float* a, const float* b, int64_t n, size_t off) {
    jobs.push_back({2, a, b, n, 0, 0, 0, 0, 0, off});
  }
  size_t subpix(const float* w, int Cout, int Cin) {
    const size_t off = reserve((int64_t)16 * Cout * Cin);
    jobs.push_back({3, w, nullptr, (int64_t)Cout * Cin * 9, Cout, Cin, 9, 0, 0, off});
    return off;
  }
  // the six U matrices [6][Cout][2 Cin] of the sub-pixel Winograd upsample kernel (conv_subwino.hip), from the torch weight
  size_t subwino(const float* w, int Cout, int Cin) {
    const size_t off = reserve((int64_t)12 * Cout * Cin);
    jobs.push_back({4, w, nullptr, (int64_t)Cout * Cin * 9, Cout, Cin, 9, 0, 0, off});
    return off;
  }
};

static __global__ void vec_add_kernel(const float* a, const float* b, float* out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}

// Run the pack jobs into `arena` (pk.size floats) on `st`.
inline int run_pack_jobs(const Packer& pk, float* arena, hipStream_t st) {
  for (auto& j : pk.jobs) {
    if (!j.src || (j.kind == 2 && !j.src2)) {
      set_error("null parameter pointer");
      return DM_ERR_ARG;
    }
    if (j.kind == 0) {
      DM_CHECK_HIP(hipMemcpyAsync(arena + j.dst, j.src, j.n * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else if (j.kind == 1) {
      const int rc = repack_conv(j.src, j.Cout, j.Cin, j.taps, arena + j.dst, j.ldw, j.col0, st);
      if (rc) return rc;
    } else if (j.kind == 3) {
      const int rc = repack_subpixel(j.src, j.Cout, j.Cin, arena + j.dst, st);
      if (rc) return rc;
    } else if (j.kind == 4) {
      const int rc = subwino_pack(j.src, j.Cout, j.Cin, arena + j.dst, st);
      if (rc) return rc;
    } else {
      hipLaunchKernelGGL(vec_add_kernel, dim3((unsigned)((j.n + 255) / 256)), dim3(256), 0, st, j.src, j.src2,
                         arena + j.dst, j.n);
      DM_LAUNCH_CHECK();
    }
  }
  return DM_OK;
}

}  // namespace dm
