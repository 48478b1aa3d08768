// fp_common.h -- what the feature-propagation forward (csrc/paper.hip, fp_kernel) and its backward
// (csrc/paper_fe_bwd.hip, fp_bwd_kernel) share: the tile geometry, the layer table and the 3-NN
// keys.  The backward recomputes the forward's neighbours and weights, so both must order
// candidates by the same key.
#pragma once
#include "common.h"

namespace dvcp {

constexpr int kFpRows = 32;      // points per workgroup
constexpr int kFpThreads = 256;  // 8 threads per point in the 3-NN scan
constexpr int kFpTile = 1024;    // xyz2 points per LDS tile
constexpr int kFpMaxC = 128;     // widest row / layer input
constexpr int kFpMaxCo = 64;     // widest layer output
constexpr int kFpMaxL = 4;

struct FpLayers {
  int L;
  int ch[kFpMaxL + 1];
  int relu[kFpMaxL];
};

__device__ __forceinline__ uint64_t fp_key(float d2, int idx) {
  return (static_cast<uint64_t>(float_order(d2)) << 32) | static_cast<uint32_t>(idx);
}
__device__ __forceinline__ float fp_key_d2(uint64_t k) {  // inverse of float_order
  const uint32_t u = static_cast<uint32_t>(k >> 32);
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
__device__ __forceinline__ void top3_insert(uint64_t (&k)[3], uint64_t v) {
  if (v < k[2]) {
    if (v < k[1]) {
      k[2] = k[1];
      if (v < k[0]) {
        k[1] = k[0];
        k[0] = v;
      } else {
        k[1] = v;
      }
    } else {
      k[2] = v;
    }
  }
}

}  // namespace dvcp
