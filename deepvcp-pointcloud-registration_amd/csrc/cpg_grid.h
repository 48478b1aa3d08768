// cpg_grid.h -- index math of the CPG candidate grid (G^3 voxels), shared by the forward (cpg.hip,
// G <= 11; cpg_tiled.hip, G <= 32) and the backward (cpg_bwd.hip).
#pragma once
#include "common.h"

namespace dvcp {

// x / d for 0 <= x < 2^16 and 1 <= d <= 2^11 as one mul_hi: m = ceil(2^32 / d) overestimates
// 1/d by less than 2^-32, so x*m/2^32 exceeds x/d by less than 2^-16, while the fractional part
// of x/d is at most 1 - 1/d <= 1 - 2^-11: the floor is exact.  (Index math of an 11^3 grid: the
// generic 32-bit division costs ~25 VALU instructions and dominated this kernel's VALU count.)
// The range covers a voxel index g < 32^3 = 2^15 over d = G or G^2 <= 2^10, so g -> (z, y, x) up to
// G = 32; it does NOT cover the Q11 element index l = 32 g + f' (< 2^20 at G = 32), which is
// never divided this way.  d = 1 gives m = 0 (2^32 does not fit): every quotient is 0, right only
// for x = 0 -- a 1-cell axis, whose only index is 0.
struct FastDiv {
  uint32_t m, d;
  __device__ __forceinline__ explicit FastDiv(uint32_t dd)
      : m(static_cast<uint32_t>((0x100000000ull + dd - 1) / dd)), d(dd) {}
  // m given: magic(dd), formed once on the host for a divisor the whole launch shares
  __device__ __forceinline__ FastDiv(uint32_t mm, uint32_t dd) : m(mm), d(dd) {}
  __host__ __device__ static uint32_t magic(uint32_t dd) {
    return static_cast<uint32_t>((0x100000000ull + dd - 1) / dd);
  }
  __device__ __forceinline__ uint32_t div(uint32_t x) const { return __umulhi(x, m); }
  __device__ __forceinline__ uint32_t mod(uint32_t x) const { return x - div(x) * d; }
};

// haloed cell of voxel g = (gz*G + gy)*G + gx in the (G+2)^3 volume
__device__ __forceinline__ int cpg_halo(int g, const FastDiv& dG, const FastDiv& dGG, int PG, int PGG) {
  const uint32_t z = dGG.div(g), r = g - z * dGG.d;
  const uint32_t y = dG.div(r), x = r - y * dG.d;
  return static_cast<int>((z + 1) * PGG + (y + 1) * PG + (x + 1));
}

}  // namespace dvcp
