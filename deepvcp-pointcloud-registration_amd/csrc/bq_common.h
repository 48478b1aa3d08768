// bq_common.h -- what the units of the fp32 ball query share (ball_query.hip has the overview): the
// constants, the workspace layout and the launchers each kernel unit exports to the dispatch.
//   bq_build.hip    packed rows, Hilbert-sorted point tiles with boxes, the centres' permutation
//   bq_scan.hip     the wave scan (any N) and the tiled scan (N <= 65536)
//   ball_query.hip  the brute-force kernel, square_distance, the dispatch, the entry points
#pragma once
#include "common.h"

namespace dvcp {

// Rows are padded to a multiple of 16 points (zeros) so every 16-point chunk of the wave scan is
// one unconditional scalar burst; the padding never hits because the loop tests n < N.
__host__ __device__ constexpr int bq_padded_n(int N) { return (N + 15) & ~15; }

constexpr int kBqTile = 64;
constexpr int kBqMaxTiles = 1024;             // tiled path: N <= 65536
constexpr int kBqSmallTiles = 256;            // N <= 16384: the small-bitmap instantiation (occupancy)
constexpr int kBqCap = 256;                   // candidate points staged in LDS per round

struct BqLayout {
  float4* packed;   // B x Npad: x, y, z, |p|^2 in original order (zero padding)
  float4* sorted;   // B x T*64: x, y, z, original index bits (padding: NaN, 0x7FFFFFFF)
  float4* tbox;     // B x T x 2: lo.xyz, hi.xyz (non-finite member: the whole space)
  int32_t* cperm;   // B x S: centre index by Hilbert position
};

inline int64_t bq_align(int64_t x) { return (x + 255) & ~int64_t(255); }

inline BqLayout bq_layout(void* ws, int B, int N, int S) {
  const int64_t T = ceil_div(N, kBqTile);
  char* p = static_cast<char*>(ws);
  BqLayout L;
  L.packed = reinterpret_cast<float4*>(p);
  p += bq_align(16 * int64_t(B) * bq_padded_n(N));
  L.sorted = reinterpret_cast<float4*>(p);
  p += bq_align(16 * int64_t(B) * T * kBqTile);
  L.tbox = reinterpret_cast<float4*>(p);
  p += bq_align(32 * int64_t(B) * T);
  L.cperm = reinterpret_cast<int32_t*>(p);
  return L;
}

inline int64_t bq_workspace_bytes(int B, int N, int S) {
  const int64_t T = ceil_div(N, kBqTile);
  return bq_align(16 * int64_t(B) * bq_padded_n(N)) + bq_align(16 * int64_t(B) * T * kBqTile) +
         bq_align(32 * int64_t(B) * T) + bq_align(4 * int64_t(B) * S);
}

// The launchers.  Each enqueues on st and returns launch_status(); launch_bq has checked the sizes.
// tiled != 0 (N <= kBqMaxTiles * kBqTile): the build also sorts tiles and centres, and the scan is
// the tiled one.
int bq_build_launch(PointsView<float> pts, int N, PointsView<float> ctr, int S, int B, const BqLayout& L, int tiled,
                    hipStream_t st);
int bq_scan_launch(const BqLayout& L, int tiled, int N, PointsView<float> ctr, int S, int B, float r2, int nsample,
                   int32_t* count, int32_t* list, int64_t* padded, hipStream_t st);

}  // namespace dvcp
