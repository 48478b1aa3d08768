// bq_build.hip -- the fp32 ball query's workspace build (bq_common.h lists the units): the packed
// (x, y, z, |p|^2) rows, and for the tiled scan the Hilbert-sorted 64-point tiles with their boxes
// and the centres' Hilbert permutation.
#include "bq_common.h"
#include "morton.h"

namespace dvcp {

__global__ void bq_pack_kernel(PointsView<float> pts, int N, float4* __restrict__ packed) {
  const int b = blockIdx.y;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int np = bq_padded_n(N);
  if (n >= np) return;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (n < N) {
    const float x = pts.at(b, 0, n), y = pts.at(b, 1, n), z = pts.at(b, 2, n);
    v = make_float4(x, y, z, sumsq3(x, y, z));
  }
  packed[static_cast<int64_t>(b) * np + n] = v;
}

// Two workgroups per cloud: packed rows and point tiles with boxes; the centres' Hilbert permutation.
__global__ __launch_bounds__(kBuildThreads) void bq_build_kernel(PointsView<float> pts, int N, PointsView<float> ctr,
                                                                 int S, BqLayout L, int tiled) {
  __shared__ uint32_t bins[kSortBins];
  __shared__ uint32_t boxk[kBqMaxTiles][6];  // float_order keys: lo.xyz (min), hi.xyz (max)
  __shared__ uint32_t wsum[16];
  __shared__ float red[2][3][16];
  const int b = blockIdx.y, tid = threadIdx.x;
  auto get_ctr = [&](int i, float (&v)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = ctr.at(b, a, i);
  };
  float lo[3], hi[3];
  if (blockIdx.x == 1) {  // the centres' curve order, beside the point work of block 0
    block_bbox(S, get_ctr, lo, hi, red);
    int32_t* cp = L.cperm + static_cast<int64_t>(b) * S;
    morton_sort(
        S, get_ctr, [&](int pos, int i, const float (&)[3]) { cp[pos] = i; }, lo, hi, bins, wsum);
    return;
  }
  const int np = bq_padded_n(N);
  float4* pk = L.packed + static_cast<int64_t>(b) * np;
  for (int i = tid; i < np; i += kBuildThreads) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < N) {
      const float x = pts.at(b, 0, i), y = pts.at(b, 1, i), z = pts.at(b, 2, i);
      v = make_float4(x, y, z, sumsq3(x, y, z));
    }
    pk[i] = v;
  }
  if (!tiled) return;
  const int T = (N + kBqTile - 1) / kBqTile;
  float4* so = L.sorted + static_cast<int64_t>(b) * T * kBqTile;
  for (int i = tid; i < T * 6; i += kBuildThreads) boxk[i / 6][i % 6] = (i % 6) < 3 ? 0xFFFFFFFFu : 0u;
  auto get_pt = [&](int i, float (&v)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = pts.at(b, a, i);
  };
  block_bbox(N, get_pt, lo, hi, red);
  morton_sort(
      N, get_pt,
      [&](int pos, int i, const float (&v)[3]) {
        so[pos] = make_float4(v[0], v[1], v[2], __int_as_float(i));
        const int t = pos / kBqTile;
        // a non-finite coordinate can pass the reference's test against any centre (NaN d2
        // is not > r^2), so its tile must never be pruned: give it the whole space
        const bool fin = __builtin_isfinite(v[0]) && __builtin_isfinite(v[1]) && __builtin_isfinite(v[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          atomicMin(&boxk[t][a], float_order(fin ? v[a] : -__builtin_huge_valf()));
          atomicMax(&boxk[t][3 + a], float_order(fin ? v[a] : __builtin_huge_valf()));
        }
      },
      lo, hi, bins, wsum);
  for (int pos = N + tid; pos < T * kBqTile; pos += kBuildThreads)
    so[pos] = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __int_as_float(0x7FFFFFFF));
  for (int t = tid; t < T; t += kBuildThreads) {
    float4* tb = L.tbox + (static_cast<int64_t>(b) * T + t) * 2;
    tb[0] = make_float4(float_unorder(boxk[t][0]), float_unorder(boxk[t][1]), float_unorder(boxk[t][2]), 0.f);
    tb[1] = make_float4(float_unorder(boxk[t][3]), float_unorder(boxk[t][4]), float_unorder(boxk[t][5]), 0.f);
  }
}

int bq_build_launch(PointsView<float> pts, int N, PointsView<float> ctr, int S, int B, const BqLayout& L, int tiled,
                    hipStream_t st) {
  hipLaunchKernelGGL(bq_build_kernel, dim3(tiled ? 2 : 1, B), dim3(kBuildThreads), 0, st, pts, N, ctr, S, L, tiled);
  return launch_status("dvcp_ball_query(build)");
}

}  // namespace dvcp
