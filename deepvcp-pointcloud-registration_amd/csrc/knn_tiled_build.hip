// knn_tiled_build.hip -- the tiled kNN's workspace (knn_tiled.hip has the overview): the queries
// in curve order, and the references sorted along the same curve into kTile-point tiles with boxes.
#include "knn_tiled_common.h"

namespace dvcp {

// The queries' curve order is a counting sort spread over many workgroups (kQSortItems queries
// each; one workgroup per cloud took ~0.15 ms at C3's 85184 queries): bounding box by atomicMax
// on order keys, per-workgroup LDS histograms added into the cloud's bins, one scan per cloud,
// then a scatter by atomicAdd on the running positions (the order inside a cell is arbitrary:
// the permutation only shapes the query waves, never a result).
constexpr int kQSortItems = 8192;

template <typename CT>
__device__ __forceinline__ void qry_point(const PointsView<CT>& qry, int b, int i, float (&v)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) v[a] = static_cast<float>(qry.at(b, a, i));  // knn_cuda's .float()
}

__device__ __forceinline__ CurveGrid qry_grid(const uint32_t* qbox, int b) {
  float lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = float_unorder(~qbox[b * 8 + a]);
    hi[a] = float_unorder(qbox[b * 8 + 3 + a]);
  }
  return curve_grid(lo, hi);
}

template <typename CT>
__global__ __launch_bounds__(kBuildThreads) void knn_qbox_kernel(PointsView<CT> qry, int Q, uint32_t* qbox) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int i0 = blockIdx.x * kQSortItems, i1 = min(Q, i0 + kQSortItems);
  float lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = __builtin_huge_valf();
    hi[a] = -__builtin_huge_valf();
  }
  for (int i = i0 + threadIdx.x; i < i1; i += kBuildThreads) {
    float v[3];
    qry_point(qry, b, i, v);
#pragma unroll
    for (int a = 0; a < 3; ++a) {  // fminf / fmaxf: NaN coordinates are ignored, as block_bbox
      lo[a] = fminf(lo[a], v[a]);
      hi[a] = fmaxf(hi[a], v[a]);
    }
  }
  // wave, then workgroup reduction: six atomics per workgroup (one per wave serialised ~1400
  // atomics on the same 48 bytes per launch: 43 us)
  __shared__ uint32_t red[kBuildThreads / kWave][6];
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    for (int off = 32; off > 0; off >>= 1) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, kWave));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, kWave));
    }
    if (lane == 0) {
      red[wave][a] = ~float_order(lo[a]);
      red[wave][3 + a] = float_order(hi[a]);
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    uint32_t m = 0u;
    for (int w = 0; w < kBuildThreads / kWave; ++w) m = max(m, red[w][threadIdx.x]);
    atomicMax(&qbox[b * 8 + threadIdx.x], m);
  }
}

template <typename CT>
__global__ __launch_bounds__(kBuildThreads) void knn_qhist_kernel(PointsView<CT> qry, int Q, const uint32_t* qbox,
                                                                  uint32_t* qbins) {
  __shared__ uint32_t bins[kSortBins];
  const int b = blockIdx.y;
  const int i0 = blockIdx.x * kQSortItems, i1 = min(Q, i0 + kQSortItems);
  for (int i = threadIdx.x; i < kSortBins; i += kBuildThreads) bins[i] = 0u;
  __syncthreads();
  const CurveGrid g = qry_grid(qbox, b);
  for (int i = i0 + threadIdx.x; i < i1; i += kBuildThreads) {
    float v[3];
    qry_point(qry, b, i, v);
    atomicAdd(&bins[curve_cell(g, v)], 1u);
  }
  __syncthreads();
  uint32_t* gb = qbins + static_cast<int64_t>(b) * kSortBins;
  for (int i = threadIdx.x; i < kSortBins; i += kBuildThreads)
    if (bins[i] != 0u) atomicAdd(&gb[i], bins[i]);
}

__global__ __launch_bounds__(kBuildThreads) void knn_qscan_kernel(uint32_t* qbins) {
  __shared__ uint32_t bins[kSortBins];
  __shared__ uint32_t wsum[16];
  uint32_t* gb = qbins + static_cast<int64_t>(blockIdx.x) * kSortBins;
  for (int i = threadIdx.x; i < kSortBins; i += kBuildThreads) bins[i] = gb[i];
  __syncthreads();
  block_scan_bins(bins, wsum);
  __syncthreads();
  for (int i = threadIdx.x; i < kSortBins; i += kBuildThreads) gb[i] = bins[i];
}

template <typename CT>
__global__ __launch_bounds__(kBuildThreads) void knn_tiled_build_kernel(PointsView<CT> ref, int M, PointsView<CT> qry,
                                                                        int Q, TiledLayout L) {
  __shared__ uint32_t bins[kSortBins];
  __shared__ uint32_t boxk[kMaxTiles][6];  // order-preserving float keys: lo.xyz (min), hi.xyz (max)
  __shared__ uint32_t wsum[16];
  __shared__ float red[2][3][16];
  const int tid = threadIdx.x;
  // With B % 8 == 0 the linear block id is re-mapped so that every block of cloud b runs on XCD
  // b % 8 (blocks reach the XCDs round robin, speed only): the scatter's 16-byte rows of a cloud
  // then meet in one L2 and leave it as whole lines (round 5's 4-byte index scatter from all eight
  // XCDs wrote 34 MB per C3 launch for 2.7 MB of permutation).
  int b = blockIdx.y, bx = blockIdx.x;
  if ((gridDim.y & 7) == 0) {
    const int lin = static_cast<int>(blockIdx.y * gridDim.x + blockIdx.x);
    const int xo = lin & 7, slot = lin >> 3;
    b = xo + 8 * (slot / static_cast<int>(gridDim.x));
    bx = slot % static_cast<int>(gridDim.x);
  }
  if (bx > 0) {  // the queries' scatter into curve order (the scanned bins are running positions)
    const int i0 = (bx - 1) * kQSortItems, i1 = min(Q, i0 + kQSortItems);
    const CurveGrid g = qry_grid(L.qbox, b);
    uint32_t* gb = L.qbins + static_cast<int64_t>(b) * kSortBins;
    float4* qs = L.qsorted + static_cast<int64_t>(b) * Q;
    for (int i = i0 + tid; i < i1; i += kBuildThreads) {
      float v[3];
      qry_point(qry, b, i, v);
      qs[atomicAdd(&gb[curve_cell(g, v)], 1u)] = make_float4(v[0], v[1], v[2], __int_as_float(i));
    }
    return;
  }
  const int T = (M + kTile - 1) / kTile;
  float4* so = L.sorted + static_cast<int64_t>(b) * T * kTile;
  // knn_cuda casts both inputs with .float()
  auto get_ref = [&](int i, float (&v)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = static_cast<float>(ref.at(b, a, i));
  };
  for (int i = tid; i < T * 6; i += kBuildThreads) boxk[i / 6][i % 6] = (i % 6) < 3 ? 0xFFFFFFFFu : 0u;
  float lo[3], hi[3];
  block_bbox(M, get_ref, lo, hi, red);
  morton_sort(
      M, get_ref,
      [&](int pos, int i, const float (&v)[3]) {
        so[pos] = make_float4(v[0], v[1], v[2], __int_as_float(i));
        const int t = pos / kTile;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          atomicMin(&boxk[t][a], float_order(v[a]));
          atomicMax(&boxk[t][3 + a], float_order(v[a]));
        }
      },
      lo, hi, bins, wsum);
  for (int pos = M + tid; pos < T * kTile; pos += kBuildThreads)
    so[pos] = make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __int_as_float(0x7FFFFFFF));
  for (int t = tid; t < T; t += kBuildThreads) {
    float4* tb = L.tbox + (static_cast<int64_t>(b) * T + t) * 2;
    tb[0] = make_float4(float_unorder(boxk[t][0]), float_unorder(boxk[t][1]), float_unorder(boxk[t][2]), 0.f);
    tb[1] = make_float4(float_unorder(boxk[t][3]), float_unorder(boxk[t][4]), float_unorder(boxk[t][5]), 0.f);
  }
}

// queries: bounding box, cell counts, scan, then the scatter beside the reference build
template <typename CT>
static void launch_build(const void* ref, int64_t rb, int64_t rc, int64_t rn, int M, const void* qry, int64_t qb,
                         int64_t qc, int64_t qn, int Q, int B, const TiledLayout& L, hipStream_t st) {
  const dim3 qgrid(ceil_div(Q, kQSortItems), B), bgrid(1 + qgrid.x, B);
  const PointsView<CT> rv{static_cast<const CT*>(ref), rb, rc, rn}, qv{static_cast<const CT*>(qry), qb, qc, qn};
  hipLaunchKernelGGL((knn_qbox_kernel<CT>), qgrid, dim3(kBuildThreads), 0, st, qv, Q, L.qbox);
  hipLaunchKernelGGL((knn_qhist_kernel<CT>), qgrid, dim3(kBuildThreads), 0, st, qv, Q, L.qbox, L.qbins);
  hipLaunchKernelGGL(knn_qscan_kernel, dim3(B), dim3(kBuildThreads), 0, st, L.qbins);
  hipLaunchKernelGGL((knn_tiled_build_kernel<CT>), bgrid, dim3(kBuildThreads), 0, st, rv, M, qv, Q, L);
}

int knn_tiled_build(int dtype, const void* ref, int64_t rb, int64_t rc, int64_t rn, int M, const void* qry,
                    int64_t qb, int64_t qc, int64_t qn, int Q, int B, const TiledLayout& L, hipStream_t st) {
  if (hipMemsetAsync(L.qbins, 0, tiled_zeroed_bytes(B), st) != hipSuccess) {
    set_error("dvcp_knn_tiled: memset failed");
    return DVCP_EHIP;
  }
  if (dtype == DVCP_F32)
    launch_build<float>(ref, rb, rc, rn, M, qry, qb, qc, qn, Q, B, L, st);
  else
    launch_build<double>(ref, rb, rc, rn, M, qry, qb, qc, qn, Q, B, L, st);
  return launch_status("dvcp_knn_tiled(build)");
}

}  // namespace dvcp
