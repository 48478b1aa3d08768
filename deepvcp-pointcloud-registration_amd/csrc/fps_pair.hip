// fps_pair.hip -- the paired launch of two full-permutation FPS layers (FpsPairArgs in
// fps_select.h): fps_pair_kernel, the remap of layer 3's indices, the gated recomputation.
#include "fps_select.h"

namespace dvcp {

// grid B: layer 3's indices (into layer 2's points) -> layer 2's pick numbers (its FPS order), for
// the clouds without a flag (layer 2 then picked every point once).  A tie group (a run of entries
// marked by bit 62 after its first) is put in ascending pick-number order -- the reference's
// lowest-index-first argmax among equal values -- with its centres' coordinates.
constexpr int kFpsRemapThreads = 1024;
__global__ __launch_bounds__(kFpsRemapThreads) void fps_pair_remap_kernel(const uint32_t* __restrict__ inv2,
                                                                          int64_t* __restrict__ idx3,
                                                                          float* __restrict__ xyz3,
                                                                          const int32_t* __restrict__ flag, int N) {
  const int b = blockIdx.x;
  if (flag[b] != 0) return;
  constexpr int64_t kMark = int64_t(1) << 62;
  const uint32_t* inv = inv2 + static_cast<int64_t>(b) * N;
  int64_t* i3 = idx3 + static_cast<int64_t>(b) * N;
  float* x3 = xyz3 + static_cast<int64_t>(b) * 3 * N;
  auto key_of = [&](int64_t v) -> int64_t {
    const int64_t n = v & ~kMark;
    return (n >= 0 && n < N) ? static_cast<int64_t>(inv[n] & 0x7FFFFFFFu) : 0;
  };
  __shared__ uint32_t marks[16384 / 32];  // the marks as written, before any entry is rewritten
  for (int w = threadIdx.x; w < (N + 31) / 32; w += kFpsRemapThreads) marks[w] = 0u;
  __syncthreads();
  for (int j = threadIdx.x; j < N; j += kFpsRemapThreads)
    if (i3[j] & kMark) atomicOr(&marks[j >> 5], 1u << (j & 31));
  __syncthreads();
  auto marked = [&](int j) { return (marks[j >> 5] >> (j & 31)) & 1u; };
  for (int j = threadIdx.x; j < N; j += kFpsRemapThreads) {
    if (marked(j)) continue;  // written by its group's first entry
    const int64_t v = i3[j];
    int e = j;
    while (e + 1 < N && marked(e + 1)) ++e;
    if (e == j) {
      i3[j] = key_of(v);
      continue;
    }
    // group j..e (at most kSelAccept entries): selection sort by pick number, in place
    for (int p = j; p <= e; ++p) {
      int best = p;
      int64_t kb = key_of(i3[p]);
      for (int q = p + 1; q <= e; ++q) {
        const int64_t kq = key_of(i3[q]);
        if (kq < kb) {
          kb = kq;
          best = q;
        }
      }
      const int64_t vp = i3[p];
      i3[best] = vp;  // (an unresolved member: its raw index)
      i3[p] = kb;     // resolved
      for (int a = 0; a < 3; ++a) {
        const float t = x3[a * N + best];
        x3[a * N + best] = x3[a * N + p];
        x3[a * N + p] = t;
      }
    }
  }
}

// Paired launch of two full-permutation fp32 layers (see FpsPairArgs); N in the select kernel's
// 1024-thread range.
static int launch_fps_pair(PointsView<float> v, int B, int N, const int64_t* start2, const int64_t* start3,
                           int64_t* idx2, float* xyz2, int64_t* idx3, float* xyz3, uint32_t* ws, hipStream_t st) {
  // ws: ticket | slot[B] | flag[B] | inv2[B x N], all zero before the launch
  FpsPairArgs<float> pa{ws, ws + 1, reinterpret_cast<int32_t*>(ws + 1 + B), ws + 1 + 2 * static_cast<int64_t>(B),
                        start3, idx3, xyz3};
  if (hipMemsetAsync(ws, 0, sizeof(uint32_t) * (1 + 2 * static_cast<size_t>(B) + static_cast<size_t>(B) * N), st) !=
      hipSuccess)
    return launch_status("dvcp_fps_pair(memset)");
  const PointsView<float> v2{xyz2, 3 * static_cast<int64_t>(N), N, 1};
  const int e = fps_for_ppt<2, 4, 8, 10, 16>(ceil_div(N, kFpsSel1024), [&](auto p) {
    constexpr int P = decltype(p)::value;
    hipLaunchKernelGGL((fps_pair_kernel<float, P>), dim3(2 * B), dim3(kFpsSel1024), 0, st, v, N, start2, idx2, xyz2,
                       pa);
    if (int e = launch_status("dvcp_fps_pair")) return e;
    hipLaunchKernelGGL(fps_pair_remap_kernel, dim3(B), dim3(kFpsRemapThreads), 0, st, pa.inv2, idx3, xyz3, pa.flag, N);
    if (int e = launch_status("dvcp_fps_pair(remap)")) return e;
    hipLaunchKernelGGL((fps_select_gated_kernel<float, P>), dim3(B), dim3(kFpsSel1024), 0, st, v2, N, start3, idx3,
                       xyz3, pa);
    return launch_status("dvcp_fps_pair(gated)");
  });
  if (e != 1) return e;
  set_error("dvcp_fps_pair: N=%d out of range", N);
  return DVCP_EINVAL;
}

}  // namespace dvcp

// Two chained full-permutation FPS layers in one launch (FE layers 2 and 3): bit-identical to
//   dvcp_fps(xyz, N, start2) -> (idx2, xyz2);  dvcp_fps(xyz2, N, start3) -> (idx3, xyz3).
// fp32, 2048 <= N <= 16384; ws: dvcp_fps_pair_workspace_bytes(B, N) bytes, 4-byte aligned.
extern "C" int64_t dvcp_fps_pair_workspace_bytes(int B, int N) {
  return B < 0 || N < 0 ? -1 : 4 * (1 + 2 * static_cast<int64_t>(B) + static_cast<int64_t>(B) * N);
}

extern "C" int dvcp_fps_pair(int dtype, const void* xyz, int64_t sb, int64_t sc, int64_t sn, int B, int N,
                             const int64_t* start2, const int64_t* start3, int64_t* idx2, void* xyz2, int64_t* idx3,
                             void* xyz3, void* ws, void* stream) {
  DVCP_REQUIRE(xyz && start2 && start3 && idx2 && xyz2 && idx3 && xyz3 && ws, "dvcp_fps_pair: null pointer");
  DVCP_REQUIRE(dtype == DVCP_F32, "dvcp_fps_pair: fp32 only (dtype %d)", dtype);
  DVCP_REQUIRE(B >= 0 && B <= 32767 && N >= dvcp::kFpsBatchedMinN && N <= dvcp::fps_select_max_n<float>(),
               "dvcp_fps_pair: bad sizes B=%d N=%d", B, N);
  DVCP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "dvcp_fps_pair: workspace not 4-byte aligned");
  if (B == 0) return DVCP_OK;
  return dvcp::launch_fps_pair(dvcp::PointsView<float>{static_cast<const float*>(xyz), sb, sc, sn}, B, N, start2,
                               start3, idx2, static_cast<float*>(xyz2), idx3, static_cast<float*>(xyz3),
                               static_cast<uint32_t*>(ws), static_cast<hipStream_t>(stream));
}
