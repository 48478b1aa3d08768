// fps_select.hip -- the one-workgroup select launches: fp32 with 1024 threads, fp64 with 512.
#include "fps_select.h"

namespace dvcp {

// fp32: 1024 threads (16 waves, 4 per SIMD, up to 16 points per lane): per-wave scan and update
// halve against 512 threads while the per-round decisions stay (tools/fps_lab: 16384 -> 10000
// 5.52 -> 5.07 ms, 10000 -> 10000 4.13 -> 3.30 ms on 16 clouds); 10 points per lane for N = 10000
// (the FE layers 2 and 3): no all-padding slots per lane.  fp64: 512 threads, from 4 points per
// lane (N >= 2048).
template <typename T>
int launch_fps_select(PointsView<T> v, int B, int N, int npoint, const int64_t* start, int64_t* out_idx, T* out_xyz,
                      hipStream_t st) {
  constexpr int NT = sizeof(T) == 4 ? kFpsSel1024 : kFpsThreads;
  auto launch = [&](auto p) {
    hipLaunchKernelGGL((fps_select_kernel<T, decltype(p)::value, false, NT>), dim3(B), dim3(NT), 0, st, v, N, npoint,
                       start, out_idx, out_xyz, nullptr);
    return launch_status("dvcp_fps");
  };
  if constexpr (sizeof(T) == 4)
    return fps_for_ppt<2, 4, 8, 10, 16>(ceil_div(N, NT), launch);
  else
    return fps_for_ppt<4, 8, 16>(ceil_div(N, NT), launch);
}
template int launch_fps_select<float>(PointsView<float>, int, int, int, const int64_t*, int64_t*, float*, hipStream_t);
template int launch_fps_select<double>(PointsView<double>, int, int, int, const int64_t*, int64_t*, double*,
                                       hipStream_t);

}  // namespace dvcp
