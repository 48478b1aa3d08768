// voxelize.hip -- the candidate grid around each key point (voxelize.py:19-83).
#include "common.h"

namespace dvcp {

// torch.arange(start, end, s) values fp32(fma(s, i, start)) with start = (c - r) - s/2,
// end = c + r, all in fp64 (voxelize.py:62-64; torch's CPU arange kernel is compiled with fma
// contraction, visible at zero crossings); length ceil((end - start)/s) must equal G (cpg.py:29-30).
template <typename T>
__global__ void voxelize_kernel(PointsView<T> pts, int Kp, double r, double s, int G, float* __restrict__ cand,
                                int32_t* __restrict__ err) {
  const int C = G * G * G;
  const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (gid >= static_cast<int64_t>(Kp) * C) return;
  const int kp = static_cast<int>(gid / C), c = static_cast<int>(gid % C);
  const int ii[3] = {c / (G * G), (c / G) % G, c % G};
  float* o = cand + (static_cast<int64_t>(b) * Kp * C + gid) * 3;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double m = static_cast<double>(pts.at(b, a, kp));
    const double lo = m - r, hi = m + r;
    const double start = lo - s / 2;
    if (err && c == 0 && static_cast<int>(ceil((hi - start) / s)) != G) *err = 1;
    o[a] = static_cast<float>(__fma_rn(s, static_cast<double>(ii[a]), start));
  }
}

}  // namespace dvcp

extern "C" int dvcp_voxelize(int dtype, const void* pts, int64_t pb, int64_t pc, int64_t pn, int B, int Kp,
                             double r, double s, int G, float* cand, int32_t* err, void* stream) {
  DVCP_REQUIRE(pts && cand, "dvcp_voxelize: null pointer");
  DVCP_REQUIRE(G > 0 && s > 0 && B <= 65535, "dvcp_voxelize: bad arguments");
  if (B == 0 || Kp == 0) return DVCP_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t total = static_cast<int64_t>(Kp) * G * G * G;
  dim3 grid(dvcp::ceil_div(total, 256), B);
  if (dtype == DVCP_F32)
    hipLaunchKernelGGL((dvcp::voxelize_kernel<float>), grid, dim3(256), 0, st,
                       dvcp::PointsView<float>{static_cast<const float*>(pts), pb, pc, pn}, Kp, r, s, G, cand, err);
  else if (dtype == DVCP_F64)
    hipLaunchKernelGGL((dvcp::voxelize_kernel<double>), grid, dim3(256), 0, st,
                       dvcp::PointsView<double>{static_cast<const double*>(pts), pb, pc, pn}, Kp, r, s, G, cand, err);
  else {
    dvcp::set_error("dvcp_voxelize: bad dtype %d", dtype);
    return DVCP_EINVAL;
  }
  return dvcp::launch_status("dvcp_voxelize");
}
