// points_pack4.hip -- dvcp_points_pack4: fp32 points as (x, y, z, 0) float4 rows, the layout
// (PointsView::rows4) the target DFE's collapsed kernel gathers with one 16-byte load per neighbour.
#include "common.h"

namespace dvcp {

// (x, y, z, 0) float4 rows of B clouds of M points (the layout dfe_tgt_mfma1_kernel's P4 reads)
__global__ void points_pack4_kernel(PointsView<float> pts, int M, int B, float4* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<int64_t>(B) * M) return;
  const int b = static_cast<int>(i / M);
  const int64_t n = i - static_cast<int64_t>(b) * M;
  out[i] = make_float4(pts.at(b, 0, n), pts.at(b, 1, n), pts.at(b, 2, n), 0.0f);
}

}  // namespace dvcp

extern "C" int dvcp_points_pack4(const float* xyz, int64_t sb, int64_t sc, int64_t sn, int M, int B, float* out,
                                 void* stream) {
  DVCP_REQUIRE(xyz && out, "dvcp_points_pack4: null pointer");
  DVCP_REQUIRE(M >= 0 && B >= 0, "dvcp_points_pack4: bad sizes");
  const int64_t total = static_cast<int64_t>(B) * M;
  if (total == 0) return DVCP_OK;
  DVCP_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "dvcp_points_pack4: out must be 16-byte aligned");
  hipLaunchKernelGGL(dvcp::points_pack4_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), dvcp::PointsView<float>{xyz, sb, sc, sn}, M, B,
                     reinterpret_cast<float4*>(out));
  return dvcp::launch_status("dvcp_points_pack4");
}
