// fps.hip -- farthest point sampling (replaces pointnet2_utils.py:63-84): the dispatch by cloud
// size and the dvcp_fps* entry points.
//
// Semantics (bit-exact with the reference): running minimum stored in fp32 for both coordinate
// dtypes (:74, :82), distance ((dx*dx + dy*dy) + dz*dz) in the coordinate dtype (:80), strict
// '<' update (:81), argmax = largest running minimum, ties to the LOWEST original index (:83).
//
// FPS is a serial chain of `npoint` dependent argmax steps per cloud.  Kernels by cloud size:
//   * N < 2048: fps_kernel, one centre per step (one workgroup of 512 threads, 2 or 4 points per
//     lane, per-step DPP argmax + one barrier, wave-box pruning) -- fps_step.hip;
//   * 2048 <= N <= 16384 (8192 fp64): fps_select_kernel, which certifies a whole prefix of the
//     serial chain per round (~27 centres on C3 clouds) from a threshold-selected candidate list:
//     fp32 1024 threads with 2, 4, 8, 10 or 16 points per lane, fp64 512 threads with 4, 8 or 16
//     -- fps_select.hip, the round itself in fps_select.h;
//   * larger, fp32 up to 65536, through dvcp_fps_parts: the split select (fps_part_kernel: 8
//     workgroups per cloud run the select rounds together, one candidate-list exchange per round;
//     opt-in from 2048: 2 workgroups reach 16384 points, 4 reach 32768, 8 reach 65536)
//     -- fps_part.hip;
//   * else fps_split_kernel (S workgroups per cloud exchanging one key per step), then
//     fps_dense_kernel -- fps_step.hip.
// dvcp_fps_pair (two chained full-permutation layers in one launch, opt-in) is fps_pair.hip.
// Every kernel but the dense one keeps each cloud's coordinates and running minima in VGPRs
// (Morton-sorted for the first three), so the loop touches no global memory except the output
// stores and the split kernels' exchanges.
#include "fps_common.h"

namespace dvcp {

// Workgroups per cloud of the select rounds when the caller does not choose (dvcp_fps_parts,
// parts 0): 8 above 16384 points, else one, unless DVCP_FPS_PARTS asks for the split select (2, 4
// or 8).  The split select shortens a lone batch's chain but costs CU time: S full-CU workgroups
// per cloud for 1 / 1.3 / 1.6 the time at S = 2 / 4 / 8 (C3), so with the bench's ten batches in
// flight the one-workgroup kernel gives the most pairs/s (round 6: 2300 against 1630 at S = 4 and
// 1310 at S = 8).  Above 16384 points the alternative is the per-step split kernel, slower still.
static int fps_parts(int N) {
  static const int forced = [] {
    const char* s = getenv("DVCP_FPS_PARTS");
    return s && *s ? atoi(s) : 0;
  }();
  if (forced == 1 || forced == 2 || forced == 4 || forced == 8) return forced;
  // above the one-workgroup kernel's 16384 points: 8 workgroups of up to 8192 (C5's layer 1,
  // 65536 -> 10000: 9.65 ms per launch with the per-step split kernel, 4.4 ms split select)
  return N > fps_select_max_n<float>() ? 8 : 1;
}

// S: workgroups per cloud of the select rounds (fp32 with a sized workspace; 1: one).
template <typename T>
static int launch_fps(PointsView<T> v, int B, int N, int npoint, const int64_t* start, int64_t* out_idx, T* out_xyz,
                      float* ws, int64_t ws_bytes, int32_t* err, int S, hipStream_t st) {
  if (N < kFpsBatchedMinN) return launch_fps_step<T>(v, B, N, npoint, start, out_idx, out_xyz, st);
  if constexpr (sizeof(T) == 4) {
    if (S > 1 && npoint > 1) {
      const int e = launch_fps_part(v, B, N, npoint, start, out_idx, out_xyz, ws, ws_bytes, err, S, st);
      if (e != 1) return e;  // (1: this (N, S) has no split select; the kernels below take it)
    }
  }
  if (N <= fps_select_max_n<T>()) return launch_fps_select<T>(v, B, N, npoint, start, out_idx, out_xyz, st);
  if (!ws) {
    set_error("dvcp_fps: N=%d needs the split/dense path and its B x N fp32 workspace (dvcp_fps_ws)", N);
    return DVCP_EINVAL;
  }
  return launch_fps_large<T>(v, B, N, npoint, start, out_idx, out_xyz, ws, err, st);
}

static int launch_fps_dtype(int dtype, const void* xyz, int64_t sb, int64_t sc, int64_t sn, int B, int N, int npoint,
                            const int64_t* start, int64_t* out_idx, void* out_xyz, float* ws, int64_t ws_bytes,
                            int32_t* err, int S, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == DVCP_F32)
    return launch_fps<float>(PointsView<float>{static_cast<const float*>(xyz), sb, sc, sn}, B, N, npoint, start,
                             out_idx, static_cast<float*>(out_xyz), ws, ws_bytes, err, S, st);
  if (dtype == DVCP_F64)
    return launch_fps<double>(PointsView<double>{static_cast<const double*>(xyz), sb, sc, sn}, B, N, npoint, start,
                              out_idx, static_cast<double*>(out_xyz), ws, ws_bytes, err, S, st);
  set_error("dvcp_fps: bad dtype %d", dtype);
  return DVCP_EINVAL;
}

}  // namespace dvcp

// ws (B x N fp32, or null up to 65535 points) serves the per-step split and dense kernels only: it
// is smaller than the split select's workspace, which is reached through dvcp_fps_parts.
extern "C" int dvcp_fps_ws(int dtype, const void* xyz, int64_t sb, int64_t sc, int64_t sn, int B, int N, int npoint,
                           const int64_t* start, int64_t* out_idx, void* out_xyz, float* ws, int32_t* err,
                           void* stream) {
  DVCP_REQUIRE(xyz && start && out_idx, "dvcp_fps: null pointer");
  DVCP_REQUIRE(B >= 0 && N > 0 && npoint >= 0, "dvcp_fps: bad sizes B=%d N=%d npoint=%d", B, N, npoint);
  DVCP_REQUIRE(N <= 65535 || ws, "dvcp_fps: N=%d needs a workspace", N);
  if (B == 0 || npoint == 0) return DVCP_OK;
  return dvcp::launch_fps_dtype(dtype, xyz, sb, sc, sn, B, N, npoint, start, out_idx, out_xyz, ws, 0, err, 1, stream);
}

// Workspace bytes dvcp_fps_parts needs for B clouds of N points (any parts).
extern "C" int64_t dvcp_fps_workspace_bytes(int B, int N) {
  return B < 0 || N < 0 ? -1 : dvcp::fps_workspace_bytes(B, N);
}

// dvcp_fps_ws with a sized workspace and the split select's workgroups per cloud: parts 0 = the
// library's choice (fps_parts), 1 = the one-workgroup select kernel (the per-step split kernel
// above 16384 points), 2 / 4 / 8 = the split select (fp32, from 2048 points up to 16384 / 32768 /
// 65536; beyond, the per-step split kernel).  ws: ws_bytes >= dvcp_fps_workspace_bytes(B, N) bytes
// (8-aligned).
extern "C" int dvcp_fps_parts(int dtype, const void* xyz, int64_t sb, int64_t sc, int64_t sn, int B, int N,
                              int npoint, const int64_t* start, int64_t* out_idx, void* out_xyz, void* ws,
                              int64_t ws_bytes, int32_t* err, int parts, void* stream) {
  DVCP_REQUIRE(xyz && start && out_idx && ws, "dvcp_fps_parts: null pointer");
  DVCP_REQUIRE(B >= 0 && N > 0 && npoint >= 0, "dvcp_fps_parts: bad sizes B=%d N=%d npoint=%d", B, N, npoint);
  DVCP_REQUIRE(parts == 0 || parts == 1 || parts == 2 || parts == 4 || parts == 8,
               "dvcp_fps_parts: parts=%d not 0, 1, 2, 4 or 8", parts);
  DVCP_REQUIRE(ws_bytes >= dvcp::fps_workspace_bytes(B, N) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
               "dvcp_fps_parts: workspace of %lld bytes (need %lld, 8-aligned)", static_cast<long long>(ws_bytes),
               static_cast<long long>(dvcp::fps_workspace_bytes(B, N)));
  if (B == 0 || npoint == 0) return DVCP_OK;
  return dvcp::launch_fps_dtype(dtype, xyz, sb, sc, sn, B, N, npoint, start, out_idx, out_xyz,
                                static_cast<float*>(ws), ws_bytes, err, parts > 0 ? parts : dvcp::fps_parts(N), stream);
}

extern "C" int dvcp_fps(int dtype, const void* xyz, int64_t sb, int64_t sc, int64_t sn, int B, int N, int npoint,
                        const int64_t* start, int64_t* out_idx, void* out_xyz, void* stream) {
  return dvcp_fps_ws(dtype, xyz, sb, sc, sn, B, N, npoint, start, out_idx, out_xyz, nullptr, nullptr, stream);
}
