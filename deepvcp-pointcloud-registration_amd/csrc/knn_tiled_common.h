// knn_tiled_common.h -- what the units of the tiled kNN share (knn_tiled.hip has the overview):
// the workspace layout, the box bounds at full and half precision, the wave reductions, and the
// launchers each kernel unit exports to the dispatch.
//   knn_tiled_build.hip  query sort and reference tile build kernels, knn_tiled_build()
//   knn_tiled_insert.hip the per-candidate insertion kernel (dvcp_knn_tiled's k <= 16, and every
//                        k of dvcp_knn_tiled_insert), knn_insert_launch()
//   knn_tiled_sel.hip    the k = 17..32 kernel (buffered selection), its tile order and the order
//                        probe, knn_sel_launch() / knn_order_probe_launch()
//   knn_tiled.hip        workspace size, dispatch, the extern "C" entry points
#pragma once
#include <type_traits>

#include "common.h"
#include "morton.h"

namespace dvcp {

constexpr int kTile = 16;             // reference points per tile (finer boxes prune and order better)
constexpr int kMaxTiles = 1024;       // per cloud: M <= 16384
constexpr uint32_t kTileIdBits = 0x3FFu;  // tile id in the low bits of a sort key (kMaxTiles - 1)
constexpr int kTiledThreads = 256;    // 4 independent waves per workgroup

struct TiledLayout {
  float4* sorted;  // B x T*kTile: x, y, z, original index bits (padding: NaN, index 0x7FFFFFFF)
  float4* tbox;    // B x T x 2: {lo.xyz, _}, {hi.xyz, _}
  float4* qsorted;  // B x Q: the queries in curve order as (x, y, z, original index bits), fp32
  uint32_t* qbins;  // B x kSortBins: the queries' cell counts, then their running positions
  uint32_t* qbox;   // B x 8: ~float_order(lo.xyz), float_order(hi.xyz) of the queries (atomicMax)
};

inline int64_t align256(int64_t x) { return (x + 255) & ~int64_t(255); }

inline TiledLayout tiled_layout(void* ws, int B, int M, int Q) {
  const int64_t T = ceil_div(M, kTile);
  char* p = static_cast<char*>(ws);
  TiledLayout L;
  L.sorted = reinterpret_cast<float4*>(p);
  p += align256(16 * int64_t(B) * T * kTile);
  L.tbox = reinterpret_cast<float4*>(p);
  p += align256(32 * int64_t(B) * T);
  L.qsorted = reinterpret_cast<float4*>(p);
  p += align256(16 * int64_t(B) * Q);
  L.qbins = reinterpret_cast<uint32_t*>(p);  // qbins and qbox are one zeroed range
  L.qbox = L.qbins + int64_t(B) * kSortBins;
  return L;
}
inline int64_t tiled_zeroed_bytes(int B) { return 4 * int64_t(B) * (kSortBins + 8); }

// The launchers.  Each enqueues on st and returns launch_status(); the caller has checked the sizes
// (0 < k <= 32, M <= kMaxTiles * kTile, B <= 65535, dtype F32 or F64).
// The reference tiles and the queries' curve order into the workspace (every caller's first step).
int knn_tiled_build(int dtype, const void* ref, int64_t rb, int64_t rc, int64_t rn, int M, const void* qry,
                    int64_t qb, int64_t qc, int64_t qn, int Q, int B, const TiledLayout& L, hipStream_t st);
int knn_insert_launch(const TiledLayout& L, int M, int Q, int B, int k, float* dist, int32_t* idx, int64_t* idx64,
                      hipStream_t st);  // k <= 32
int knn_sel_launch(const TiledLayout& L, int M, int Q, int B, int k, float* dist, int32_t* idx, int64_t* idx64,
                   hipStream_t st);  // k = 17..32
int knn_order_probe_launch(const TiledLayout& L, int M, int Q, int B, int32_t* info, int32_t* order, float* lb,
                           int32_t* bucket, hipStream_t st);

// The kernels that hold one key or bound per tile in registers are instantiated for R registers of
// 64 tiles each: f(std::integral_constant<int, R>) for the smallest R of 1, 2, 4, 8, 16 that holds
// T <= kMaxTiles tiles.
template <typename F>
int knn_for_tile_regs(int T, F&& f) {
  if (T <= 64) return f(std::integral_constant<int, 1>());
  if (T <= 128) return f(std::integral_constant<int, 2>());
  if (T <= 256) return f(std::integral_constant<int, 4>());
  if (T <= 512) return f(std::integral_constant<int, 8>());
  return f(std::integral_constant<int, 16>());
}

// Lower bound of the computed d2 between a point in box [a_lo, a_hi] and a point in box
// [b_lo, b_hi] (per axis gap fl(b_lo - a_hi) or fl(a_lo - b_hi), then the d2 formula).
__device__ __forceinline__ float box_box_lb2(float alx, float aly, float alz, float ahx, float ahy, float ahz,
                                             float blx, float bly, float blz, float bhx, float bhy, float bhz) {
  const float gx = fmaxf(fmaxf(blx - ahx, alx - bhx), 0.0f);
  const float gy = fmaxf(fmaxf(bly - ahy, aly - bhy), 0.0f);
  const float gz = fmaxf(fmaxf(blz - ahz, alz - bhz), 0.0f);
  return (gx * gx + gy * gy) + gz * gz;
}

// Tile boxes at half precision, rounded outward (largest half <= lo, smallest half >= hi; NaN
// and +-inf pass through): 8 bytes per corner pair instead of 32, and box_box_lb2 over the widened
// box is still a lower bound of every computed d2 in the tile (the gaps are monotone in the box).
__device__ __forceinline__ uint32_t half_down(float x) {
  const _Float16 h = static_cast<_Float16>(x);
  uint32_t hb = __builtin_bit_cast(uint16_t, h);
  if (static_cast<float>(h) > x) hb = (hb & 0x8000u) ? hb + 1u : (hb == 0u ? 0x8001u : hb - 1u);
  return hb;
}
__device__ __forceinline__ uint32_t half_up(float x) {
  const _Float16 h = static_cast<_Float16>(x);
  uint32_t hb = __builtin_bit_cast(uint16_t, h);
  if (static_cast<float>(h) < x) hb = (hb & 0x8000u) ? (hb == 0x8000u ? 0x0001u : hb - 1u) : hb + 1u;
  return hb;
}
__device__ __forceinline__ float half_lo(uint32_t w) {
  return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(w & 0xFFFFu)));
}
__device__ __forceinline__ float half_hi(uint32_t w) {
  return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(w >> 16)));
}
// {lo.x | lo.y << 16, lo.z | hi.x << 16, hi.y | hi.z << 16}
__device__ __forceinline__ uint3 pack_hbox(const float4& lo, const float4& hi) {
  return make_uint3(half_down(lo.x) | (half_down(lo.y) << 16), half_down(lo.z) | (half_up(hi.x) << 16),
                    half_up(hi.y) | (half_up(hi.z) << 16));
}
__device__ __forceinline__ float hbox_lb2(const uint3& h, float ax, float ay, float az, float bx, float by, float bz) {
  return box_box_lb2(ax, ay, az, bx, by, bz, half_lo(h.x), half_hi(h.x), half_lo(h.y), half_hi(h.y), half_lo(h.z),
                     half_hi(h.z));
}

template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_max_u(uint32_t v) {
  return max(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, ROWS, 0xF, false)));
}
// max over the wave of non-negative float bits (k-th distances; +inf allowed)
__device__ __forceinline__ float wave_max_nonneg(float x) {
  uint32_t v = __float_as_uint(x);
  v = dpp_max_u<0x111, 0xF>(v);
  v = dpp_max_u<0x112, 0xF>(v);
  v = dpp_max_u<0x114, 0xF>(v);
  v = dpp_max_u<0x118, 0xF>(v);
  v = dpp_max_u<0x142, 0xA>(v);
  v = dpp_max_u<0x143, 0xC>(v);
  return __uint_as_float(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63)));
}
// max over the wave of any floats (order-preserving bits)
__device__ __forceinline__ float wave_max_nonneg_signed(float x) {
  uint32_t v = float_order(x);
  v = dpp_max_u<0x111, 0xF>(v);
  v = dpp_max_u<0x112, 0xF>(v);
  v = dpp_max_u<0x114, 0xF>(v);
  v = dpp_max_u<0x118, 0xF>(v);
  v = dpp_max_u<0x142, 0xA>(v);
  v = dpp_max_u<0x143, 0xC>(v);
  return float_unorder(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63)));
}
__device__ __forceinline__ uint32_t wave_umax_i(uint32_t v) {
  v = dpp_max_u<0x111, 0xF>(v);
  v = dpp_max_u<0x112, 0xF>(v);
  v = dpp_max_u<0x114, 0xF>(v);
  v = dpp_max_u<0x118, 0xF>(v);
  v = dpp_max_u<0x142, 0xA>(v);
  v = dpp_max_u<0x143, 0xC>(v);
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}
// min over the wave of non-negative floats (+inf allowed): their bits order like the values
__device__ __forceinline__ float wave_min_nonneg(float x) {
  return __uint_as_float(~wave_umax_i(~__float_as_uint(x)));
}

}  // namespace dvcp
