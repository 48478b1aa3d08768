// fps_common.h -- shared by the FPS units (fps.hip lists them): wave reductions on DPP, the Morton
// setup, the running-minimum update, and the launches the dispatch in fps.hip calls.
#pragma once
#include <type_traits>

#include "common.h"

namespace dvcp {

// ------------------------------------------------------------------------------- DPP helpers
template <int CTRL, int ROWS = 0xF>
__device__ __forceinline__ float dpp_maxf(float v) {
  const int o = __builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROWS, 0xF, false);
  return fmaxf(v, __int_as_float(o));
}
template <int CTRL, int ROWS = 0xF>
__device__ __forceinline__ int dpp_mini(int v) {
  const int o = __builtin_amdgcn_update_dpp(v, v, CTRL, ROWS, 0xF, false);
  return min(v, o);
}
// row_shr:1,2,4,8 then row_bcast:15 (rows 1,3) and row_bcast:31 (rows 2,3): lane 63 holds the
// reduction of all 64 lanes.
__device__ __forceinline__ float wave_maxf_dpp(float v) {
  v = dpp_maxf<0x111>(v);
  v = dpp_maxf<0x112>(v);
  v = dpp_maxf<0x114>(v);
  v = dpp_maxf<0x118>(v);
  v = dpp_maxf<0x142, 0xA>(v);
  v = dpp_maxf<0x143, 0xC>(v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ int wave_mini_dpp(int v) {
  v = dpp_mini<0x111>(v);
  v = dpp_mini<0x112>(v);
  v = dpp_mini<0x114>(v);
  v = dpp_mini<0x118>(v);
  v = dpp_mini<0x142, 0xA>(v);
  v = dpp_mini<0x143, 0xC>(v);
  return __builtin_amdgcn_readlane(v, 63);
}
template <typename T>
__device__ __forceinline__ T readlane_t(T v, int lane);
template <>
__device__ __forceinline__ float readlane_t<float>(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
template <>
__device__ __forceinline__ double readlane_t<double>(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane(static_cast<int>(b & 0xFFFFFFFFll), lane);
  const int hi = __builtin_amdgcn_readlane(static_cast<int>(b >> 32), lane);
  return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}

template <typename T>
__device__ __forceinline__ T readfirstlane_t(T v) {
  return readlane_t(v, 0);
}

// Lower bound of the distance from c to an axis-aligned box, rounded like a point distance
// (branch-free: outside the slab exactly one difference is positive, inside both are <= 0).
template <typename T>
__device__ __forceinline__ T box_lb2(T cx, T cy, T cz, const T (&bx)[6]) {
  const T ex = fmax(fmax(bx[0] - cx, cx - bx[3]), static_cast<T>(0));
  const T ey = fmax(fmax(bx[1] - cy, cy - bx[4]), static_cast<T>(0));
  const T ez = fmax(fmax(bx[2] - cz, cz - bx[5]), static_cast<T>(0));
  return (ex * ex + ey * ey) + ez * ez;
}

template <typename T>
struct alignas(16) FpsSlot {
  float v;
  int i;
  T x, y, z;
};

constexpr int kFpsThreads = 512;  // 8 waves: 2 per SIMD, up to 256 VGPRs each
constexpr int kFpsSel1024 = 1024;  // the fp32 select kernel's workgroup: 16 waves, 4 per SIMD
constexpr int kMortonBins = 4096;
constexpr int kFpsProf = 13;      // timing probe words per wave (fps_kernel<..., TIMING=true>)

__device__ __forceinline__ uint32_t spread4(uint32_t v) {  // 4 bits -> every third bit
  v &= 0xF;
  return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6);
}

__device__ __forceinline__ uint64_t fps_clock() {
  const uint64_t t = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  return t;
}

// Setup shared by the FPS kernels: counting sort of the cloud by 12-bit Morton cell (16^3 cells
// over its bounding box): put(pos, n) for each point n and its sorted position pos.  Only the
// point -> wave/group assignment depends on it, never a result.
template <typename T, int THREADS, typename Put>
__device__ void fps_morton_sort(const PointsView<T>& pts, int b, int N, uint32_t* bins, Put put,
                                T (*red)[3][THREADS / kWave], uint32_t* wsum) {
  constexpr int W = THREADS / kWave;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  T lo[3] = {static_cast<T>(__builtin_huge_val()), static_cast<T>(__builtin_huge_val()),
             static_cast<T>(__builtin_huge_val())};
  T hi[3] = {-lo[0], -lo[1], -lo[2]};
  for (int n = tid; n < N; n += THREADS) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const T v = pts.at(b, a, n);
      lo[a] = v < lo[a] ? v : lo[a];
      hi[a] = v > hi[a] ? v : hi[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    for (int off = 32; off > 0; off >>= 1) {
      const T ol = __shfl_xor(lo[a], off, kWave), oh = __shfl_xor(hi[a], off, kWave);
      lo[a] = ol < lo[a] ? ol : lo[a];
      hi[a] = oh > hi[a] ? oh : hi[a];
    }
    if (lane == 0) {
      red[0][a][wave] = lo[a];
      red[1][a][wave] = hi[a];
    }
  }
  for (int i = tid; i < kMortonBins; i += THREADS) bins[i] = 0u;
  __syncthreads();
  T blo[3], bscale[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    T l = red[0][a][0], h = red[1][a][0];
    for (int w = 1; w < W; ++w) {
      l = red[0][a][w] < l ? red[0][a][w] : l;
      h = red[1][a][w] > h ? red[1][a][w] : h;
    }
    blo[a] = l;
    bscale[a] = h > l ? static_cast<T>(16) / (h - l) : static_cast<T>(0);
  }
  auto cell_of = [&](int n) -> uint32_t {
    uint32_t c = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      int q = static_cast<int>((pts.at(b, a, n) - blo[a]) * bscale[a]);
      q = q < 0 ? 0 : (q > 15 ? 15 : q);
      c |= spread4(static_cast<uint32_t>(q)) << a;
    }
    return c;
  };
  for (int n = tid; n < N; n += THREADS) atomicAdd(&bins[cell_of(n)], 1u);
  __syncthreads();
  {  // exclusive scan of the bins: PER per thread, wave scan, then across waves
    constexpr int PER = kMortonBins / THREADS;
    uint32_t v[PER], s = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      v[k] = bins[tid * PER + k];
      s += v[k];
    }
    uint32_t incl = s;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t u = __shfl_up(incl, off, kWave);
      if (lane >= off) incl += u;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    uint32_t run = base + incl - s;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      bins[tid * PER + k] = run;
      run += v[k];
    }
  }
  __syncthreads();
  for (int n = tid; n < N; n += THREADS) put(atomicAdd(&bins[cell_of(n)], 1u), n);
  __syncthreads();
}

// ---------------------------------------------------------------------- select-round helpers
// Below this cloud size the one-centre-per-step kernel is faster (few groups, short steps; and
// npoint > N tails, where every running minimum is 0, give rounds of one) -- tools/fps_lab.
constexpr int kFpsBatchedMinN = 2048;

template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_umax(uint32_t v) {
  return max(v, static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, ROWS, 0xF, false)));
}
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_umin(uint32_t v) {
  return min(v, static_cast<uint32_t>(
                    __builtin_amdgcn_update_dpp(static_cast<int>(0xFFFFFFFFu), static_cast<int>(v), CTRL, ROWS, 0xF, false)));
}
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
  v = dpp_umax<0x111, 0xF>(v);
  v = dpp_umax<0x112, 0xF>(v);
  v = dpp_umax<0x114, 0xF>(v);
  v = dpp_umax<0x118, 0xF>(v);
  v = dpp_umax<0x142, 0xA>(v);
  v = dpp_umax<0x143, 0xC>(v);
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}
// Two independent wave maxima; the DPP chains interleave, so they cost about one chain's latency.
__device__ __forceinline__ void wave_umax2(uint32_t a, uint32_t b, uint32_t& ma, uint32_t& mb) {
  a = dpp_umax<0x111, 0xF>(a);
  b = dpp_umax<0x111, 0xF>(b);
  a = dpp_umax<0x112, 0xF>(a);
  b = dpp_umax<0x112, 0xF>(b);
  a = dpp_umax<0x114, 0xF>(a);
  b = dpp_umax<0x114, 0xF>(b);
  a = dpp_umax<0x118, 0xF>(a);
  b = dpp_umax<0x118, 0xF>(b);
  a = dpp_umax<0x142, 0xA>(a);
  b = dpp_umax<0x142, 0xA>(b);
  a = dpp_umax<0x143, 0xC>(a);
  b = dpp_umax<0x143, 0xC>(b);
  ma = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(a), 63));
  mb = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(b), 63));
}
__device__ __forceinline__ uint32_t wave_umin(uint32_t v) {
  v = dpp_umin<0x111, 0xF>(v);
  v = dpp_umin<0x112, 0xF>(v);
  v = dpp_umin<0x114, 0xF>(v);
  v = dpp_umin<0x118, 0xF>(v);
  v = dpp_umin<0x142, 0xA>(v);
  v = dpp_umin<0x143, 0xC>(v);
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), 63));
}
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_uadd(uint32_t v) {
  return v + static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, ROWS, 0xF, false));
}
// Inclusive prefix sum over the wave on DPP (row_shr 1, 2, 4, 8 inside each 16-lane row, then
// row_bcast 15 / 31 across rows): no ds_bpermute round trips in the per-round critical path.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  v = dpp_uadd<0x111, 0xF>(v);
  v = dpp_uadd<0x112, 0xF>(v);
  v = dpp_uadd<0x114, 0xF>(v);
  v = dpp_uadd<0x118, 0xF>(v);
  v = dpp_uadd<0x142, 0xA>(v);
  v = dpp_uadd<0x143, 0xC>(v);
  return v;
}

// (Round 5, measured and not kept: the update's x / y differences and squares as packed fp32 pairs,
// v_pk_add_f32 / v_pk_mul_f32, 13 instead of 15 VALU per pair -- 2.99 -> 3.02 ms at 10000,
// profiles/round5/r5bh_fps_pk.log.)
// The fp32 running-minimum update is an integer min of the bit patterns (see fps_update).
// Non-finite coordinates are outside the parity contract: a NaN point keeps 1e10 in the reference
// (NaN < m is false), which then picks it at every later step (its own distance never drops); the
// select kernels certify prefixes on d(c, c) = 0 and diverge there, as does the integer min on a
// NaN with the sign bit set (it is stored; the reference keeps m).  Callers pass finite clouds.
//
// The reference's running-minimum update (:80-82): d in the coordinate dtype, strict '<', stored fp32.
template <typename T>
__device__ __forceinline__ float fps_update(float m, T px, T py, T pz, T cx, T cy, T cz) {
  const T dx = px - cx, dy = py - cy, dz = pz - cz;
  const T d = (dx * dx + dy * dy) + dz * dz;
  if constexpr (sizeof(T) == 4) {
    // = (d < m ? d : m) as one signed-integer min of the bit patterns: d >= +0 (a sum of squares;
    // a NaN d has a larger pattern than any m and keeps m) and m is 1e10, a kept d, or -1 on a
    // padding lane -- all ordered like their patterns.  (fminf adds a canonicalizing v_max.)
    return __int_as_float(min(__float_as_int(d), __float_as_int(m)));
  } else {
    return d < static_cast<T>(m) ? static_cast<float>(d) : m;
  }
}

// --------------------------------------------------------------------------------- launches
// Each is defined in the one unit that instantiates its kernels (explicitly, for float and double).
// The largest cloud of the one-workgroup select kernel: 16 points per lane.
template <typename T>
constexpr int fps_select_max_n() { return 16 * (sizeof(T) == 4 ? kFpsSel1024 : kFpsThreads); }
constexpr uint32_t kFpsSpinCap = 1u << 22;  // polls before a waiting workgroup gives up (a guard)

// Points per lane: f(std::integral_constant<int, P>) for the first P of the list with ppt <= P, so a
// launch instantiates its kernel for exactly the listed P; returns 1 when none covers ppt.
template <int P, int... Ps, typename F>
int fps_for_ppt(int ppt, F&& f) {
  if (ppt <= P) return f(std::integral_constant<int, P>{});
  if constexpr (sizeof...(Ps) > 0) return fps_for_ppt<Ps...>(ppt, f);
  return 1;
}

// fps_step.hip: fps_kernel, N < kFpsBatchedMinN
template <typename T>
int launch_fps_step(PointsView<T> v, int B, int N, int npoint, const int64_t* start, int64_t* out_idx, T* out_xyz,
                    hipStream_t st);
// fps_select.hip: fps_select_kernel, kFpsBatchedMinN <= N <= fps_select_max_n<T>()
template <typename T>
int launch_fps_select(PointsView<T> v, int B, int N, int npoint, const int64_t* start, int64_t* out_idx, T* out_xyz,
                      hipStream_t st);
// fps_step.hip: clouds above the select kernel's -- fps_split_kernel, then fps_dense_kernel; ws: B x N fp32
template <typename T>
int launch_fps_large(PointsView<T> v, int B, int N, int npoint, const int64_t* start, int64_t* out_idx, T* out_xyz,
                     float* ws, int32_t* err, hipStream_t st);
// fps_part.hip: the split select, S workgroups per cloud; returns 1 (nothing launched) when the
// workspace or the instantiated point slots do not cover this (N, S)
int64_t fps_workspace_bytes(int B, int N);
int launch_fps_part(PointsView<float> v, int B, int N, int npoint, const int64_t* start, int64_t* out_idx,
                    float* out_xyz, float* ws, int64_t ws_bytes, int32_t* err, int S, hipStream_t st);

}  // namespace dvcp
