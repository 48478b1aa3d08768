// bq_scan.hip -- the fp32 ball query's two scans over the built workspace (bq_common.h lists the
// units).  Both produce exactly the index-order result of ball_query_kernel (ball_query.hip).
//
// bq_wave_kernel (any N): one wave = 64 centres with its own early exit; points are streamed in
// ascending index order as wave-uniform scalar loads of packed (x, y, z, |p|^2) rows.
//
// bq_tiled_kernel (N <= 65536): a sparse radius (most centres far from nsample hits) makes the
// scan above visit every point for every centre.  bq_build_kernel sorts the points along a Hilbert curve into
// 64-point tiles with boxes and the centres into a Hilbert permutation, so a wave's 64 centres
// have a compact box.  The wave marks, in an LDS bitmap indexed by ORIGINAL point index, every
// point whose distance bound to the wave box passes the radius with a rounding margin, then
// scans the set bits in ascending index order with the same test, append rule and early exit.
// A point left out of the bitmap provably fails the reference's test (see bq_prune_thr), so the
// result is identical, and the scan touches only the neighbourhood of the wave.
#include "bq_common.h"
#include "morton.h"

namespace dvcp {

__global__ __launch_bounds__(256) void bq_wave_kernel(const float4* __restrict__ packed, int N, PointsView<float> ctr,
                                                      int S, float r2, int nsample, int32_t* __restrict__ count,
                                                      int32_t* __restrict__ list, int64_t* __restrict__ padded) {
  const int b = blockIdx.y;
  const int s = blockIdx.x * 256 + threadIdx.x;
  if ((blockIdx.x * 256 + (threadIdx.x & ~63)) >= S) return;  // whole wave past the end
  const bool live = s < S;
  float cx = 0.f, cy = 0.f, cz = 0.f;
  if (live) {
    cx = ctr.at(b, 0, s);
    cy = ctr.at(b, 1, s);
    cz = ctr.at(b, 2, s);
  }
  const float ssc = sumsq3(cx, cy, cz);
  const int64_t row = (static_cast<int64_t>(b) * S + s) * nsample;
  int cnt = live ? 0 : nsample;
  int first = N;
  const const_float* P = (const const_float*)uniform_ptr(packed + static_cast<int64_t>(b) * bq_padded_n(N));
  for (int n0 = 0; n0 < N; n0 += 16) {
    float c[64];
#pragma unroll
    for (int u = 0; u < 64; ++u) c[u] = P[4 * n0 + u];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int n = n0 + j;
      const float d2 = expansion_d2(dot3_blas(cx, cy, cz, c[4 * j], c[4 * j + 1], c[4 * j + 2]), ssc, c[4 * j + 3]);
      if ((n < N) & !(d2 > r2) & (cnt < nsample)) {
        first = cnt == 0 ? n : first;
        if (list) list[row + cnt] = n;
        if (padded) padded[row + cnt] = n;
        ++cnt;
      }
    }
    if (__ballot(cnt < nsample) == 0) break;
  }
  if (!live) return;
  if (count) count[static_cast<int64_t>(b) * S + s] = cnt;
  if (list && cnt == 0) list[row] = 0;  // (see bq_tiled_kernel)
  if (padded)
    for (int j = cnt; j < nsample; ++j) padded[row + j] = first;
}

__device__ __forceinline__ float wave_fmin(float v) {
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, kWave));
  return v;
}
__device__ __forceinline__ float wave_fmax(float v) {
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}

// Prune threshold.  The reference's d2 = ((-2 dot) + |c|^2) + |p|^2 (dot an fma chain) differs
// from the exact squared distance by at most ~10 u (|c|^2 + |p|^2) (u = 2^-24; each of the six
// roundings is bounded by u times a magnitude <= 2 (|c|^2 + |p|^2)); a gap-based box bound
// computed in fp32 exceeds the exact bound by at most (1 + 2^-20).  A point whose computed bound
// exceeds (r^2 + 16 u (|c|^2max + |p|^2max)) (1 + 2^-19) therefore has computed d2 > r^2.
__device__ __forceinline__ float bq_prune_thr(float r2, float ssc_max, float ssp_max) {
  return (r2 + 0x1p-20f * (ssc_max + ssp_max)) * (1.0f + 0x1p-19f);
}

// |p|^2 upper bound over a box (per axis the larger endpoint magnitude)
__device__ __forceinline__ float box_ss_max(float lx, float ly, float lz, float hx, float hy, float hz) {
  const float ax = fmaxf(fabsf(lx), fabsf(hx)), ay = fmaxf(fabsf(ly), fabsf(hy)), az = fmaxf(fabsf(lz), fabsf(hz));
  return ((ax * ax + ay * ay) + az * az) * (1.0f + 0x1p-20f);
}

__device__ __forceinline__ float bq_gap(float lo, float hi, float v_lo, float v_hi) {
  return fmaxf(fmaxf(v_lo - hi, lo - v_hi), 0.0f);
}

// MAXT bounds the tile count; the per-wave bitmap holds MAXT * 2 words (one bit per point).
template <int MAXT>
__global__ __launch_bounds__(256) void bq_tiled_kernel(BqLayout L, int N, PointsView<float> ctr, int S, float r2,
                                                       int nsample, int32_t* __restrict__ count,
                                                       int32_t* __restrict__ list, int64_t* __restrict__ padded,
                                                       int xcd) {
  __shared__ uint32_t bm[4][MAXT * 2];
  __shared__ float4 cpt[4][kBqCap];
  __shared__ int32_t cid[4][kBqCap];
  // cloud and block within it; xcd != 0 (B % 8 == 0): workgroups reach the XCDs round robin by
  // linear id, which is re-mapped so XCD x takes clouds x, x + 8, ... (one cloud's tiles and rows
  // per L2)
  int b = blockIdx.y, bx = blockIdx.x;
  if (xcd) {
    const int lin = static_cast<int>(blockIdx.y * gridDim.x + blockIdx.x);
    const int slot = lin >> 3;
    b = (lin & 7) + 8 * (slot / static_cast<int>(gridDim.x));
    bx = slot % static_cast<int>(gridDim.x);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q0 = (bx * 4 + wave) * 64;
  if (q0 >= S) return;
  const int T = (N + kBqTile - 1) / kBqTile;
  const int NW = (N + 31) >> 5;
  const int np = bq_padded_n(N);
  const bool live = q0 + lane < S;
  const int s = live ? L.cperm[static_cast<int64_t>(b) * S + q0 + lane] : 0;
  float cx = 0.f, cy = 0.f, cz = 0.f;
  if (live) {
    cx = ctr.at(b, 0, s);
    cy = ctr.at(b, 1, s);
    cz = ctr.at(b, 2, s);
  }
  const float ssc = sumsq3(cx, cy, cz);
  const bool fin = __builtin_isfinite(cx) && __builtin_isfinite(cy) && __builtin_isfinite(cz);
  const float inf = __builtin_huge_valf();
  // Lane groups.  A run of 64 curve-consecutive centres can straddle a jump of the curve (a few
  // lanes' centres far from the rest): its box, and so the candidate union every lane scans, is
  // then many times that of either part, and such waves set the kernel's duration (C3: median
  // wave ~60 us, the slowest ~300 us with 10x the median's candidates, all in clouds with
  // outliers).  The wave therefore looks for the best single cut of its lane range (the split
  // minimising the summed r-expanded box volumes, by prefix and suffix box scans), keeps it when
  // it saves 30 %, and tries once more inside each part: up to four lane groups, each running the
  // bitmap pass and the scan for its own box while the other lanes idle.  A centre's list
  // depends only on its own tests, so the grouping never changes a result.
  int cut1 = -1, cut2 = -1, cut3 = -1;
  if (__ballot(live && !fin) == 0) {  // (a non-finite centre needs every point anyway)
    const float rr2 = 2.0f * sqrtf(r2);
    const bool bl = live;
    auto box_vol = [&](const float (&lo)[3], const float (&hi)[3]) {
      return !(hi[0] >= lo[0]) ? 0.0f : ((hi[0] - lo[0] + rr2) * (hi[1] - lo[1] + rr2)) * (hi[2] - lo[2] + rr2);
    };
    // the best single cut of lanes [a, e): the first lane of the second part, or -1
    auto best_cut = [&](int a, int e) -> int {
      const bool in = bl && lane >= a && lane < e;
      const float c3[3] = {cx, cy, cz};
      float plo[3], phi[3], slo[3], shi[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        plo[d] = slo[d] = in ? c3[d] : inf;
        phi[d] = shi[d] = in ? c3[d] : -inf;
      }
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float ul = __shfl_up(plo[d], off, kWave), uh = __shfl_up(phi[d], off, kWave);
          const float dl = __shfl_down(slo[d], off, kWave), dh = __shfl_down(shi[d], off, kWave);
          if (lane >= off) {
            plo[d] = fminf(plo[d], ul);
            phi[d] = fmaxf(phi[d], uh);
          }
          if (lane + off < 64) {
            slo[d] = fminf(slo[d], dl);
            shi[d] = fmaxf(shi[d], dh);
          }
        }
      }
      const float vp = box_vol(plo, phi);  // lanes a..lane
      const float vs = box_vol(slo, shi);  // lanes lane..e-1
      const float vprev = __shfl_up(vp, 1, kWave);
      const float whole = __shfl(vp, 63, kWave);
      const float cost = (lane > a && lane < e) ? vprev + vs : inf;
      float m = cost;
      for (int off = 32; off > 0; off >>= 1) m = fminf(m, __shfl_xor(m, off, kWave));
      if (!(m < 0.7f * whole)) return -1;
      return static_cast<int>(__builtin_ctzll(__ballot(cost == m)));
    };
    cut1 = best_cut(0, 64);
    if (cut1 > 0) {
      cut2 = best_cut(0, cut1);
      cut3 = best_cut(cut1, 64);
    }
  }
  const int ngroups = 1 + (cut1 >= 0) + (cut2 >= 0) + (cut3 >= 0);
  const int gid = (cut2 >= 0 && lane >= cut2) + (cut1 >= 0 && lane >= cut1) + (cut3 >= 0 && lane >= cut3);
  uint32_t* mybm = bm[wave];
  const float4* tb = L.tbox + static_cast<int64_t>(b) * T * 2;
  const float4* so = L.sorted + static_cast<int64_t>(b) * T * kBqTile;
  const float4* pk = L.packed + static_cast<int64_t>(b) * np;
  const int64_t row = (static_cast<int64_t>(b) * S + s) * nsample;
  int cnt = live ? 0 : nsample;
  int first = N;
  float4* mypt = cpt[wave];
  int32_t* myid = cid[wave];
  for (int g = 0; g < ngroups; ++g) {
    const bool act = live && gid == g;
    if (__ballot(act) == 0) continue;
    // the group's box; a non-finite centre needs every point
    const float wlx = wave_fmin(act ? (fin ? cx : -inf) : inf), whx = wave_fmax(act ? (fin ? cx : inf) : -inf);
    const float wly = wave_fmin(act ? (fin ? cy : -inf) : inf), why = wave_fmax(act ? (fin ? cy : inf) : -inf);
    const float wlz = wave_fmin(act ? (fin ? cz : -inf) : inf), whz = wave_fmax(act ? (fin ? cz : inf) : -inf);
    const float ssc_max = wave_fmax(act && fin ? ssc : 0.0f);

    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < NW; i += 64) mybm[i] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int t0 = 0; t0 < T; t0 += 64) {
      const int t = t0 + lane;
      bool cand = false;
      if (t < T) {
        const float4 lo = tb[2 * t], hi = tb[2 * t + 1];
        const float gx = bq_gap(lo.x, hi.x, wlx, whx), gy = bq_gap(lo.y, hi.y, wly, why), gz = bq_gap(lo.z, hi.z, wlz, whz);
        const float lb2 = (gx * gx + gy * gy) + gz * gz;
        cand = !(lb2 > bq_prune_thr(r2, ssc_max, box_ss_max(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z)));
      }
      uint64_t mask = __ballot(cand);
      while (mask) {
        // up to four candidate tiles per pass, their loads in flight together
        int tt[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          tt[u] = mask ? t0 + __builtin_ctzll(mask) : -1;
          mask &= mask - 1;
        }
        float4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = so[max(tt[u], 0) * kBqTile + lane];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int idx = __float_as_int(q[u].w);
          const float gx = bq_gap(q[u].x, q[u].x, wlx, whx), gy = bq_gap(q[u].y, q[u].y, wly, why),
                      gz = bq_gap(q[u].z, q[u].z, wlz, whz);
          const float lb2 = (gx * gx + gy * gy) + gz * gz;
          const float ssp = ((q[u].x * q[u].x + q[u].y * q[u].y) + q[u].z * q[u].z) * (1.0f + 0x1p-20f);
          // NaN coordinates give NaN bounds, which are kept (never "> thr")
          if (tt[u] >= 0 && idx < N && !(lb2 > bq_prune_thr(r2, ssc_max, ssp)))
            atomicOr(&mybm[idx >> 5], 1u << (idx & 31));
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    for (int c0 = 0; c0 < NW; c0 += 64) {
      const uint32_t word = (c0 + lane < NW) ? mybm[c0 + lane] : 0u;
      const int pc = __builtin_popcount(word);
      int incl = pc;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += u;
      }
      const int total = __shfl(incl, 63, kWave);
      const int excl = incl - pc;
      for (int base = 0; base < total; base += kBqCap) {
        // this round's candidates (positions [base, base + kBqCap) in index order): indices first,
        // then the points gathered cooperatively (several loads in flight per lane)
        int p = excl;
        uint32_t wd = word;
        while (wd && p < base + kBqCap) {
          const int bit = __builtin_ctz(wd);
          wd &= wd - 1;
          if (p >= base) myid[p - base] = (c0 + lane) * 32 + bit;
          ++p;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int nc = min(kBqCap, total - base);
#pragma unroll
        for (int u = 0; u < kBqCap / 64; ++u) {
          const int j = u * 64 + lane;
          if (j < nc) mypt[j] = pk[myid[j]];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int j0 = 0; j0 < nc; j0 += 64) {
          const int je = min(nc, j0 + 64);
          for (int j1 = j0; j1 < je; j1 += 8) {
            float4 q[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) q[u] = mypt[j1 + u];  // j1 + 7 < kBqCap
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const float d2 = expansion_d2(dot3_blas(cx, cy, cz, q[u].x, q[u].y, q[u].z), ssc, q[u].w);
              if (act & (j1 + u < je) & !(d2 > r2) & (cnt < nsample)) {
                const int n = myid[j1 + u];
                first = cnt == 0 ? n : first;
                if (list) list[row + cnt] = n;
                if (padded) padded[row + cnt] = n;
                ++cnt;
              }
            }
          }
          if (__ballot(act && cnt < nsample) == 0) goto group_done;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
  group_done:;
  }
  if (!live) return;
  if (count) count[static_cast<int64_t>(b) * S + s] = cnt;
  // A centre without hits (the reference pads it with index N, :104) gets a valid first list
  // entry, point 0: consumers that clamp count to >= 1 (training passes) then read in bounds, and
  // the forward MLP tables give such a centre a zero row without reading its list.
  if (list && cnt == 0) list[row] = 0;
  if (padded)
    for (int j = cnt; j < nsample; ++j) padded[row + j] = first;
}

int bq_scan_launch(const BqLayout& L, int tiled, int N, PointsView<float> ctr, int S, int B, float r2, int nsample,
                   int32_t* count, int32_t* list, int64_t* padded, hipStream_t st) {
  if (tiled)
    hipLaunchKernelGGL(N <= kBqSmallTiles * kBqTile ? bq_tiled_kernel<kBqSmallTiles> : bq_tiled_kernel<kBqMaxTiles>,
                       dim3(ceil_div(S, 256), B), dim3(256), 0, st, L, N, ctr, S, r2, nsample, count, list, padded,
                       B % 8 == 0 ? 1 : 0);
  else
    hipLaunchKernelGGL(bq_wave_kernel, dim3(ceil_div(S, 256), B), dim3(256), 0, st, L.packed, N, ctr, S, r2, nsample,
                       count, list, padded);
  return launch_status("dvcp_ball_query");
}

}  // namespace dvcp
