// knn_tiled_insert.hip -- the tiled kNN's per-candidate insertion kernel (knn_tiled.hip has the
// overview): a bitonic sort of the wave's tile keys, then every candidate is inserted into the
// lane's sorted list as it appears.  The insertion network is KT slots deep and the whole wave
// executes it for every point that is a candidate for any lane.  dvcp_knn_tiled runs it for
// k <= 16, where that is cheap.  At 32 slots it was the kernel's cost, ~220 such steps per wave
// at C3: round 3 replaced it there with the buffered selection of knn_tiled_sel.hip, 1.37 -> 1.18
// ms per C3 call at the time, and the 32-slot instantiations are reached
// only through dvcp_knn_tiled_insert, the second exact implementation of the parity tests.
#include "knn_tiled_common.h"

namespace dvcp {

// Tiles whose boxes are read (LDS) and tested together.  The loops over it run once; they stay
// because folding them by hand changes the kernels' control flow and machine code (tools/kcmp.py).
constexpr int kBoxBatch = 1;

// Bitonic sort (ascending) of 64*R keys held as keys[r] at position r*64 + lane.
template <int R>
__device__ __forceinline__ void wave_bitonic(uint32_t (&keys)[R]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 2; k <= 64 * R; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j >= 64) {  // partner is another register of the same lane
        const int jr = j >> 6;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if ((r & jr) == 0) {
            const int i = r * 64 + lane;
            const bool up = (i & k) == 0;
            const uint32_t a = keys[r], c = keys[r + jr];
            const bool sw = up ? (a > c) : (a < c);
            keys[r] = sw ? c : a;
            keys[r + jr] = sw ? a : c;
          }
        }
      } else {  // partner lane = lane ^ j, same register
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int i = r * 64 + lane;
          const uint32_t o = static_cast<uint32_t>(__shfl_xor(static_cast<int>(keys[r]), j, kWave));
          const bool lower = (lane & j) == 0;  // this lane holds the lower index of the pair
          const bool up = (i & k) == 0;
          const uint32_t mn = min(keys[r], o), mx = max(keys[r], o);
          keys[r] = (lower == up) ? mn : mx;
        }
      }
    }
  }
}

// KT: slots of the sorted list (1, 8, 16 or 32: the first that holds k); R: registers of 64 tile keys.
template <int KT, int R>
__global__ __launch_bounds__(kTiledThreads) void knn_tiled_query_kernel(const float4* __restrict__ sorted,
                                                                        const float4* __restrict__ tbox,
                                                                        const float4* __restrict__ qsorted, int M,
                                                                        int Q, int k, float* __restrict__ dist,
                                                                        int32_t* __restrict__ idx,
                                                                        int64_t* __restrict__ idx64, int B8) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // Cloud and block within it.  Workgroups reach the 8 XCDs round robin by linear id, so with
  // B % 8 == 0 the linear id is re-mapped to give XCD x the clouds x, x + 8, ...: each cloud's
  // sorted points and boxes are then fetched into one XCD's L2 instead of all eight.
  int b = blockIdx.y, bx = blockIdx.x;
  if ((B8 & 1) != 0) {
    const int lin = static_cast<int>(blockIdx.y * gridDim.x + blockIdx.x);
    const int xo = lin & 7, slot = lin >> 3;
    b = xo + 8 * (slot / static_cast<int>(gridDim.x));
    bx = slot % static_cast<int>(gridDim.x);
  }
  const int T = (M + kTile - 1) / kTile;
  // the cloud's tile boxes in LDS (all four waves scan the same cloud): the per-lane box test
  // then reads an LDS broadcast instead of waiting on a scalar load per tile
  __shared__ float4 sbox[2 * kMaxTiles];
  {
    const float4* tbg = tbox + static_cast<int64_t>(b) * T * 2;
    for (int i = threadIdx.x; i < 2 * T; i += kTiledThreads) sbox[i] = tbg[i];
    __syncthreads();
  }
  const int sq = (bx * (kTiledThreads / kWave) + wave) * kWave + lane;
  if ((bx * (kTiledThreads / kWave) + wave) * kWave >= Q) return;  // whole wave past the end
  const bool live = sq < Q;
  // this lane's query in curve order: one coalesced 16-byte row (converted to fp32 by the scatter,
  // knn_cuda's .float())
  const float4 qrow = live ? qsorted[static_cast<int64_t>(b) * Q + sq] : make_float4(0.f, 0.f, 0.f, 0.f);
  const int q = __float_as_int(qrow.w);
  const float qx = qrow.x, qy = qrow.y, qz = qrow.z;
  // the wave's query box (live lanes only)
  float wl[3] = {live ? qx : __builtin_huge_valf(), live ? qy : __builtin_huge_valf(),
                 live ? qz : __builtin_huge_valf()};
  float wh[3] = {live ? qx : -__builtin_huge_valf(), live ? qy : -__builtin_huge_valf(),
                 live ? qz : -__builtin_huge_valf()};
#pragma unroll
  for (int a = 0; a < 3; ++a)
    for (int off = 32; off > 0; off >>= 1) {
      wl[a] = fminf(wl[a], __shfl_xor(wl[a], off, kWave));
      wh[a] = fmaxf(wh[a], __shfl_xor(wh[a], off, kWave));
    }
  const float4* tb = tbox + static_cast<int64_t>(b) * T * 2;
  // tile keys: lb2(query box, tile box) with the low 10 mantissa bits replaced by the tile id.
  // Truncation only lowers a non-negative float, so key value <= the true bound.
  uint32_t keys[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int t = r * 64 + lane;
    if (t < T) {
      const float4 lo = tb[2 * t], hi = tb[2 * t + 1];
      const float lb = box_box_lb2(wl[0], wl[1], wl[2], wh[0], wh[1], wh[2], lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
      keys[r] = (__float_as_uint(lb) & ~kTileIdBits) | static_cast<uint32_t>(t);
    } else {
      keys[r] = 0xFFFFFFFFu;
    }
  }
  wave_bitonic<R>(keys);

  // The list is kept as 64-bit keys (d2 bits << 32 | index): d2 >= 0 orders like its bits, so
  // one unsigned compare orders by (d2, index) and an insertion is one compare + two selects
  // per slot.
  // (stored as 32-bit halves: a dynamically indexed 64-bit array is not promoted to registers)
  uint32_t kh[KT], kl[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) {  // empty slot: (+inf, 0xFFFFFFFF), above every finite point
    kh[t] = 0x7F800000u;
    kl[t] = ~0u;
  }
  constexpr uint64_t kEmpty = (static_cast<uint64_t>(0x7F800000u) << 32) | 0xFFFFFFFFu;
#define DVCP_KK(t) ((static_cast<uint64_t>(kh[t]) << 32) | kl[t])
  const int kq = k - 1;  // wave-uniform: kh[kq], kl[kq] are indexed register reads
  float kth = live ? __builtin_huge_valf() : 0.0f;  // dead lanes never need more points
  uint64_t kkey = live ? kEmpty : 0ull;
  float wkth = wave_max_nonneg(kth);
  const float4* P = uniform_ptr(sorted + static_cast<int64_t>(b) * T * kTile);
  bool stop = false;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    for (int i0 = 0; i0 < 64 && !stop; i0 += kBoxBatch) {
      if (r * 64 + i0 >= T) break;
      // kBoxBatch tiles of the order: keys, then their boxes (LDS broadcasts) and this lane's bounds
      uint32_t key4[kBoxBatch];
      float lb4[kBoxBatch];
#pragma unroll
      for (int j = 0; j < kBoxBatch; ++j) {
        key4[j] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(keys[r]), i0 + j));
        const int tj = static_cast<int>(key4[j] & kTileIdBits) < T ? static_cast<int>(key4[j] & kTileIdBits) : 0;
        const float4 lo = sbox[2 * tj], hi = sbox[2 * tj + 1];
        lb4[j] = box_box_lb2(qx, qy, qz, qx, qy, qz, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
      }
#pragma unroll
      for (int j = 0; j < kBoxBatch; ++j) {
        if (r * 64 + i0 + j >= T) break;
        const uint32_t key = key4[j];
        if (__uint_as_float(key & ~kTileIdBits) > wkth) {  // every later tile is farther
          stop = true;
          break;
        }
        const int t = static_cast<int>(key & kTileIdBits);
        const float lbq = lb4[j];
        const bool act = live & (lbq <= kth);
        if (__ballot(act) == 0) continue;
        const const_float* tp = (const const_float*)(P + t * kTile);
        uint64_t ins = 0;
        for (int j0 = 0; j0 < kTile; j0 += 16) {
          // the whole 16-point chunk is loaded (scalar loads, one wait) before any branch
          float c[64];
#pragma unroll
          for (int u = 0; u < 64; ++u) c[u] = tp[4 * j0 + u];
          // pass 1 (unrolled): every distance of the chunk, and which points are a candidate for
          // some lane against the k-th key at chunk start (a superset: the key only decreases)
          float d2v[16];
          uint32_t piv[16];
          uint32_t todo = 0;
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const float dx = c[4 * j] - qx, dy = c[4 * j + 1] - qy, dz = c[4 * j + 2] - qz;
            d2v[j] = (dx * dx + dy * dy) + dz * dz;
            piv[j] = __float_as_uint(c[4 * j + 3]);
            const uint64_t pk = (static_cast<uint64_t>(__float_as_uint(d2v[j])) << 32) | piv[j];
            // d2 < inf also rejects NaN (padding) and infinite distances, as dvcp_knn does
            const bool cand = act & (d2v[j] < __builtin_huge_valf()) & (pk < kkey);
            todo |= __ballot(cand) != 0 ? (1u << j) : 0u;
          }
          // pass 2: those points in order, each re-tested against the current key, then inserted
          // (one compare + two selects per slot)
          while (todo) {
            const int j = __builtin_ctz(todo);
            todo &= todo - 1;
            const float d2 = d2v[j];  // indexed register reads (uniform j)
            const uint32_t pi = piv[j];
            const uint64_t pk = (static_cast<uint64_t>(__float_as_uint(d2)) << 32) | pi;
            const bool cand = act & (d2 < __builtin_huge_valf()) & (pk < kkey);
            const uint64_t m = __ballot(cand);
            if (m == 0) continue;
            ins |= m;
            // a non-candidate lane compares with the all-ones key, which is below no slot
            const uint64_t pkc = cand ? pk : ~0ull;
            bool lt[KT];
#pragma unroll
            for (int u = 0; u < KT; ++u) lt[u] = pkc < DVCP_KK(u);
#pragma unroll
            for (int u = KT - 1; u > 0; --u) {
              kh[u] = lt[u - 1] ? kh[u - 1] : (lt[u] ? __float_as_uint(d2) : kh[u]);
              kl[u] = lt[u - 1] ? kl[u - 1] : (lt[u] ? pi : kl[u]);
            }
            kh[0] = lt[0] ? __float_as_uint(d2) : kh[0];
            kl[0] = lt[0] ? pi : kl[0];
            kkey = live ? (KT == 1 ? DVCP_KK(0) : DVCP_KK(kq)) : 0ull;
            kth = __uint_as_float(static_cast<uint32_t>(kkey >> 32));
          }
        }
        if (ins != 0) wkth = wave_max_nonneg(kth);
      }
    }
  }
  if (!live) return;
  const int64_t o = (static_cast<int64_t>(b) * Q + q) * k;
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    if (t < k) {
      const bool ok = DVCP_KK(t) != kEmpty;  // fewer than k finite points: like dvcp_knn (inf, -1)
      const float d2 = __uint_as_float(kh[t]);
      const int i = static_cast<int>(kl[t]);
      if (dist) dist[o + t] = ok ? sqrt_rn(d2) : __builtin_huge_valf();
      if (idx) idx[o + t] = ok ? i : -1;
      if (idx64) idx64[o + t] = ok ? i : -1;
    }
  }
#undef DVCP_KK
}

template <int KT, int R>
static int launch_insert(const TiledLayout& L, int M, int Q, int B, int k, float* dist, int32_t* idx, int64_t* idx64,
                         hipStream_t st) {
  const dim3 grid(ceil_div(Q, kTiledThreads), B);
  const int xcd = B % 8 == 0 ? 1 : 0;  // XCD-aware cloud mapping (equal clouds per XCD)
  hipLaunchKernelGGL((knn_tiled_query_kernel<KT, R>), grid, dim3(kTiledThreads), 0, st, L.sorted, L.tbox, L.qsorted,
                     M, Q, k, dist, idx, idx64, xcd);
  return launch_status("dvcp_knn_tiled(query)");
}

// k <= 8: tile keys in one register (M <= 1024) or sixteen (any M); k = 9..16 has the sixteen
// only; k = 17..32 the smallest count that holds the tiles.
int knn_insert_launch(const TiledLayout& L, int M, int Q, int B, int k, float* dist, int32_t* idx, int64_t* idx64,
                      hipStream_t st) {
  const int T = ceil_div(M, kTile);
  if (k <= 1)
    return T <= 64 ? launch_insert<1, 1>(L, M, Q, B, k, dist, idx, idx64, st)
                   : launch_insert<1, 16>(L, M, Q, B, k, dist, idx, idx64, st);
  if (k <= 8)
    return T <= 64 ? launch_insert<8, 1>(L, M, Q, B, k, dist, idx, idx64, st)
                   : launch_insert<8, 16>(L, M, Q, B, k, dist, idx, idx64, st);
  if (k <= 16) return launch_insert<16, 16>(L, M, Q, B, k, dist, idx, idx64, st);
  return knn_for_tile_regs(T, [&](auto r) {
    return launch_insert<32, decltype(r)::value>(L, M, Q, B, k, dist, idx, idx64, st);
  });
}

}  // namespace dvcp
