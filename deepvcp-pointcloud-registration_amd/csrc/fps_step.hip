// fps_step.hip -- the FPS kernels that pick one centre per step: fps_kernel (N < 2048), and for
// clouds above the select kernel's the split kernel (S workgroups per cloud) and the dense kernel;
// the step floor probe of bench.py.
#include "fps_common.h"

namespace dvcp {

// THREADS threads (W = THREADS/64 waves) per cloud; PPT points per lane in VGPRs.
// TIMING (diagnostics, tools/fps_lab): per-wave sums of the step phases in shader clocks.
template <typename T, int THREADS, int PPT, bool PRUNE, bool TIMING = false>
__global__ __launch_bounds__(THREADS) void fps_kernel(PointsView<T> pts, int N, int npoint,
                                                      const int64_t* __restrict__ start,
                                                      int64_t* __restrict__ out_idx, T* __restrict__ out_xyz,
                                                      unsigned long long* __restrict__ prof) {
  constexpr int W = THREADS / kWave;
  constexpr int RANGE = kWave * PPT;  // sorted positions per wave
  static_assert(W <= 16 && (W & (W - 1)) == 0, "slot reduction covers one DPP row");
  static_assert(PPT % 2 == 0 || PPT == 1, "original indices are packed two per VGPR");
  __shared__ uint32_t bins[kMortonBins];
  __shared__ uint16_t perm[THREADS * PPT];
  __shared__ uint8_t owner[THREADS * PPT];
  __shared__ FpsSlot<T> slots[2][W];
  __shared__ T red[2][3][W];
  __shared__ uint32_t wsum[W];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  fps_morton_sort<T, THREADS>(pts, b, N, bins, [&](uint32_t pos, int n) { perm[pos] = static_cast<uint16_t>(n); },
                              red, wsum);
  for (int pos = tid; pos < N; pos += THREADS) owner[perm[pos]] = static_cast<uint8_t>(pos / RANGE);
  __syncthreads();
  // ---- setup 3: each wave lists its points in ascending original index (stream compaction) ---
  // Slot p of a lane then holds the wave's (p*64 + lane)-th smallest index, so a lane meets its
  // points in index order and a strict '>' keeps the lowest index among equal maxima (:83).
  {
    int k = 0;
    for (int base = 0; base < N; base += kWave) {
      const int n = base + lane;
      const bool mine = (n < N) && owner[n] == wave;
      const uint64_t m = __ballot(mine);
      if (mine) perm[wave * RANGE + k + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0))] =
          static_cast<uint16_t>(n);
      k += __popcll(m);
    }
  }
  __syncthreads();

  // ---- setup 4: this lane's points, running minima, packed indices; the wave's box -----------
  const int count = min(RANGE, max(0, N - wave * RANGE));
  T px[PPT], py[PPT], pz[PPT];
  float dmin[PPT];
  uint32_t pidp[(PPT + 1) / 2];
  T wb[6];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    wb[a] = static_cast<T>(__builtin_huge_val());
    wb[3 + a] = -wb[a];
  }
#pragma unroll
  for (int p = 0; p < (PPT + 1) / 2; ++p) pidp[p] = 0u;
#pragma unroll
  for (int p = 0; p < PPT; ++p) {
    const int k = p * kWave + lane;
    if (k < count) {
      const uint32_t n = perm[wave * RANGE + k];
      pidp[p >> 1] |= n << ((p & 1) * 16);
      px[p] = pts.at(b, 0, n);
      py[p] = pts.at(b, 1, n);
      pz[p] = pts.at(b, 2, n);
      dmin[p] = 1e10f;  // torch.ones(B, N) * 1e10 (fp32), :74
      wb[0] = px[p] < wb[0] ? px[p] : wb[0];
      wb[1] = py[p] < wb[1] ? py[p] : wb[1];
      wb[2] = pz[p] < wb[2] ? pz[p] : wb[2];
      wb[3] = px[p] > wb[3] ? px[p] : wb[3];
      wb[4] = py[p] > wb[4] ? py[p] : wb[4];
      wb[5] = pz[p] > wb[5] ? pz[p] : wb[5];
    } else {
      px[p] = py[p] = pz[p] = static_cast<T>(0);
      dmin[p] = -1.0f;  // never updated (d >= 0) and never selected
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    for (int off = 32; off > 0; off >>= 1) {
      const T ol = __shfl_xor(wb[a], off, kWave), oh = __shfl_xor(wb[3 + a], off, kWave);
      wb[a] = ol < wb[a] ? ol : wb[a];
      wb[3 + a] = oh > wb[3 + a] ? oh : wb[3 + a];
    }
    wb[a] = readfirstlane_t(wb[a]);
    wb[3 + a] = readfirstlane_t(wb[3 + a]);
  }

  int64_t cur = start[b];
  if (cur < 0 || cur >= N) cur = 0;  // host validates; keep the kernel in bounds regardless
  T cx = pts.at(b, 0, cur), cy = pts.at(b, 1, cur), cz = pts.at(b, 2, cur);

  int64_t* oi = out_idx + static_cast<int64_t>(b) * npoint;
  T* ox = out_xyz ? out_xyz + static_cast<int64_t>(b) * 3 * npoint : nullptr;

  // the wave's cached best (wave-uniform): value, original index, coordinates
  float wv = __builtin_huge_valf();  // forces the first step to update
  int wi = 0x7FFFFFFF;
  T wx = 0, wy = 0, wz = 0;
  const bool empty_wave = count == 0;
  uint64_t ph[4] = {0, 0, 0, 0}, nact = 0;

  for (int step = 0; step < npoint; ++step) {
    uint64_t t0 = 0, t1 = 0, t2 = 0;
    if constexpr (TIMING) t0 = fps_clock();
    if (tid == 0) {
      oi[step] = cur;
      if (ox) {
        ox[step] = cx;
        ox[npoint + step] = cy;
        ox[2 * npoint + step] = cz;
      }
    }
    const bool active = !empty_wave & (!PRUNE || !(box_lb2(cx, cy, cz, wb) >= static_cast<T>(wv)));
    if (active) {
      float bv = -1.0f;
      int bp = 0;
#pragma unroll
      for (int p = 0; p < PPT; ++p) {
        const T dx = px[p] - cx, dy = py[p] - cy, dz = pz[p] - cz;
        const T d = (dx * dx + dy * dy) + dz * dz;  // torch.sum((xyz - c) ** 2, -1), :80
        if constexpr (sizeof(T) == 4) {
          dmin[p] = fminf(d, dmin[p]);  // == (d < dmin ? d : dmin) for finite values, :81-82
        } else {
          dmin[p] = d < static_cast<T>(dmin[p]) ? static_cast<float>(d) : dmin[p];
        }
        const bool c = dmin[p] > bv;  // strict: the first (lowest-index) of equal maxima stays
        bp = c ? p : bp;
        bv = c ? dmin[p] : bv;
      }
      if constexpr (TIMING) t1 = fps_clock();
      wv = wave_maxf_dpp(bv);
      const uint64_t tied = __ballot(bv == wv);
      int wl;
      if ((tied & (tied - 1)) == 0) {
        wl = __ffsll(static_cast<long long>(tied)) - 1;
      } else {  // equal maxima in several lanes: the lowest original index among them
        uint32_t mine = 0x7FFFFFFFu;
#pragma unroll
        for (int p = 0; p < PPT; ++p) mine = bp == p ? ((pidp[p >> 1] >> ((p & 1) * 16)) & 0xFFFFu) : mine;
        const int mi = wave_mini_dpp(bv == wv ? static_cast<int>(mine) : 0x7FFFFFFF);
        wl = __ffsll(static_cast<long long>(__ballot((bv == wv) & (static_cast<int>(mine) == mi)))) - 1;
      }
      // the winning lane's slot index is wave-uniform: indexed register reads (s_set_gpr_idx)
      const int wp = __builtin_amdgcn_readlane(bp, wl);
      wi = static_cast<int>((static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(pidp[wp >> 1]), wl)) >>
                             ((wp & 1) * 16)) & 0xFFFFu);
      wx = readlane_t(px[wp], wl);
      wy = readlane_t(py[wp], wl);
      wz = readlane_t(pz[wp], wl);
      if constexpr (TIMING) ++nact;
    } else if constexpr (TIMING) {
      t1 = fps_clock();
    }
    FpsSlot<T>* buf = slots[step & 1];
    if (lane == 0) buf[wave] = FpsSlot<T>{empty_wave ? -2.0f : wv, empty_wave ? 0x7FFFFFFF : wi, wx, wy, wz};
    if constexpr (TIMING) t2 = fps_clock();
    lds_barrier();  // the output stores above stay in flight across the barrier
    uint64_t t3 = 0;
    if constexpr (TIMING) t3 = fps_clock();
    // block argmax over the W slots in lanes 0..W-1 (row 0): value desc, then index asc
    const FpsSlot<T> mine = buf[lane & (W - 1)];
    float v = mine.v;
    if constexpr (W > 1) v = dpp_maxf<0x111, 0x1>(v);
    if constexpr (W > 2) v = dpp_maxf<0x112, 0x1>(v);
    if constexpr (W > 4) v = dpp_maxf<0x114, 0x1>(v);
    if constexpr (W > 8) v = dpp_maxf<0x118, 0x1>(v);
    const float gv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), W - 1));
    const uint64_t tied = __ballot((lane < W) & (mine.v == gv));
    int ws;
    if ((tied & (tied - 1)) == 0) {
      ws = __ffsll(static_cast<long long>(tied)) - 1;
    } else {
      int ii = ((lane < W) & (mine.v == gv)) ? mine.i : 0x7FFFFFFF;
      if constexpr (W > 1) ii = dpp_mini<0x111, 0x1>(ii);
      if constexpr (W > 2) ii = dpp_mini<0x112, 0x1>(ii);
      if constexpr (W > 4) ii = dpp_mini<0x114, 0x1>(ii);
      if constexpr (W > 8) ii = dpp_mini<0x118, 0x1>(ii);
      const int mi = __builtin_amdgcn_readlane(ii, W - 1);
      ws = __ffsll(static_cast<long long>(__ballot((lane < W) & (mine.v == gv) & (mine.i == mi)))) - 1;
    }
    cur = __builtin_amdgcn_readlane(mine.i, ws);
    cx = readlane_t(mine.x, ws);
    cy = readlane_t(mine.y, ws);
    cz = readlane_t(mine.z, ws);
    if constexpr (TIMING) {
      const uint64_t t4 = fps_clock();
      ph[0] += t1 - t0;  // box test + point update
      ph[1] += t2 - t1;  // wave argmax + slot publish
      ph[2] += t3 - t2;  // barrier wait
      ph[3] += t4 - t3;  // slot reduction
    }
  }
  if constexpr (TIMING) {
    if (prof && lane == 0) {
      unsigned long long* o = prof + (static_cast<int64_t>(b) * W + wave) * kFpsProf;
      o[0] = ph[0];
      o[1] = ph[1];
      o[2] = ph[2];
      o[3] = ph[3];
      o[4] = nact;
      o[5] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);  // HW_ID: wave slot, SIMD, CU
      o[6] = static_cast<unsigned long long>(count);
      o[7] = 0;
    }
  }
}

// Step floor of the FPS chain (bench.py's latency roofline): fps_kernel's per-step
// synchronisation with no point work -- each wave's 64-lane DPP argmax + ballot, one LDS slot per
// wave, one barrier, the W-slot DPP reduction and readlanes -- each step's value depending on the
// previous step's winner, so the steps form one dependent chain as in FPS.
template <int W>
__global__ __launch_bounds__(W * kWave) void fps_floor_kernel(int steps, float* __restrict__ out) {
  __shared__ FpsSlot<float> slots[2][W];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float base = static_cast<float>(lane * 7 % 64) + 64.0f * static_cast<float>(wave * 3 % W);
  int cur = 0;
  for (int step = 0; step < steps; ++step) {
    const float bv = base + static_cast<float>(cur & 1) * 0.5f;
    const float wv = wave_maxf_dpp(bv);
    const uint64_t tied = __ballot(bv == wv);
    const int wl = __ffsll(static_cast<long long>(tied)) - 1;
    FpsSlot<float>* buf = slots[step & 1];
    if (lane == 0) buf[wave] = FpsSlot<float>{wv, wave * kWave + wl, 0.f, 0.f, 0.f};
    lds_barrier();
    const FpsSlot<float> mine = buf[lane & (W - 1)];
    float v = mine.v;
    if constexpr (W > 1) v = dpp_maxf<0x111, 0x1>(v);
    if constexpr (W > 2) v = dpp_maxf<0x112, 0x1>(v);
    if constexpr (W > 4) v = dpp_maxf<0x114, 0x1>(v);
    if constexpr (W > 8) v = dpp_maxf<0x118, 0x1>(v);
    const float gv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), W - 1));
    const int ws = __ffsll(static_cast<long long>(__ballot((lane < W) & (mine.v == gv)))) - 1;
    cur = __builtin_amdgcn_readlane(mine.i, ws) + step;
  }
  if (tid == 0) out[blockIdx.x] = static_cast<float>(cur);
}

// Dense fallback (no sort, no pruning) for clouds larger than the sorted kernel's VGPR budget.
template <typename T>
__global__ __launch_bounds__(kFpsThreads) void fps_dense_kernel(PointsView<T> pts, int N, int npoint,
                                                                const int64_t* __restrict__ start,
                                                                int64_t* __restrict__ out_idx, T* __restrict__ out_xyz,
                                                                float* __restrict__ ws) {
  constexpr int kDenseWaves = kFpsThreads / kWave;
  __shared__ FpsSlot<T> slots[2][kDenseWaves];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* dmin = ws + static_cast<int64_t>(b) * N;
  for (int n = tid; n < N; n += kFpsThreads) dmin[n] = 1e10f;
  int64_t cur = start[b];
  if (cur < 0 || cur >= N) cur = 0;
  T cx = pts.at(b, 0, cur), cy = pts.at(b, 1, cur), cz = pts.at(b, 2, cur);
  for (int step = 0; step < npoint; ++step) {
    if (tid == 0) {
      out_idx[static_cast<int64_t>(b) * npoint + step] = cur;
      if (out_xyz) {
        T* ox = out_xyz + static_cast<int64_t>(b) * 3 * npoint;
        ox[step] = cx;
        ox[npoint + step] = cy;
        ox[2 * npoint + step] = cz;
      }
    }
    float bv = -1.0f;
    int bi = 0x7FFFFFFF;
    for (int n = tid; n < N; n += kFpsThreads) {  // ascending n per thread: strict '>' keeps the lower index
      const T dx = pts.at(b, 0, n) - cx, dy = pts.at(b, 1, n) - cy, dz = pts.at(b, 2, n) - cz;
      const T d = (dx * dx + dy * dy) + dz * dz;
      float m = dmin[n];
      if (d < static_cast<T>(m)) {
        m = static_cast<float>(d);
        dmin[n] = m;
      }
      if (m > bv) {
        bv = m;
        bi = n;
      }
    }
    const float wvv = wave_maxf_dpp(bv);
    const int mi = wave_mini_dpp(bv == wvv ? bi : 0x7FFFFFFF);
    if (lane == 0) {
      slots[step & 1][wave].v = wvv;
      slots[step & 1][wave].i = mi;
    }
    __syncthreads();
    float gv = -2.0f;
    int gi = 0x7FFFFFFF;
    for (int w = 0; w < kDenseWaves; ++w) {
      const float v = slots[step & 1][w].v;
      const int i = slots[step & 1][w].i;
      if (v > gv || (v == gv && i < gi)) {
        gv = v;
        gi = i;
      }
    }
    cur = gi;
    cx = pts.at(b, 0, cur);
    cy = pts.at(b, 1, cur);
    cz = pts.at(b, 2, cur);
  }
}

// Split FPS for clouds above one CU's register budget (C5: 65536 points): S workgroups per cloud,
// each holding a contiguous chunk of P * NT points (coordinates and running minima in VGPRs, 512
// threads, P = 16 points per lane, or 32 for fp32 clouds above 131072 points).  Every step each workgroup updates its
// minima with the current centre and publishes its best point as one 64-bit key: the fp32 minimum's
// bits (monotonic for values >= 0), then the complemented index (18 bits), then the step's 14-bit
// tag -- so among one step's keys the maximum is the largest minimum with the lowest index, the
// dense kernel's and the reference's argmax rule.  Wave 0 of every workgroup then polls the cloud's
// S key slots, one lane per slot, until all carry this step's tag, and takes their maximum: one
// L2 round trip per poll, no arrival counter (round 4: the counter's release/acquire round trip
// plus a separate read of the keys made a step ~3.6 us).  Slots are double-buffered by step parity:
// a workgroup can only publish step + 2 after every peer has published step + 1, i.e. after every
// peer read step's keys; the slots start invalid (all ones: no minimum has those bits).
//
// Progress does not rest on the whole grid being co-resident.  A workgroup takes its (cloud,
// chunk) from a ticket counter when it starts running, not from blockIdx, so the tickets handed
// out so far cover whole clouds plus at most one partly started cloud per launch: a waiting
// workgroup only ever waits for peers of that one cloud, which take the next free slots on the
// device (S - 1 slots per concurrent launch).  The wait is still bounded (spin_cap polls) as a
// guard: a workgroup that gives up raises the launch's error word, which the host checks
// (dvcp/_lib.py check_device_flags), and writes the start point (index and coordinates) for the
// steps it could not finish, so nothing downstream reads out of bounds or a garbage centre.
constexpr int kFpsSplitMax = 16;
constexpr int kSplitTagBits = 14, kSplitIdxBits = 18;  // N <= 16 x 16384 points per cloud
constexpr uint64_t kSplitTagMask = (1ull << kSplitTagBits) - 1;
constexpr uint32_t kSplitIdxMask = (1u << kSplitIdxBits) - 1;

constexpr int kFpsSplitThreads = 512;  // (1024 threads x 16 points spilled 840 B at 128 VGPRs)
// Points per lane: 16 (chunks of 8192 points: twice the workgroups, half the per-step update)
// while that needs at most kFpsSplitMax workgroups per cloud; fp32 clouds above 131072 points take
// chunks of 16384.  (Chunks of 4096 ran one C5 launch in 19.4 instead of 22.3 ms, but with ten
// batches in flight their spinning workgroups cost the C5 bench 367.7 -> 288.5 pairs/s.)
template <typename T>
inline int fps_split_ppt(int N) {
  return sizeof(T) == 4 && ceil_div(N, 16 * kFpsSplitThreads) > kFpsSplitMax ? 32 : 16;
}
template <typename T>
constexpr int fps_split_max_chunk() { return (sizeof(T) == 4 ? 32 : 16) * kFpsSplitThreads; }

template <typename T, int P, int NT>
__global__ __launch_bounds__(NT) void fps_split_kernel(PointsView<T> pts, int N, int npoint, int S,
                                                       const int64_t* __restrict__ start,
                                                       int64_t* __restrict__ out_idx, T* __restrict__ out_xyz,
                                                       uint64_t* __restrict__ keys, uint32_t* __restrict__ ticket,
                                                       int32_t* __restrict__ err, uint32_t spin_cap) {
  constexpr int kW = NT / kWave;
  constexpr int chunk = P * NT;
  __shared__ uint64_t wbest[kW];
  __shared__ uint64_t gbest;
  __shared__ int timed_out;
  __shared__ uint32_t my_ticket;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) {
    my_ticket = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    timed_out = 0;
  }
  __syncthreads();
  const int b = static_cast<int>(my_ticket) / S, s = static_cast<int>(my_ticket) % S;
  const int n0 = s * chunk, n1 = min(N, n0 + chunk);
  T px[P], py[P], pz[P];
  float dm[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int n = n0 + p * NT + tid;
    const bool ok = n < n1;
    px[p] = ok ? pts.at(b, 0, n) : static_cast<T>(0);
    py[p] = ok ? pts.at(b, 1, n) : static_cast<T>(0);
    pz[p] = ok ? pts.at(b, 2, n) : static_cast<T>(0);
    dm[p] = 1e10f;
  }
  int64_t first = start[b];
  if (first < 0 || first >= N) first = 0;
  int64_t cur = first;
  T cx = pts.at(b, 0, cur), cy = pts.at(b, 1, cur), cz = pts.at(b, 2, cur);
  uint64_t* kb = keys + static_cast<int64_t>(b) * 2 * S;
  int step = 0;
  for (; step < npoint; ++step) {
    if (s == 0 && tid == 0) {
      out_idx[static_cast<int64_t>(b) * npoint + step] = cur;
      if (out_xyz) {
        T* ox = out_xyz + static_cast<int64_t>(b) * 3 * npoint;
        ox[step] = cx;
        ox[npoint + step] = cy;
        ox[2 * npoint + step] = cz;
      }
    }
    uint64_t best = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int n = n0 + p * NT + tid;
      const T dx = px[p] - cx, dy = py[p] - cy, dz = pz[p] - cz;
      const T d = (dx * dx + dy * dy) + dz * dz;
      float m = dm[p];
      if (d < static_cast<T>(m)) m = static_cast<float>(d);
      dm[p] = m;
      const uint64_t key = (static_cast<uint64_t>(__float_as_uint(m)) << 32) |
                           (static_cast<uint64_t>(kSplitIdxMask - static_cast<uint32_t>(n)) << kSplitTagBits);
      best = (n < n1 && key > best) ? key : best;
    }
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t o = __shfl_xor(best, off, kWave);
      best = o > best ? o : best;
    }
    if (lane == 0) wbest[wave] = best;
    __syncthreads();
    if (wave == 0) {
      const uint64_t tag = static_cast<uint64_t>(step) & kSplitTagMask;
      uint64_t* slot = kb + (step & 1) * S;
      if (lane == 0) {
        uint64_t wb = wbest[0];
        for (int w = 1; w < kW; ++w) wb = wbest[w] > wb ? wbest[w] : wb;
        __hip_atomic_store(slot + s, wb | tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      uint64_t v = 0;
      uint32_t polls = 0;
      for (;;) {
        v = lane < S ? __hip_atomic_load(slot + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        const bool ok = lane >= S || ((v & kSplitTagMask) == tag && static_cast<uint32_t>(v >> 32) != 0xFFFFFFFFu);
        if (__ballot(!ok) == 0) break;
        __builtin_amdgcn_s_sleep(1);
        if (++polls > spin_cap) {
          if (lane == 0) timed_out = 1;
          break;
        }
      }
      uint64_t g = lane < S ? v : 0ull;
      for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(g, off, kWave);
        g = o > g ? o : g;
      }
      if (lane == 0) gbest = g;
    }
    __syncthreads();
    if (timed_out) break;
    cur = static_cast<int64_t>(kSplitIdxMask - static_cast<uint32_t>((gbest >> kSplitTagBits) & kSplitIdxMask));
    cx = pts.at(b, 0, cur);
    cy = pts.at(b, 1, cur);
    cz = pts.at(b, 2, cur);
    __syncthreads();  // gbest / wbest are rewritten next step
  }
  if (step < npoint) {  // gave up waiting: flag the launch, keep every index and centre valid
    if (tid == 0) __hip_atomic_fetch_or(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (s == 0) {
      // the remaining steps repeat the start point: in-range indices AND finite centres, so the
      // ball query / MLP launched behind this one read real points before the host raises
      const T fx = pts.at(b, 0, first), fy = pts.at(b, 1, first), fz = pts.at(b, 2, first);
      T* ox = out_xyz ? out_xyz + static_cast<int64_t>(b) * 3 * npoint : nullptr;
      for (int k = step + tid; k < npoint; k += NT) {
        out_idx[static_cast<int64_t>(b) * npoint + k] = first;
        if (ox) {
          ox[k] = fx;
          ox[npoint + k] = fy;
          ox[2 * npoint + k] = fz;
        }
      }
    }
  }
}

// Workspace of the split kernel, carved from the caller's B x N fp32 buffer (>= 64 KiB per cloud):
// keys [B][2][S] u64 | ticket u32 | err i32 (err is the caller's when given).
struct FpsSplitWs {
  uint64_t* keys;
  uint32_t* ticket;
  int32_t* err;
};
static FpsSplitWs fps_split_ws(float* ws, int B, int S) {
  FpsSplitWs w;
  w.keys = reinterpret_cast<uint64_t*>(ws);
  w.ticket = reinterpret_cast<uint32_t*>(w.keys + static_cast<int64_t>(B) * 2 * S);
  w.err = reinterpret_cast<int32_t*>(w.ticket + 1);
  return w;
}

// Launch the split kernel over B clouds; `withhold` > 0 (tests only) launches that many fewer
// workgroups, so the last cloud never completes and its workgroups must give up.
template <typename T>
static int launch_fps_split(PointsView<T> v, int B, int N, int npoint, const int64_t* start, int64_t* out_idx,
                            T* out_xyz, float* ws, int32_t* err, uint32_t spin_cap, int withhold, hipStream_t st) {
  constexpr int NT = kFpsSplitThreads;
  const int P = fps_split_ppt<T>(N);
  const int S = ceil_div(N, P * NT);
  if (N > S * P * NT || N - 1 > static_cast<int>(kSplitIdxMask)) {
    set_error("dvcp_fps(split): N=%d too large", N);
    return DVCP_EINVAL;
  }
  FpsSplitWs w = fps_split_ws(ws, B, S);
  hipError_t e = hipMemsetAsync(w.keys, 0xFF, sizeof(uint64_t) * 2 * static_cast<size_t>(B) * S, st);  // invalid
  if (e == hipSuccess) e = hipMemsetAsync(w.ticket, 0, sizeof(uint32_t) * 2, st);
  if (e != hipSuccess) return launch_status("dvcp_fps(split memset)");
  if (!err) err = w.err;
  const int grid = B * S - withhold;
  if (grid > 0) {
    if (P == 16)
      hipLaunchKernelGGL((fps_split_kernel<T, 16, NT>), dim3(grid), dim3(NT), 0, st, v, N, npoint, S, start, out_idx,
                         out_xyz, w.keys, w.ticket, err, spin_cap);
    else if constexpr (sizeof(T) == 4)
      hipLaunchKernelGGL((fps_split_kernel<T, 32, NT>), dim3(grid), dim3(NT), 0, st, v, N, npoint, S, start, out_idx,
                         out_xyz, w.keys, w.ticket, err, spin_cap);
  }
  return launch_status("dvcp_fps(split)");
}

template <typename T>
int launch_fps_step(PointsView<T> v, int B, int N, int npoint, const int64_t* start, int64_t* out_idx, T* out_xyz,
                    hipStream_t st) {
  if (N <= 2 * kFpsThreads)
    hipLaunchKernelGGL((fps_kernel<T, kFpsThreads, 2, true>), dim3(B), dim3(kFpsThreads), 0, st, v, N, npoint, start,
                       out_idx, out_xyz, nullptr);
  else  // N < kFpsBatchedMinN = 4 * kFpsThreads
    hipLaunchKernelGGL((fps_kernel<T, kFpsThreads, 4, true>), dim3(B), dim3(kFpsThreads), 0, st, v, N, npoint, start,
                       out_idx, out_xyz, nullptr);
  return launch_status("dvcp_fps");
}
template int launch_fps_step<float>(PointsView<float>, int, int, int, const int64_t*, int64_t*, float*, hipStream_t);
template int launch_fps_step<double>(PointsView<double>, int, int, int, const int64_t*, int64_t*, double*, hipStream_t);

template <typename T>
int launch_fps_large(PointsView<T> v, int B, int N, int npoint, const int64_t* start, int64_t* out_idx, T* out_xyz,
                     float* ws, int32_t* err, hipStream_t st) {
  if (ceil_div(N, fps_split_max_chunk<T>()) <= kFpsSplitMax)
    return launch_fps_split<T>(v, B, N, npoint, start, out_idx, out_xyz, ws, err, kFpsSpinCap, 0, st);
  hipLaunchKernelGGL((fps_dense_kernel<T>), dim3(B), dim3(kFpsThreads), 0, st, v, N, npoint, start, out_idx, out_xyz,
                     ws);
  return launch_status("dvcp_fps(dense)");
}
template int launch_fps_large<float>(PointsView<float>, int, int, int, const int64_t*, int64_t*, float*, float*,
                                     int32_t*, hipStream_t);
template int launch_fps_large<double>(PointsView<double>, int, int, int, const int64_t*, int64_t*, double*, float*,
                                      int32_t*, hipStream_t);

}  // namespace dvcp

// bench.py: `blocks` workgroups of 512 threads each run the FPS step floor chain for `steps` steps.
extern "C" int dvcp_fps_step_floor(int steps, int blocks, float* out, void* stream) {
  DVCP_REQUIRE(out && steps >= 0 && blocks > 0 && blocks <= 65535, "dvcp_fps_step_floor: bad arguments");
  hipLaunchKernelGGL((dvcp::fps_floor_kernel<dvcp::kFpsThreads / dvcp::kWave>), dim3(blocks), dim3(dvcp::kFpsThreads),
                     0, static_cast<hipStream_t>(stream), steps, out);
  return dvcp::launch_status("dvcp_fps_step_floor");
}

// Test hook for the split kernel's guard: runs the split path with the given poll cap and
// `withhold` workgroups left out of the grid (so the last cloud cannot complete).
extern "C" int dvcp_fps_split_probe(int dtype, const void* xyz, int64_t sb, int64_t sc, int64_t sn, int B, int N,
                                    int npoint, const int64_t* start, int64_t* out_idx, void* out_xyz, float* ws,
                                    int32_t* err, uint32_t spin_cap, int withhold, void* stream) {
  DVCP_REQUIRE(xyz && start && out_idx && ws && err, "dvcp_fps_split_probe: null pointer");
  DVCP_REQUIRE(B > 0 && N > 0 && npoint > 0 && withhold >= 0, "dvcp_fps_split_probe: bad sizes");
  const int S = dvcp::ceil_div(N, (dtype == DVCP_F32 ? dvcp::fps_split_ppt<float>(N) : dvcp::fps_split_ppt<double>(N)) *
                                     dvcp::kFpsSplitThreads);
  DVCP_REQUIRE(S >= 2 && S <= dvcp::kFpsSplitMax && withhold < S, "dvcp_fps_split_probe: N=%d is not a split size", N);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == DVCP_F32)
    return dvcp::launch_fps_split<float>(dvcp::PointsView<float>{static_cast<const float*>(xyz), sb, sc, sn}, B, N,
                                         npoint, start, out_idx, static_cast<float*>(out_xyz), ws, err, spin_cap,
                                         withhold, st);
  if (dtype == DVCP_F64)
    return dvcp::launch_fps_split<double>(dvcp::PointsView<double>{static_cast<const double*>(xyz), sb, sc, sn}, B,
                                          N, npoint, start, out_idx, static_cast<double*>(out_xyz), ws, err, spin_cap,
                                          withhold, st);
  dvcp::set_error("dvcp_fps_split_probe: bad dtype %d", dtype);
  return DVCP_EINVAL;
}
