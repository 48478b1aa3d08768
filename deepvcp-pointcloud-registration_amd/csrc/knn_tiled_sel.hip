// knn_tiled_sel.hip -- the tiled kNN for k = 17..32, the forward's k = 32 (knn_tiled.hip has the
// overview): the wave's tile order (knn_wave_order), the buffered-selection kernel that scans it,
// and the probe kernel that writes the same order out for the tests.
//
// Buffered selection.  Same tiles and per-lane pruning as the insertion kernel (knn_tiled_insert.hip),
// with the wave's tile order from knn_wave_order below (buckets of the lower bound behind a
// certified bound, not a sort), and a lane does not insert each candidate into its sorted top-32
// as it appears (a 32-slot insertion network that the whole wave executes for every point that is
// a candidate for ANY lane: ~220 such steps per wave at C3, that kernel's cost at k = 32).
// Instead each lane appends its own candidates -- (d2, index) keys below its current k-th key --
// to a private 16-entry LDS buffer, and when some lane's buffer would overflow the wave merges:
// every lane sorts its buffer (16-key bitonic network in registers), folds it into its sorted
// top-32 (C[i] = min(top[i], buf[31 - i]) is bitonic and holds the 32 smallest keys; one
// 32-key bitonic merge sorts it) and re-reads its k-th key.  The wave then pays per merge, ~850
// VALU instructions for up to 16 candidates per lane, instead of ~160 per union candidate.
// Exactness is unchanged: the merged list is always the 32 smallest (d2, index) keys of every
// point appended, and a point is only left out when its key is not below a k-th key that is at
// least the true one (filters and pruning use the last merged, i.e. a stale-high, k-th key).
//
// Measured and not kept (DESIGN.md section 4.5 has the rest):
//  * Prefetching a tile's 256 bytes one sorted position ahead made every scanned tile wait for its
//    successor's load at the loop latch, ~660 clk per skipped tile by per-wave cycle counters
//    (round 3, profiles/round3/r3x_knn_diag_*.log): a tile is loaded once some lane needs it.
//  * An exact per-lane bulk test over each 64-position chunk -- every lane's tile box against all
//    64 queries of the wave -- 0.92 against 0.75 ms per C3 batch (round 4).
//  * Issuing the tile loads of 2 or 3 surviving positions together before their visits: 0.77 /
//    0.83 against 0.76 ms -- the scan is not waiting on those loads (round 4).
//  * One vector load and 48 readlanes per active tile instead of scalar loads: 0.763 / 0.755
//    against 0.751 / 0.742 ms per C3 call, identical results (round 4, tools/knn_bench.py --fast on
//    one box, profiles/round4/r4t/r4t_knn_sload_ab.log), although the 48 scalar values push the
//    kernel's register pressure (filtering in two 8-point batches, or re-loading the tile after a
//    merge instead of holding it, spilled 80-624 B).
//  * Output rows staged through LDS so that eight lanes store one row as 16-byte pieces: 0.776
//    against 0.749 ms with each lane storing its own rows (round 5, profiles/round5/r5n_*).
#include "knn_tiled_common.h"

namespace dvcp {

constexpr int kSelBufN = 16;   // buffer capacity per lane (>= kTile: a merge makes room for a whole tile)
constexpr int kSelSortN = 16;
constexpr int kSordWords = (kMaxTiles + 2) / 3;  // a wave's tile order, three 10-bit ids per word

// This lane's index, formed where it is used (an opaque v_mbcnt pair the compiler cannot hoist):
// a lane-dependent value held across the select kernel's scan was its last scratch spill.
__device__ __forceinline__ int knn_fresh_lane() {
  int r;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(r));
  return r;
}

// (d2, index) keys packed into doubles of [1, 2) (see knn_sel_query_kernel): 14 index bits
constexpr double kKeyEmpty = __builtin_bit_cast(double, 0x3FF0000000000000ull | (0x7F800000ull << 14) | 0x3FFFull);
__device__ __forceinline__ double key_pack(float d2, uint32_t index) {
  return __builtin_bit_cast(double, 0x3FF0000000000000ull | (static_cast<uint64_t>(__float_as_uint(d2)) << 14) |
                                        static_cast<uint64_t>(index & 0x3FFFu));
}
__device__ __forceinline__ float key_d2(double kd) {
  return __uint_as_float(static_cast<uint32_t>((__builtin_bit_cast(uint64_t, kd) >> 14) & 0x7FFFFFFFull));
}
__device__ __forceinline__ int key_index(double kd) {
  return static_cast<int>(__builtin_bit_cast(uint64_t, kd) & 0x3FFFull);
}
__device__ __forceinline__ void key_ce_f64(double& a, double& b, bool asc) {
  const double lo = __builtin_fmin(a, b), hi = __builtin_fmax(a, b);
  a = asc ? lo : hi;
  b = asc ? hi : lo;
}

// ---------------------------------------------------------------------------------------------
// The wave's tile order (knn_sel_query_kernel): a certified bound and two counting passes instead
// of a 1024-key bitonic sort.  The selection is exact for any visit order as long as no tile that
// can hold one of a lane's 32 nearest keys is left out; the order only makes the k-th distances
// converge early and carries the stop rule, so a bucket order is enough.
//
// Certificate.  ub(tile) is the far-corner distance between the wave's query box and the tile's
// outward-rounded half box, in the d2 expression's own shape: per axis f = max(fl(bh - wl),
// fl(wh - bl)) >= |fl(p - q)| for every point p of the tile and query q of the wave (rounding is
// monotone), so (fx*fx + fy*fy) + fz*fz, rounded the same way, is >= every computed d2; the
// (1 + 2^-20) margin on top pays for nothing the argument needs (as bq_prune_thr's).  A tile
// certifies when all its 16 slots are real points and its box is finite.  B0, the second smallest
// certified ub, then bounds the 32nd key of every live lane from above: two tiles, 32 points.  B0
// is +inf (nothing dropped) when fewer than two tiles certify (M < 32 among them) or a
// live query is not finite.
//
// Order.  A tile with lb > B0 is dropped: every computed d2 in it is above every lane's 32nd key,
// ties included.  The others are counting-sorted by knn_bucket(lb, top), the one expression
// used here and by the scan's stop rule; it is monotone in lb, so bucket(lb) > bucket(x) implies
// lb > x.  Inside a bucket the order is whatever the LDS adds return.
// (Starting every lane's k-th distance at B0 instead of +inf was measured too and changed
// nothing, 0.688-0.692 against 0.690-0.692 ms per C3 call: not kept.)
constexpr int kOrdBuckets = 256;  // counters per wave (a multiple of 64: four per lane)
constexpr int kOrdShift = 19;     // bucket = float bits >> 19: 16 buckets per octave of the bound
constexpr float kUbMargin = 1.0f + 0x1p-20f;

// Buckets are logarithmic: the bits of a non-negative float order like its value, so bits >> 19
// is monotone with 16 steps per octave, and the 256 buckets end at `top`, the step of the
// wave's range (B0, or the largest finite bound when B0 is inf).  They reach 16 octaves below
// it; whatever is lower, zero included, shares bucket 0, and whatever is above, +inf included,
// the last.  Integer arithmetic only: a zero range (every reference equal to the query) or an
// empty one cannot produce inf or NaN.  (Measured on the C3 micro-benchmark, DESIGN.md section
// 4.5: 64 buckets linear in the bound were no faster than the sort they replace -- the first
// tiles visited, far below B0, decide how fast the k-th distances fall, and they shared a bucket.)
__device__ __forceinline__ int knn_bucket_top(float range) {
  return static_cast<int>(__float_as_uint(range) >> kOrdShift);
}
__device__ __forceinline__ int knn_bucket(float lb, int top) {
  const int below = top - static_cast<int>(__float_as_uint(lb) >> kOrdShift);
  return max(0, kOrdBuckets - 1 - max(0, below));
}

// The wave's lower bound of a tile: hbox_lb2 against the wave's query box with the low 10 mantissa
// bits cleared (room for the tile id beside it in one register of the scan; clearing them only
// lowers a non-negative float, so it stays a lower bound and stays monotone).  The order, the drop
// rule and the scan all use this one value.
__device__ __forceinline__ float knn_tile_lb(const uint3& h, const float (&wl)[3], const float (&wh)[3]) {
  return __uint_as_float(__float_as_uint(hbox_lb2(h, wl[0], wl[1], wl[2], wh[0], wh[1], wh[2])) & ~kTileIdBits);
}

// Upper bound of the computed d2 between a point in box [a_lo, a_hi] and a point of the half box
// h (+inf when a corner of h is inf or NaN: fmaxf would drop a NaN side)
__device__ __forceinline__ float hbox_ub2(const uint3& h, float alx, float aly, float alz, float ahx, float ahy,
                                          float ahz) {
  const float blx = half_lo(h.x), bly = half_hi(h.x), blz = half_lo(h.y);
  const float bhx = half_hi(h.y), bhy = half_lo(h.z), bhz = half_hi(h.z);
  const float fx = fmaxf(bhx - alx, ahx - blx), fy = fmaxf(bhy - aly, ahy - bly), fz = fmaxf(bhz - alz, ahz - blz);
  const float u = ((fx * fx + fy * fy) + fz * fz) * kUbMargin;
  const float s = ((fabsf(blx) + fabsf(bly)) + fabsf(blz)) + ((fabsf(bhx) + fabsf(bhy)) + fabsf(bhz));
  return s < __builtin_huge_valf() ? u : __builtin_huge_valf();
}

// The wave's query box over its live lanes (wave-uniform: SGPRs); returns whether every live query
// is finite.
__device__ __forceinline__ bool knn_wave_box(bool live, float qx, float qy, float qz, float (&wl)[3], float (&wh)[3]) {
  const float q[3] = {qx, qy, qz};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = live ? q[a] : __builtin_huge_valf(), hi = live ? q[a] : -__builtin_huge_valf();
    wl[a] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(-wave_max_nonneg_signed(-lo))));
    wh[a] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(wave_max_nonneg_signed(hi))));
  }
  return __ballot(live && !((fabsf(qx) + fabsf(qy)) + fabsf(qz) < __builtin_huge_valf())) == 0;
}

struct WaveOrder {
  float b0;  // the certified bound (+inf: none)
  int top;   // knn_bucket's
  int kept;  // positions written to sordw
};

// Steps 1-2 for one wave.  hbox: the cloud's T half boxes (LDS); wl/wh: the wave's query box;
// qfinite: every live query is finite; cnt: kOrdBuckets words of wave-private LDS; sordw: the
// wave's kSordWords words, left holding `kept` tile ids in bucket order, three per word.
// lbv[r] returns the lower bound of tile r * 64 + lane (the probe's output).
template <int R>
__device__ __forceinline__ WaveOrder knn_wave_order(const uint3* hbox, int T, int M, const float (&wl)[3],
                                                    const float (&wh)[3], bool qfinite, uint32_t* cnt,
                                                    uint32_t* sordw, float (&lbv)[R]) {
  const int lane = threadIdx.x & 63;
  const float inf = __builtin_huge_valf();
  for (int i = lane; i < kSordWords; i += kWave) sordw[i] = 0u;
  constexpr int kPer = kOrdBuckets / kWave;  // consecutive counters per lane
#pragma unroll
  for (int j = 0; j < kPer; ++j) cnt[j * kWave + lane] = 0u;
  // this lane's tiles: lower bounds, the two smallest certified upper bounds, the largest bound
  float m1 = inf, m2 = inf, lbmax = 0.0f;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    lbv[r] = 0.0f;
    if (r * 64 < T) {
      const int t = r * 64 + lane;
      if (t < T) {
        const uint3 hb = hbox[t];
        lbv[r] = knn_tile_lb(hb, wl, wh);
        lbmax = fmaxf(lbmax, lbv[r] < inf ? lbv[r] : 0.0f);
        // (the padded last tile holds fewer than kTile points: no certificate)
        const float ub = (t + 1) * kTile <= M ? hbox_ub2(hb, wl[0], wl[1], wl[2], wh[0], wh[1], wh[2]) : inf;
        const float u = ub >= 0.0f ? ub : inf;  // (NaN: an empty wave box)
        m2 = fminf(m2, fmaxf(m1, u));
        m1 = fminf(m1, u);
      }
    }
  }
  WaveOrder o;
  {
    const float g1 = wave_min_nonneg(m1);
    const uint64_t own = __ballot(m1 == g1);
    const int owner = own ? __builtin_ctzll(own) : 0;
    const float g2 = wave_min_nonneg(lane == owner ? m2 : m1);
    o.b0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(qfinite ? g2 : inf)));  // (SGPRs)
  }
  o.top = __builtin_amdgcn_readfirstlane(knn_bucket_top(o.b0 < inf ? o.b0 : wave_max_nonneg(lbmax)));
  // pass 1: tiles per bucket
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (r * 64 < T) {
      const int t = r * 64 + lane;
      if (t < T && !(lbv[r] > o.b0)) atomicAdd(&cnt[knn_bucket(lbv[r], o.top)], 1u);
    }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // bucket bases: exclusive prefix sum over the wave (lane l owns counters l * kPer ..)
  {
    uint32_t c[kPer], sum = 0u;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      c[j] = cnt[lane * kPer + j];
      sum += c[j];
    }
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(incl), off, kWave));
      incl += lane >= off ? up : 0u;
    }
    o.kept = __builtin_amdgcn_readlane(static_cast<int>(incl), 63);
    __builtin_amdgcn_wave_barrier();
    uint32_t base = incl - sum;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      cnt[lane * kPer + j] = base;
      base += c[j];
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // pass 2: every kept tile takes a slot of its bucket
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (r * 64 < T) {
      const int t = r * 64 + lane;
      if (t < T && !(lbv[r] > o.b0)) {
        const uint32_t p = atomicAdd(&cnt[knn_bucket(lbv[r], o.top)], 1u);
        atomicOr(&sordw[p / 3], static_cast<uint32_t>(t) << (10 * (p % 3)));
      }
    }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return o;
}

// Every k in 17..32 selects the 32 nearest keys (the pruning bound is the 32nd) and writes the
// first k: ordered by (d^2, index), the first k of the 32 nearest are the k nearest.  (Round 5
// had a k < 32 instantiation bounding by the k-th key: its select loop over the slots cost 272 B
// of scratch per lane; k = 17..31 are test and API cases, the forward's k is 32.)
template <int R>
__global__ __launch_bounds__(kTiledThreads) __attribute__((amdgpu_waves_per_eu(3))) void knn_sel_query_kernel(const float4* __restrict__ sorted,
                                                                      const float4* __restrict__ tbox,
                                                                      const float4* __restrict__ qsorted, int M,
                                                                      int Q, int k,
                                                                      float* __restrict__ dist,
                                                                      int32_t* __restrict__ idx,
                                                                      int64_t* __restrict__ idx64, int B8) {
  constexpr int KT = 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int b = blockIdx.y, bx = blockIdx.x;
  if ((B8 & 1) != 0) {  // XCD-aware cloud mapping, as knn_tiled_query_kernel
    const int lin = static_cast<int>(blockIdx.y * gridDim.x + blockIdx.x);
    const int xo = lin & 7, slot = lin >> 3;
    b = xo + 8 * (slot / static_cast<int>(gridDim.x));
    bx = slot % static_cast<int>(gridDim.x);
  }
  const int T = (M + kTile - 1) / kTile;
  // 12 + 32 + 5.3 KB of LDS (half-precision boxes, candidate buffers, tile order): three
  // workgroups per CU
  __shared__ uint3 hbox[kMaxTiles];
  // each wave's tile order, three 10-bit tile ids per word (the chunked scan recomputes the bounds
  // from them: 16 registers of keys held across the scan spilled to scratch)
  __shared__ uint32_t sord[kTiledThreads / kWave][kSordWords];
  __shared__ double sbuf[kTiledThreads / kWave][kSelBufN][kWave];  // lane-private candidate buffers (packed keys)
  __shared__ float4 stile[kTiledThreads / kWave][kTile];            // the wave's current tile (appends)
  {
    const float4* tbg = tbox + static_cast<int64_t>(b) * T * 2;
    for (int i = threadIdx.x; i < T; i += kTiledThreads) hbox[i] = pack_hbox(tbg[2 * i], tbg[2 * i + 1]);
    __syncthreads();
  }
  // the wave's first curve position (wave-uniform) and this lane's
  const int sq0 = __builtin_amdgcn_readfirstlane((bx * (kTiledThreads / kWave) + wave) * kWave);
  const int sq = sq0 + lane;
  if (sq0 >= Q) return;  // whole wave past the end
  const bool live = sq < Q;
  // this lane's query in curve order: one coalesced 16-byte row (converted to fp32 by the scatter,
  // knn_cuda's .float())
  const float4 qrow = live ? qsorted[static_cast<int64_t>(b) * Q + sq] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float qx = qrow.x, qy = qrow.y, qz = qrow.z;
  // the query's output row index, re-read from its curve row where the rows are written (held
  // across the scan, it and the position were spilled)
  auto out_row = [&]() {
    const int sqn = sq0 + knn_fresh_lane();
    return __float_as_int(qsorted[static_cast<int64_t>(b) * Q + sqn].w);
  };
  float wl[3], wh[3];
  const bool qfinite = knn_wave_box(live, qx, qy, qz, wl, wh);
  // the wave's tile order in sord[wave] (the counters alias the candidate buffer, empty until the
  // scan starts)
  WaveOrder ord;
  {
    float lbv[R];
    ord = knn_wave_order<R>(hbox, T, M, wl, wh, qfinite, reinterpret_cast<uint32_t*>(sbuf[wave]), sord[wave], lbv);
  }

  // This lane's 32 smallest keys so far, ascending.  A key (d2, index) is packed into the mantissa
  // of a double in [1, 2): bits 0x3FF0'0000'0000'0000 | d2_bits << 14 | index (M <= 16384: 14 index
  // bits; non-negative d2 bits order like the values), so doubles order exactly like the keys and
  // a compare-exchange is one v_min_f64 + one v_max_f64 instead of a 64-bit compare and four selects.
  double tk[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) tk[t] = kKeyEmpty;
  float kth = live ? __builtin_huge_valf() : 0.0f;  // dead lanes never take a point
  float wkth = wave_max_nonneg(kth);
  int fill = 0;
  double(*mybuf)[kWave] = sbuf[wave];

  auto merge = [&]() {
    const int n = static_cast<int>(wave_umax_i(static_cast<uint32_t>(fill)));  // wave-uniform
    if (n == 0) return;
    double bk[kSelSortN];
#pragma unroll
    for (int i = 0; i < kSelSortN; ++i) {
      bk[i] = kKeyEmpty;
      if (i < kSelBufN && i < n) {
        const double e = mybuf[i][lane];
        bk[i] = i < fill ? e : bk[i];
      }
    }
    // bitonic sort of the 16 buffered keys, ascending
#pragma unroll
    for (int kk = 2; kk <= kSelSortN; kk <<= 1)
#pragma unroll
      for (int j = kk >> 1; j > 0; j >>= 1)
#pragma unroll
        for (int i = 0; i < kSelSortN; ++i) {
          const int l = i ^ j;
          if (l > i) key_ce_f64(bk[i], bk[l], (i & kk) == 0);
        }
    // C[i] = min(top[i], buf[31 - i]) (buf[16..31] = empty): bitonic, the 32 smallest keys
#pragma unroll
    for (int i = KT - kSelSortN; i < KT; ++i) tk[i] = __builtin_fmin(tk[i], bk[KT - 1 - i]);
    // bitonic merge, ascending
#pragma unroll
    for (int j = KT >> 1; j > 0; j >>= 1)
#pragma unroll
      for (int i = 0; i < KT; ++i) {
        const int l = i ^ j;
        if (l > i) key_ce_f64(tk[i], tk[l], true);
      }
    kth = live ? key_d2(tk[KT - 1]) : 0.0f;
    wkth = wave_max_nonneg(kth);
    fill = 0;
  };

  // (Per-wave cycle counters, round 3, C3: ~185 tiles pass the wave's bound, ~32 of them have a
  // lane within its own k-th distance, 11 merges = 20-24 % of the wave's clock.  Loading only the
  // tiles some lane needs, found by a look-ahead test, was slower: 0.97 -> 1.11 ms per call,
  // profiles/round3/r3x_knn_diag_*.log.)
  const float* P = reinterpret_cast<const float*>(sorted) + static_cast<int64_t>(b) * T * kTile * 4;
  // Visit tile `key` (its bound already known not to exceed wkth): the per-lane test, then the
  // distances, the filter and the appends.
  // (two lambdas, each taking the tile id from the key on its own: merged into one, the kernels'
  // machine code changes by an s_and, tools/kcmp.py)
  auto visit_bounded = [&](uint32_t key, float lbq) {
    const int t = static_cast<int>(key & kTileIdBits);
    const bool act = live & (lbq <= kth);
    if (__ballot(act) == 0) return;
    // An active tile's 16 points reach the wave as scalar loads (the tile index is wave-uniform,
    // the tile is read-only here); the appends, which index the tile per lane, load their LDS copy
    // from L2 when a lane needs one.
    float c[3 * kTile];
    {
      const float4* Pt = reinterpret_cast<const float4*>(P) + static_cast<int64_t>(t) * kTile;
#pragma unroll
      for (int j = 0; j < kTile; ++j) {
        const float4 pj = Pt[j];
        c[3 * j] = pj.x;
        c[3 * j + 1] = pj.y;
        c[3 * j + 2] = pj.z;
      }
    }
    // d2 is recomputed wherever it is needed (the same expression, the same bits) instead of
    // being held in 16 VGPRs across the merge and the appends
    auto d2_of = [&](int j) {
      const float dx = c[3 * j] - qx, dy = c[3 * j + 1] - qy, dz = c[3 * j + 2] - qz;
      return (dx * dx + dy * dy) + dz * dz;
    };
    uint32_t cm = 0;
    // Filter on the distance alone, d2 <= kf: a superset of the keys below the k-th key (a tie
    // with a higher index is appended too and dropped by the merge, which orders full keys);
    // kf is finite, so inf and NaN (padding) never pass, as in dvcp_knn.
    const float kf = fminf(kth, __builtin_bit_cast(float, 0x7F7FFFFFu));
#pragma unroll
    for (int j = 0; j < kTile; ++j) cm |= (act && d2_of(j) <= kf) ? (1u << j) : 0u;
    if (wave_umax_i(static_cast<uint32_t>(fill + __popc(cm))) > static_cast<uint32_t>(kSelBufN)) {
      merge();  // room for the whole tile; then re-filter against the new k-th key
      const float kf2 = fminf(kth, __builtin_bit_cast(float, 0x7F7FFFFFu));
#pragma unroll
      for (int j = 0; j < kTile; ++j) cm &= d2_of(j) <= kf2 ? ~0u : ~(1u << j);
    }
    // appends: each lane walks its own mask, reading its points from the wave's copy of the tile
    // in LDS (the wave loops max-over-lanes popc(mask) times instead of over the union of the
    // masks with four readlanes per point); the same d2 expression, the same bits
    if (__ballot(cm != 0) != 0) {  // wave-uniform: every lane writes its float of the tile
      reinterpret_cast<float*>(stile[wave])[lane] = P[static_cast<int64_t>(t) * (4 * kTile) + lane];
      __builtin_amdgcn_wave_barrier();
      uint32_t my = cm;
      while (__ballot(my != 0) != 0) {
        if (my != 0) {
          const int j = __builtin_ctz(my);
          my &= my - 1;
          const float4 pt = stile[wave][j];
          const float dx = pt.x - qx, dy = pt.y - qy, dz = pt.z - qz;
          mybuf[fill][lane] = key_pack((dx * dx + dy * dy) + dz * dz, __float_as_uint(pt.w));
          ++fill;
        }
      }
      __builtin_amdgcn_wave_barrier();  // (the next active tile rewrites stile)
    }
  };
  auto visit = [&](uint32_t key) {
    const int t = static_cast<int>(key & kTileIdBits);
    visit_bounded(key, hbox_lb2(hbox[t], qx, qy, qz, qx, qy, qz));
  };

  // Chunked scan.  The order is taken 64 positions at a time, one position per lane, and a
  // tile-parallel prefilter drops the positions no query can need: lane i tests its tile's box
  // against the boxes of the wave's kKnnSub lane groups (16 Hilbert-consecutive queries each) with
  // each group's largest k-th distance.  A position survives when some group's bound reaches its
  // k-th distance; only survivors get the per-lane test (visit).  The group bounds come from k-th
  // distances read at chunk start: merges only lower them, so a stale bound keeps a superset and
  // the scan stays exact; every surviving position is re-checked against the wave's current bound.
  constexpr int kKnnSub = 4, kSubLanes = kWave / kKnnSub;
  float gl[3] = {wl[0], wl[1], wl[2]}, gh[3] = {wh[0], wh[1], wh[2]};  // (overwritten below)
  {
    float a[3] = {live ? qx : __builtin_huge_valf(), live ? qy : __builtin_huge_valf(),
                  live ? qz : __builtin_huge_valf()};
    float z[3] = {live ? qx : -__builtin_huge_valf(), live ? qy : -__builtin_huge_valf(),
                  live ? qz : -__builtin_huge_valf()};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
#pragma unroll
      for (int off = kSubLanes / 2; off > 0; off >>= 1) {
        a[ax] = fminf(a[ax], __shfl_xor(a[ax], off, kWave));
        z[ax] = fmaxf(z[ax], __shfl_xor(z[ax], off, kWave));
      }
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      gl[ax] = a[ax];
      gh[ax] = z[ax];
    }
  }
  // every group's box, in LDS (read back as broadcasts per chunk: 24 wave-uniform values held in
  // registers across the scan would spill)
  __shared__ float4 sgbox[kTiledThreads / kWave][kKnnSub][2];
  if ((lane & (kSubLanes - 1)) == 0) {
    sgbox[wave][lane / kSubLanes][0] = make_float4(gl[0], gl[1], gl[2], 0.0f);
    sgbox[wave][lane / kSubLanes][1] = make_float4(gh[0], gh[1], gh[2], 0.0f);
  }
  // The order (sord[wave], ord.kept positions) is in buckets of the wave's lower bound, not
  // sorted inside one, so nothing here assumes a total order.  A position's bound is recomputed
  // from its tile id (the same expression as in knn_wave_order: the same bits).  A position is
  // needed iff its own bound does not exceed wkth; a bound above wkth at visit time skips that
  // position only.  The scan ends after a chunk whose last position's bucket is above wkth's:
  // every later tile has a bucket >= that one, and bucket(lb) > bucket(wkth) implies lb > wkth.
  bool stop = false;
#pragma unroll 1
  for (int base = 0; base < ord.kept && !stop; base += kWave) {
    const bool inr = base + lane < ord.kept;
    const int pos = base + lane;
    const int tt = inr ? static_cast<int>((sord[wave][pos / 3] >> (10 * (pos % 3))) & kTileIdBits) : 0;
    const uint3 hb = hbox[tt];
    const float mylb = knn_tile_lb(hb, wl, wh);  // lane i: position base + i
    const uint32_t mykey = __float_as_uint(mylb) | static_cast<uint32_t>(tt);
    const int blast = __builtin_amdgcn_readlane(knn_bucket(mylb, ord.top), min(kWave, ord.kept - base) - 1);
    // the groups' k-th distances (largest per group) as of now
    // (a row-wise DPP max of the non-negative bits, left in each group's last lane: no lane
    // addresses to hold across the scan)
    static_assert(kSubLanes == 16, "one DPP row per lane group");
    uint32_t gk = __float_as_uint(kth);
    gk = dpp_max_u<0x111, 0xF>(gk);
    gk = dpp_max_u<0x112, 0xF>(gk);
    gk = dpp_max_u<0x114, 0xF>(gk);
    gk = dpp_max_u<0x118, 0xF>(gk);
    float gks[kKnnSub];
#pragma unroll
    for (int g = 0; g < kKnnSub; ++g)
      gks[g] = __uint_as_float(static_cast<uint32_t>(
          __builtin_amdgcn_readlane(static_cast<int>(gk), g * kSubLanes + kSubLanes - 1)));
    const float blx = half_lo(hb.x), bly = half_hi(hb.x), blz = half_lo(hb.y);
    const float bhx = half_hi(hb.y), bhy = half_lo(hb.z), bhz = half_hi(hb.z);
    bool pass = false;
#pragma unroll
    for (int g = 0; g < kKnnSub; ++g) {
      const float4 lo = sgbox[wave][g][0], hi = sgbox[wave][g][1];
      pass |= box_box_lb2(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, blx, bly, blz, bhx, bhy, bhz) <= gks[g];
    }
    uint64_t cand = __ballot(pass && inr && !(mylb > wkth));
    while (cand) {
      const int i = __builtin_ctzll(cand);
      cand &= cand - 1ull;
      const uint32_t key = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(mykey), i));
      if (__uint_as_float(key & ~kTileIdBits) > wkth) continue;  // this tile only: a later one may be nearer
      visit(key);
    }
    stop = blast > knn_bucket(wkth, ord.top);
  }
  merge();
  if (dist && idx && !idx64 && k == KT) {
    // the forward's case: each lane writes its own 128-B rows as eight 16-byte stores (whole lines
    // per lane)
    if (!live) return;
    const int qo = out_row();
    float4* dr = reinterpret_cast<float4*>(dist + (static_cast<int64_t>(b) * Q + qo) * 32);
    int4* ir = reinterpret_cast<int4*>(idx + (static_cast<int64_t>(b) * Q + qo) * 32);
#pragma unroll
    for (int v = 0; v < KT / 4; ++v) {
      float dv[4];
      int iv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double kv = tk[4 * v + e];
        const bool ok = kv != kKeyEmpty;
        dv[e] = ok ? sqrt_rn(key_d2(kv)) : __builtin_huge_valf();
        iv[e] = ok ? key_index(kv) : -1;
      }
      dr[v] = make_float4(dv[0], dv[1], dv[2], dv[3]);
      ir[v] = make_int4(iv[0], iv[1], iv[2], iv[3]);
    }
    return;
  }
  if (!live) return;
  // the query's output row (its index re-read: held across the scan it was spilled)
  const int qo = out_row();
  const int64_t o = (static_cast<int64_t>(b) * Q + qo) * k;
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    if (t < k) {
      const bool ok = tk[t] != kKeyEmpty;  // fewer than k finite points
      const float d2 = key_d2(tk[t]);
      const int i = key_index(tk[t]);
      if (dist) dist[o + t] = ok ? sqrt_rn(d2) : __builtin_huge_valf();
      if (idx) idx[o + t] = ok ? i : -1;
      if (idx64) idx64[o + t] = ok ? i : -1;
    }
  }
}

// Test hook (dvcp_knn_tiled_order_probe): knn_sel_query_kernel's wave box and tile order for every
// wave, written out instead of scanned.  Row = cloud * ceil(Q / 64) + wave of the curve order.
template <int R>
__global__ __launch_bounds__(kTiledThreads) void knn_order_probe_kernel(const float4* __restrict__ tbox,
                                                                        const float4* __restrict__ qsorted, int M,
                                                                        int Q, int32_t* __restrict__ info,
                                                                        int32_t* __restrict__ order,
                                                                        float* __restrict__ lbs,
                                                                        int32_t* __restrict__ buckets, int B8) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int b = blockIdx.y, bx = blockIdx.x;
  if ((B8 & 1) != 0) {  // XCD-aware cloud mapping, as knn_sel_query_kernel
    const int lin = static_cast<int>(blockIdx.y * gridDim.x + blockIdx.x);
    const int xo = lin & 7, slot = lin >> 3;
    b = xo + 8 * (slot / static_cast<int>(gridDim.x));
    bx = slot % static_cast<int>(gridDim.x);
  }
  const int T = (M + kTile - 1) / kTile;
  __shared__ uint3 hbox[kMaxTiles];
  __shared__ uint32_t sord[kTiledThreads / kWave][kSordWords];
  __shared__ uint32_t scnt[kTiledThreads / kWave][kOrdBuckets];
  {
    const float4* tbg = tbox + static_cast<int64_t>(b) * T * 2;
    for (int i = threadIdx.x; i < T; i += kTiledThreads) hbox[i] = pack_hbox(tbg[2 * i], tbg[2 * i + 1]);
    __syncthreads();
  }
  const int sq0 = __builtin_amdgcn_readfirstlane((bx * (kTiledThreads / kWave) + wave) * kWave);
  const int sq = sq0 + lane;
  if (sq0 >= Q) return;
  const bool live = sq < Q;
  const float4 qrow = live ? qsorted[static_cast<int64_t>(b) * Q + sq] : make_float4(0.f, 0.f, 0.f, 0.f);
  float wl[3], wh[3];
  const bool qfinite = knn_wave_box(live, qrow.x, qrow.y, qrow.z, wl, wh);
  float lbv[R];
  const WaveOrder ord = knn_wave_order<R>(hbox, T, M, wl, wh, qfinite, scnt[wave], sord[wave], lbv);
  const int64_t row = static_cast<int64_t>(b) * ((Q + kWave - 1) / kWave) + sq0 / kWave;
  if (lane == 0) {
    info[row * 4 + 0] = T - ord.kept;
    info[row * 4 + 1] = ord.kept;
    info[row * 4 + 2] = ord.b0 < __builtin_huge_valf() ? 1 : 0;
    info[row * 4 + 3] = __float_as_int(ord.b0);
  }
  for (int p = lane; p < T; p += kWave)
    order[row * T + p] = p < ord.kept ? static_cast<int>((sord[wave][p / 3] >> (10 * (p % 3))) & kTileIdBits) : -1;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int t = r * 64 + lane;
    if (t < T) {
      lbs[row * T + t] = lbv[r];
      buckets[row * T + t] = lbv[r] > ord.b0 ? -1 : knn_bucket(lbv[r], ord.top);
    }
  }
}

int knn_sel_launch(const TiledLayout& L, int M, int Q, int B, int k, float* dist, int32_t* idx, int64_t* idx64,
                   hipStream_t st) {
  const dim3 grid(ceil_div(Q, kTiledThreads), B);
  const int xcd = B % 8 == 0 ? 1 : 0;  // XCD-aware cloud mapping (equal clouds per XCD)
  return knn_for_tile_regs(ceil_div(M, kTile), [&](auto r) {
    hipLaunchKernelGGL((knn_sel_query_kernel<decltype(r)::value>), grid, dim3(kTiledThreads), 0, st, L.sorted,
                       L.tbox, L.qsorted, M, Q, k, dist, idx, idx64, xcd);
    return launch_status("dvcp_knn_tiled(select)");
  });
}

int knn_order_probe_launch(const TiledLayout& L, int M, int Q, int B, int32_t* info, int32_t* order, float* lb,
                           int32_t* bucket, hipStream_t st) {
  const dim3 grid(ceil_div(Q, kTiledThreads), B);
  const int xcd = B % 8 == 0 ? 1 : 0;
  return knn_for_tile_regs(ceil_div(M, kTile), [&](auto r) {
    hipLaunchKernelGGL((knn_order_probe_kernel<decltype(r)::value>), grid, dim3(kTiledThreads), 0, st, L.tbox,
                       L.qsorted, M, Q, info, order, lb, bucket, xcd);
    return launch_status("dvcp_knn_tiled_order_probe");
  });
}

}  // namespace dvcp
