// sa_mfma_sa3.hip -- the sa3 table (67-64-64) with a workspace: the grouped kernel behind
// sa_pre_mfma_kernel's U rows (sa_mfma_common.h has the layers).
#include "sa_mfma_common.h"

namespace dvcp {

// 32-row tiles, not sa2's 16-row half tiles: A/B on one box (tools/sa_bench.py, r4q) sa2 0.312 ->
// 0.299 ms with half tiles, sa3 0.626 -> 0.659 ms (its balls mostly fill whole 32-row tiles; the
// half-tile bookkeeping costs more).  Takes the waves it needs (132 VGPRs, three per SIMD, see
// sa_layer2).
// feat, fb, fn: unused (the parameter list of sa_plain_mfma_kernel)
template <typename T, int D, int C1, int C2>
__global__ __launch_bounds__(kMfmaWaves * kWave) __attribute__((amdgpu_waves_per_eu(3))) void sa3_mfma_kernel(
    PointsView<T> pts, PointsView<T> ctr, int S, int B, const float* __restrict__ feat, int64_t fb, int64_t fn,
    const int32_t* __restrict__ count, const int32_t* __restrict__ list, int nsample,
    const float* __restrict__ params, const float* __restrict__ U, int64_t ub, const int32_t* __restrict__ order,
    float* __restrict__ out, int xcd) {
  using Sh = SaMfmaShape<D, C1, C2>;
  constexpr int C0 = Sh::C0, MT = Sh::MT, CT = Sh::CT;
  __shared__ SaMfmaLds<D, C1, C2> L;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r32 = lane & 31;
  // wave-uniform by construction; said so, the centre walk below stays in scalar registers and branches
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- stage the weights (params: W1, b1, scale1, shift1, W2, b2, scale2, shift2) ---------
  const float* W1 = params;
  const float* pb1 = W1 + C1 * C0;
  const float* ps1 = pb1 + C1;
  const float* pt1 = ps1 + C1;
  const float* W2 = pt1 + C1;
  const float* pb2 = W2 + C2 * C1;
  const float* ps2 = pb2 + C2;
  const float* pt2 = ps2 + C2;
  for (int i = tid; i < MT * 2 * 64; i += blockDim.x) {
    const int l = i % 64, s = (i / 64) % 2, mt = i / 128;
    const int ch = s == 0 ? (l >> 5) : ((l >> 5) == 0 ? 2 : -1);
    L.wx[mt][s][l] = ch < 0 ? 0.0f : W1[(32 * mt + (l & 31)) * C0 + ch] * ps1[32 * mt + (l & 31)];
  }
  // k-step s, lane half hh, element j <-> layer-1 channel 32 (s / 2) + acc_row(8 (s % 2) + j, hh): the
  // layer-1 accumulator registers 8 (s % 2) .. + 7 of tile s / 2 are the A fragment as they stand
  for (int i = tid; i < CT * Sh::KB * 64; i += blockDim.x) {
    const int l = i % 64, s = (i / 64) % Sh::KB, ct = i / (64 * Sh::KB);
    const int o = 32 * ct + (l & 31);
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      w[j] = W2[o * C1 + 32 * (s / 2) + acc_row(8 * (s % 2) + j, l >> 5)] * ps2[o];
    const Split3 ws = split3(w);
    L.w2s[ct][s][0][l] = ws.p0;
    L.w2s[ct][s][1][l] = ws.p1;
    L.w2s[ct][s][2][l] = ws.p2;
  }
  for (int i = tid; i < MT * 32; i += blockDim.x) {
    const int r = i % 16, hh = (i / 16) % 2, mt = i / 32;
    const int c = 32 * mt + acc_row(r, hh);
    L.b1[mt][hh][r] = pb1[c];
    L.s1[mt][hh][r] = ps1[c];
    L.t1[mt][hh][r] = pt1[c];
  }
  float b2[CT], s2[CT], t2[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    b2[ct] = pb2[32 * ct + r32];
    s2[ct] = ps2[32 * ct + r32];
    t2[ct] = pt2[32 * ct + r32];
    // BN2 folded into W2 (above) and the bias: (W h + b) s + t = (s W) h + (s b + t)
    b2[ct] = static_cast<float>(static_cast<double>(b2[ct]) * s2[ct] + static_cast<double>(t2[ct]));
  }
  __syncthreads();

  // ---- one centre per wave, grid-strided over the centre index space (sa_mfma_common.h) ------
  int xo = 0;
  int64_t q0, qs, total;
  if (xcd) {
    xo = static_cast<int>(blockIdx.x) & 7;
    total = static_cast<int64_t>((B - xo + 7) / 8) * S;
    q0 = static_cast<int64_t>(blockIdx.x >> 3) * kMfmaWaves + wave;
    qs = static_cast<int64_t>(gridDim.x >> 3) * kMfmaWaves;
  } else {
    total = static_cast<int64_t>(B) * S;
    q0 = static_cast<int64_t>(blockIdx.x) * kMfmaWaves + wave;
    qs = static_cast<int64_t>(gridDim.x) * kMfmaWaves;
  }
  // A three-stage software pipeline over each 64-centre batch's flat tile sequence: while tile t
  // runs its MFMAs, the list entry of tile t + 2 is loaded, and the U row and point of tile t + 1
  // are gathered through the entry loaded one step earlier into the freed layer-1 registers during
  // tile t's last MFMAs.  The pipeline is primed at the start of every 64-centre batch and drains
  // at its end; loads past the last tile go through a valid tile's indices and are dropped.
  for (int64_t qc = q0; qc < total; qc += 64 * qs) {
    const int64_t qm = qc + lane * qs;
    int m_b = 0, m_rows = 0;  // rows 0: no hit (the centre's output is 0)
    int64_t m_fc = 0;
    T m_cx = T(0), m_cy = T(0), m_cz = T(0);
    sa_centre_meta(qm, total, xcd, xo, S, order, count, nsample, ctr, m_b, m_rows, m_fc, m_cx, m_cy, m_cz);
    const int ncen = static_cast<int>(min<int64_t>(64, (total - qc + qs - 1) / qs));
    // 32-row tiles, one centre at a time (sa3).  The flat sequence is every tile of every centre
    // with hits, in order (lane mask of the batch); a centre without hits runs no tile, reads no
    // list entry and gets its zeros here.  Past the last tile the walk names the first tile of
    // the last centre with hits.
    // With two 16-register accumulator starts per tile a second register set costs a wave per SIMD
    // (148 VGPRs, 3 waves), so this path keeps one set: tile t + 1's U row is loaded into layer
    // 1's accumulator registers once tile t's last split-3 has read them, and arrives under the
    // tile's last MFMAs and its maximum (128 VGPRs, 4 waves).  List entries still run two tiles
    // ahead.
    const uint64_t live_c = __ballot(lane < ncen && m_rows > 0);
    for (uint64_t e = __ballot(lane < ncen && m_rows == 0); e; e &= e - 1) {
      const int64_t fce = lane_bcast(m_fc, static_cast<int>(__builtin_ctzll(e)));
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        if (h == 0) out[fce * C2 + 32 * ct + r32] = 0.0f;
    }
    if (live_c == 0) continue;
    const int jlast = 63 - static_cast<int>(__builtin_clzll(live_c));
    struct Tile {
      int j, n0;  // centre (lane of the batch) and first row
      bool live;
    };
    int cj = static_cast<int>(__builtin_ctzll(live_c)), cn = 0;  // the next tile to name; cj 64: none left
    auto next = [&]() {
      Tile t;
      t.live = cj < 64;
      if (!t.live) {
        t.j = jlast;
        t.n0 = 0;
        return t;
      }
      t.j = cj;
      t.n0 = cn;
      if (cn + 32 < lane_bcast(m_rows, cj)) {
        cn += 32;
      } else {
        const uint64_t m = cj >= 63 ? 0ull : (live_c & (~0ull << (cj + 1)));
        cj = m ? static_cast<int>(__builtin_ctzll(m)) : 64;
        cn = 0;
      }
      return t;
    };
    struct Gathered {  // what a tile waits for: the accumulator start (its U row) and its point
      f32x16 u[MT];
      T px, py, pz;
    };
    // stage 1: the list entry of this lane's row (padded rows repeat the first hit); only centres
    // with hits are named, so rows >= 1
    auto entry = [&](const Tile& t) {
      const int64_t fc = lane_bcast(m_fc, t.j);
      const int row = t.n0 + r32;
      return list[fc * nsample + (row < lane_bcast(m_rows, t.j) ? row : 0)];
    };
    // stage 2: the U row (channels (r&3) + 8(r>>2) + 4h of each 32-channel tile, one 32-channel
    // tile per call) and the point behind list entry n
    auto gather_u = [&](const Tile& t, int n, Gathered& g, int mt) {
      sa_gather_u(sa_u_row<C1>(U, ub, lane_bcast(m_b, t.j), n, h), mt, g.u[mt]);
    };
    auto gather_p = [&](const Tile& t, int n, Gathered& g) { pts.load3(lane_bcast(m_b, t.j), n, g.px, g.py, g.pz); };
    // The accumulators of layer 2 start from zero (an inline-constant C operand) and the bias is
    // added once to the centre's maximum: max_i fl(a_i + b) = fl(max_i a_i + b) (rounding is
    // monotone), then the ReLU (max_i relu(v_i) = relu(max_i v_i)).
    float mx[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) mx[ct] = -__builtin_huge_valf();
    // stage 3: the tile's MFMAs, split-3 and maximum; the centre's row goes out after its last tile.
    // refill(mt) is called once layer 1's registers of channel tile mt have been read for the last time.
    auto compute = [&](const Tile& t, const Gathered& g, auto refill) {
      // An opaque zero added to every LDS weight index: the fragments are re-read per tile
      // (one ds_read per MFMA) instead of being hoisted out of the loop into ~100 registers.
      int zo = 0;
      asm volatile("" : "+v"(zo));
      const T cx = lane_bcast(m_cx, t.j), cy = lane_bcast(m_cy, t.j), cz = lane_bcast(m_cz, t.j);
      f32x16 acc1[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc1[mt] = g.u[mt];
      sa_layer1_xyz(acc1, g.px, g.py, g.pz, cx, cy, cz, h, L.wx, lane + zo);
      f32x16 acc2[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[ct][r] = 0.0f;
      sa_layer2<MT, CT, true>(acc1, acc2, [&](int ct, int st, int pc) { return L.w2s[ct][st][pc][lane + zo]; }, refill);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx[ct] = fmaxf(mx[ct], acc2[ct][r]);
      if (t.n0 + 32 >= lane_bcast(m_rows, t.j)) {
        const int64_t fc = lane_bcast(m_fc, t.j);
        // the two lane halves hold different points of the same channel
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
          const float m = fmaxf(fmaxf(mx[ct], __shfl_xor(mx[ct], 32, kWave)) + b2[ct], 0.0f);
          if (h == 0) out[fc * C2 + 32 * ct + r32] = m;
          mx[ct] = -__builtin_huge_valf();
        }
      }
    };
    // prime: tiles 0 and 1 named, their list entries loaded, tile 0 gathered
    Tile t0 = next(), t1 = next();
    Gathered g;
    int na = entry(t0), nb = entry(t1);  // two registers, alternating by the two-step unrolled loop
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) gather_u(t0, na, g, mt);
    gather_p(t0, na, g);
    // one step: nuse is the list entry of tile t + 1 (loaded one step ago), nload takes tile t + 2's
    auto step = [&](int nuse, int& nload) {
      const Tile t2 = next();
      nload = entry(t2);
      compute(t0, g, [&](int mt) {
        gather_u(t1, nuse, g, mt);
        if (mt == MT - 1) gather_p(t1, nuse, g);
      });
      t0 = t1;
      t1 = t2;
    };
    do {  // live_c != 0: tile 0 exists
      step(nb, na);
      if (!t0.live) break;
      step(na, nb);
    } while (t0.live);
  }
}

template <typename T>
void launch_sa3_mfma(const SaTableArgs<T>& a, hipStream_t st) {
  const SaGrid g(a.B, a.S);
  hipLaunchKernelGGL((sa3_mfma_kernel<T, 64, 64, 64>), dim3(g.grid), dim3(kMfmaWaves * kWave), 0, st, a.pts, a.ctr,
                     a.S, a.B, a.feat, a.fb, a.fn, a.count, a.list, a.nsample, a.params, a.U, a.ub, a.order, a.out,
                     g.xcd);
}
template void launch_sa3_mfma<float>(const SaTableArgs<float>&, hipStream_t);
template void launch_sa3_mfma<double>(const SaTableArgs<double>&, hipStream_t);

}  // namespace dvcp
