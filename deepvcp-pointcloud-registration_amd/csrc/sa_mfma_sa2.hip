// sa_mfma_sa2.hip -- the sa2 table (35-32-64) with a workspace: the grouped kernel behind
// sa_pre_mfma_kernel's U rows (sa_mfma_common.h has the layers and the pipeline).
#include "sa_mfma_common.h"

namespace dvcp {

// Held at four waves per SIMD (left at "three or more" it takes 132 VGPRs once the split's
// subtractions stay scalar; held, the fp32 instance fits 128 without scratch, the fp64-coordinate
// one spills one 8-byte loop invariant outside the tile loop).
// feat, fb, fn: unused (the parameter list of sa_plain_mfma_kernel)
template <typename T, int D, int C1, int C2>
__global__ __launch_bounds__(kMfmaWaves * kWave) __attribute__((amdgpu_waves_per_eu(4))) void sa2_mfma_kernel(
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
  // are gathered through the entry loaded one step earlier into a second register set ahead of
  // tile t's MFMAs, the two sets alternating by a two-step unrolled loop.  The pipeline is primed
  // at the start of every 64-centre batch and drains at its end; loads past the last tile go
  // through a valid tile's indices and are dropped.
  for (int64_t qc = q0; qc < total; qc += 64 * qs) {
    const int64_t qm = qc + lane * qs;
    int m_b = 0, m_rows = 0;  // rows 0: no hit (the centre's output is 0)
    int64_t m_fc = 0;
    T m_cx = T(0), m_cy = T(0), m_cz = T(0);
    sa_centre_meta(qm, total, xcd, xo, S, order, count, nsample, ctr, m_b, m_rows, m_fc, m_cx, m_cy, m_cz);
    const int ncen = static_cast<int>(min<int64_t>(64, (total - qc + qs - 1) / qs));
    // Rows in 16-row half tiles: a tile takes the next two half tiles of the wave's centres in
    // order (rows 0-15 are accumulator registers 0..7 of both lane halves, rows 16-31 registers
    // 8..15), so a centre wastes at most 15 padded rows instead of 31, and the two halves' maxima
    // fold into running per-centre maxima in order.  Padded rows repeat the centre's first hit.
    int js = 0, hs = 0;  // the next half tile: centre js, half hs
    auto nh_of = [&](int jj) { return max(1, (lane_bcast(m_rows, jj) + 15) >> 4); };
    int nhj = ncen > 0 ? nh_of(0) : 0;
    int runj = -1;
    float run[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) run[ct] = 0.0f;
    auto flush = [&]() {
      const int64_t fcr = lane_bcast(m_fc, runj);
      const bool empty = lane_bcast(m_rows, runj) == 0;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        if (h == 0) out[fcr * C2 + 32 * ct + r32] = empty ? 0.0f : fmaxf(run[ct] + b2[ct], 0.0f);
    };
    auto fold = [&](int jj, const float (&m)[CT]) {
      if (jj != runj) {
        if (runj >= 0) flush();
        runj = jj;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) run[ct] = m[ct];
      } else {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) run[ct] = fmaxf(run[ct], m[ct]);
      }
    };
    // This lane's point is row r32 of the tile: its centre is the first or the second half tile's.
    // The centre's metadata comes by one ds_bpermute per value through the selected lane index.
    const bool sB = r32 >= 16;
    struct Gathered {  // what a tile waits for: the accumulator start (its U row) and its point
      f32x16 u[MT];
      T px, py, pz;
    };
    // stage 1: the list entry of this lane's row
    auto entry = [&](const HalfPair& t) { return half_pair_entry(t, m_fc, m_rows, r32, count, list, nsample); };
    // stage 2: the U row and the point behind list entry ne
    auto gather = [&](const HalfPair& t, int ne, Gathered& g) {
      const int jl = sB ? t.jB : t.jA;
      const int b = lane_gather(m_b, jl);
      const int n = lane_gather(m_rows, jl) == 0 ? 0 : ne;
      const float4* ur = sa_u_row<C1>(U, ub, b, n, h);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) sa_gather_u(ur, mt, g.u[mt]);
      // (points in packed (x, y, z, pad) rows measured no faster here -- sa2 0.298 -> 0.306, sa3
      // 0.594 -> 0.597 ms, r5ae_sa_p4_bench.log: the U rows dominate the gather -- so the FE passes
      // the (B, 3, N) layout; load3 takes either)
      pts.load3(b, n, g.px, g.py, g.pz);
    };
    // stage 3: the tile's MFMAs, split-3 and maxima
    auto compute = [&](const HalfPair& t, const Gathered& g) {
      int zo = 0;
      asm volatile("" : "+v"(zo));
      const int jl = sB ? t.jB : t.jA;
      const T cx = lane_gather(m_cx, jl), cy = lane_gather(m_cy, jl), cz = lane_gather(m_cz, jl);
      f32x16 acc1[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc1[mt] = g.u[mt];
      sa_layer1_xyz(acc1, g.px, g.py, g.pz, cx, cy, cz, h, L.wx, lane + zo);
      f32x16 acc2[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[ct][r] = 0.0f;
      sa_layer2<MT, CT, false>(acc1, acc2, [&](int ct, int st, int pc) { return L.w2s[ct][st][pc][lane + zo]; }, [](int) {});
      float mA[CT], mB[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        float a0 = acc2[ct][0], a1 = acc2[ct][8];
#pragma unroll
        for (int r = 1; r < 8; ++r) {
          a0 = fmaxf(a0, acc2[ct][r]);
          a1 = fmaxf(a1, acc2[ct][8 + r]);
        }
        mA[ct] = fmaxf(a0, __shfl_xor(a0, 32, kWave));
        mB[ct] = fmaxf(a1, __shfl_xor(a1, 32, kWave));
      }
      fold(t.jA, mA);
      if (t.hasB) fold(t.jB, mB);
    };
    // (The driver from here on is sa1's too.  As one function that takes the three stages it
    // changed the register numbering and branch offsets of both kernels.)
    auto next = [&]() { return next_half_pair(js, hs, nhj, ncen, nh_of); };
    // prime: tiles 0 and 1 named, their list entries loaded, tile 0 gathered
    HalfPair t0 = next(), t1 = next();
    Gathered ga, gb;
    int na = entry(t0), nb = entry(t1);  // the list entries alternate like the register sets
    gather(t0, na, ga);
    // one step: nuse is the list entry of tile t + 1 (loaded one step ago), nload takes tile t + 2's
    auto step = [&](const Gathered& cur, Gathered& nxt, int nuse, int& nload) {
      const HalfPair t2 = next();
      nload = entry(t2);
      gather(t1, nuse, nxt);
      __builtin_amdgcn_sched_barrier(0);  // the loads above stay ahead of the tile's MFMAs
      compute(t0, cur);
      t0 = t1;
      t1 = t2;
    };
    do {  // ncen >= 1: tile 0 exists
      step(ga, gb, nb, na);
      if (!t0.live) break;
      step(gb, ga, na, nb);
    } while (t0.live);
    if (runj >= 0) flush();
  }
}

template <typename T>
void launch_sa2_mfma(const SaTableArgs<T>& a, hipStream_t st) {
  const SaGrid g(a.B, a.S);
  hipLaunchKernelGGL((sa2_mfma_kernel<T, 32, 32, 64>), dim3(g.grid), dim3(kMfmaWaves * kWave), 0, st, a.pts, a.ctr,
                     a.S, a.B, a.feat, a.fb, a.fn, a.count, a.list, a.nsample, a.params, a.U, a.ub, a.order, a.out,
                     g.xcd);
}
template void launch_sa2_mfma<float>(const SaTableArgs<float>&, hipStream_t);
template void launch_sa2_mfma<double>(const SaTableArgs<double>&, hipStream_t);

}  // namespace dvcp
