// sa_mfma_sa1.hip -- the three-layer set-abstraction table (sa1: 3-16-16-32 on xyz, 6-16-16-32 with
// normals; deep_feat_extraction.py:19, pointnet2_utils.py:122-132 + :195-200) on the matrix cores.  The row-per-thread kernel
// (sa_mlp.hip) spends ~816 fp32 FMAs and 32 LDS atomics per grouped row; here a wave takes 32 rows
// (two 16-row half tiles, as the sa2 kernel, sa_mfma_sa2.hip) through three chained MFMAs whose
// accumulators feed the next layer in place:
//   layer 1, fp32 32x32x2:       H1^T (32 ch x 32 rows) = W1 (32 x C0) . X^T, channels 16..31 zero
//        (A: lane = output channel, one input channel per lane half and k-step; B: lane = row)
//   layer 2, bf16 32x32x16 x 6:  H2^T = W2 (32 x 16) . H1^T -- the B operand (lane = row, k in
//        registers) is layer 1's accumulator registers 0..7 as they stand: k-slot 8h + r of lane
//        half h is channel acc_row(r, h); W2's A fragment is stored in that channel order
//   layer 3, bf16 32x32x16 x 6:  H3 (32 rows x 32 ch) = H2 . W3^T -- the A operand (lane = row, k
//        in registers) is again layer 2's registers 0..7, W3^T's B fragment in the same order
// Layer 3's accumulator has channels on lanes and rows in registers: rows 0-15 (the first half
// tile) are registers 0..7 of both lane halves, rows 16-31 registers 8..15, so each half tile's
// maximum is a per-lane max plus one exchange between lane halves.  BN (eval) is folded into the
// weights and biases, (W x + b) s + t = (s W) x + (s b + t); layer 3's bias and ReLU go after the
// maximum (max_i fl(a_i + b) = fl(max_i a_i + b), rounding is monotone).  Layers 2 and 3 keep fp32
// accuracy through the three-way bf16 split of sa_mfma_common.h.  A centre without hits (count < 1:
// the reference would gather index N, :104) gets zeros, as the row-per-thread kernel gives it.
#include "sa_mfma_common.h"

namespace dvcp {

struct Sa1Lds {
  float w1[3][64];   // layer-1 A fragment per k-step: lane (o, kh) -> s1_o W1[o][2 s + kh]  (o < 16)
  bf16x8 w2[3][64];  // layer-2 A fragment pieces: lane (o, kh), element r -> s2_o W2[o][acc_row(r, kh)]
  bf16x8 w3[3][64];  // layer-3 B fragment pieces: lane (o, kh), element r -> s3_o W3[o][acc_row(r, kh)]
  float b1[2][8];    // folded biases of layers 1, 2 by [lane half][accumulator register]
  float b2[2][8];
};

template <typename T, typename FT, int D>
__global__ __launch_bounds__(kMfmaWaves * kWave) void sa1_mfma_kernel(
    PointsView<T> pts, PointsView<T> ctr, int S, int B, const FT* __restrict__ feat, int64_t fb, int64_t fd, int64_t fn,
    const int32_t* __restrict__ count, const int32_t* __restrict__ list, int nsample, const float* __restrict__ params,
    float* __restrict__ out, int xcd) {
  constexpr int C0 = 3 + D, C1 = 16, C2 = 16, C3 = 32;
  constexpr int KS = (C0 + 1) / 2;  // layer-1 k-steps: input channels (2 s, 2 s + 1) on lane halves (0, 1)
  static_assert(D == 0 || D == 3, "sa1 tables");
  __shared__ Sa1Lds L;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r32 = lane & 31;
  // wave-uniform by construction; said so, the centre walk below stays in scalar registers and branches
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const float* W1 = params;
  const float* pb1 = W1 + C1 * C0;
  const float* ps1 = pb1 + C1;
  const float* pt1 = ps1 + C1;
  const float* W2 = pt1 + C1;
  const float* pb2 = W2 + C2 * C1;
  const float* ps2 = pb2 + C2;
  const float* pt2 = ps2 + C2;
  const float* W3 = pt2 + C2;
  const float* pb3 = W3 + C3 * C2;
  const float* ps3 = pb3 + C3;
  const float* pt3 = ps3 + C3;
  auto fold_bias = [](float b, float s, float t) {
    return static_cast<float>(static_cast<double>(b) * s + static_cast<double>(t));
  };
  for (int i = tid; i < KS * 64; i += blockDim.x) {
    const int l = i % 64, s = i / 64, o = l & 31, c = 2 * s + (l >> 5);
    L.w1[s][l] = (o < C1 && c < C0) ? W1[o * C0 + c] * ps1[o] : 0.0f;
  }
  if (tid < 64) {
    const int o = tid & 31, kh = tid >> 5;
    float a[8], w[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      a[r] = o < C2 ? W2[o * C1 + acc_row(r, kh)] * ps2[o] : 0.0f;
      w[r] = W3[o * C2 + acc_row(r, kh)] * ps3[o];
    }
    const Split3 sa = split3(a), sw = split3(w);
    L.w2[0][tid] = sa.p0;
    L.w2[1][tid] = sa.p1;
    L.w2[2][tid] = sa.p2;
    L.w3[0][tid] = sw.p0;
    L.w3[1][tid] = sw.p1;
    L.w3[2][tid] = sw.p2;
  } else if (tid < 80) {
    const int kh = (tid - 64) >> 3, r = tid & 7, c = acc_row(r, kh);
    L.b1[kh][r] = fold_bias(pb1[c], ps1[c], pt1[c]);
    L.b2[kh][r] = fold_bias(pb2[c], ps2[c], pt2[c]);
  }
  const float b3 = fold_bias(pb3[r32], ps3[r32], pt3[r32]);
  __syncthreads();

  // centres grid-strided over the centre index space (sa_mfma_common.h), in index order
  int64_t total, q0, qs;
  int xo = 0;
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
  for (int64_t qc = q0; qc < total; qc += 64 * qs) {
    // this lane's centre of the next 64: cloud, flat index, rows (0: no hit), coordinates
    // (through sa_centre_meta with a null order the clamp and the index arithmetic come out differently)
    const int64_t qm = qc + lane * qs;
    int m_b = 0, m_rows = 0;
    int64_t m_fc = 0;
    T m_cx = T(0), m_cy = T(0), m_cz = T(0);
    if (qm < total) {
      const int64_t q = xcd ? (xo + 8 * (qm / S)) * static_cast<int64_t>(S) + qm % S : qm;
      m_b = static_cast<int>(q / S);
      m_fc = q;
      const int r = count[q];
      m_rows = r < 0 ? 0 : (r > nsample ? nsample : r);
      const int c = static_cast<int>(q % S);
      ctr.load3(m_b, c, m_cx, m_cy, m_cz);
    }
    const int ncen = static_cast<int>(min<int64_t>(64, (total - qc + qs - 1) / qs));
    int js = 0, hs = 0;  // the next half tile: centre js, half hs
    auto nh_of = [&](int jj) { return max(1, (lane_bcast(m_rows, jj) + 15) >> 4); };
    int nhj = ncen > 0 ? nh_of(0) : 0;
    int runj = -1;
    float run = 0.0f;
    auto flush = [&]() {
      const int64_t fcr = lane_bcast(m_fc, runj);
      const bool empty = lane_bcast(m_rows, runj) == 0;
      if (h == 0) out[fcr * C3 + r32] = empty ? 0.0f : fmaxf(run + b3, 0.0f);
    };
    auto fold = [&](int jj, float m) {
      if (jj != runj) {
        if (runj >= 0) flush();
        runj = jj;
        run = m;
      } else {
        run = fmaxf(run, m);
      }
    };
    // The same three-stage pipeline over the batch's flat tile sequence as sa2_mfma_kernel's
    // (sa_mfma_sa2.hip): list entry of tile t + 2, point (and normal) of tile t + 1, MFMAs of tile t.
    const bool sB = r32 >= 16;  // this lane's row r32 of the tile: first or second half tile
    struct Gathered {
      T px, py, pz;
      FT f0, f1;  // D == 3: feature channel 0, and channel 1 (lane half 0) or 2 (half 1)
    };
    auto entry = [&](const HalfPair& t) { return half_pair_entry(t, m_fc, m_rows, r32, count, list, nsample); };
    auto gather = [&](const HalfPair& t, int ne, Gathered& g) {
      const int jl = sB ? t.jB : t.jA;
      const int b = lane_gather(m_b, jl);
      const int n = lane_gather(m_rows, jl) == 0 ? 0 : ne;
      pts.load3(b, n, g.px, g.py, g.pz);
      if constexpr (D != 0) {
        const FT* f = feat + b * fb + static_cast<int64_t>(n) * fn;
        g.f0 = f[0];
        g.f1 = h == 0 ? f[fd] : f[2 * fd];
      }
    };
    auto compute = [&](const HalfPair& t, const Gathered& g) {
      // opaque zero on the LDS indices: fragments re-read per tile, not hoisted into registers
      int zo = 0;
      asm volatile("" : "+v"(zo));
      const int jl = sB ? t.jB : t.jA;
      const T cx = lane_gather(m_cx, jl), cy = lane_gather(m_cy, jl), cz = lane_gather(m_cz, jl);
      const float dx = static_cast<float>(g.px - cx);
      const float dy = static_cast<float>(g.py - cy);
      const float dz = static_cast<float>(g.pz - cz);
      float x[KS];
      x[0] = h == 0 ? dx : dy;
      if constexpr (D == 0) {
        x[1] = h == 0 ? dz : 0.0f;
      } else {
        x[1] = h == 0 ? dz : static_cast<float>(g.f0);
        x[2] = static_cast<float>(g.f1);
      }
      f32x16 a1;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        a1[r] = L.b1[h][r + zo];
        a1[8 + r] = 0.0f;
      }
#pragma unroll
      for (int s = 0; s < KS; ++s) a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(L.w1[s][lane + zo], x[s], a1, 0, 0, 0);
      float v[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = sa_relu(a1[r]);
      const Split3 p1 = split3(v);
      f32x16 a2;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        a2[r] = L.b2[h][r + zo];
        a2[8 + r] = 0.0f;
      }
      const Split3 w2{L.w2[0][lane + zo], L.w2[1][lane + zo], L.w2[2][lane + zo]};
      a2 = mfma_split3(w2, p1.p0, p1.p1, p1.p2, a2);
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = sa_relu(a2[r]);
      const Split3 p2 = split3(v);
      f32x16 a3;
#pragma unroll
      for (int r = 0; r < 16; ++r) a3[r] = 0.0f;
      a3 = mfma_split3(p2, L.w3[0][lane + zo], L.w3[1][lane + zo], L.w3[2][lane + zo], a3);
      float mA = a3[0], mB = a3[8];
#pragma unroll
      for (int r = 1; r < 8; ++r) {
        mA = fmaxf(mA, a3[r]);
        mB = fmaxf(mB, a3[8 + r]);
      }
      mA = fmaxf(mA, __shfl_xor(mA, 32, kWave));
      mB = fmaxf(mB, __shfl_xor(mB, 32, kWave));
      fold(t.jA, mA);
      if (t.hasB) fold(t.jB, mB);
    };
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

template <typename T, typename FT, int D>
int launch_sa1_mfma(const void* xyz, int64_t sb, int64_t sc, int64_t sn, const void* c, int64_t cb, int64_t cc,
                    int64_t cn, int S, int B, const void* feat, int64_t fb, int64_t fd, int64_t fn, const int32_t* count,
                    const int32_t* list, int nsample, const float* params, float* out, hipStream_t st) {
  PointsView<T> pv{static_cast<const T*>(xyz), sb, sc, sn};
  PointsView<T> cv{static_cast<const T*>(c), cb, cc, cn};
  const SaGrid g(B, S);
  hipLaunchKernelGGL((sa1_mfma_kernel<T, FT, D>), dim3(g.grid), dim3(kMfmaWaves * kWave), 0, st, pv, cv, S, B,
                     static_cast<const FT*>(feat), fb, fd, fn, count, list, nsample, params, out, g.xcd);
  return launch_status("dvcp_sa_group_mlp(mfma3)");
}

#define DVCP_SA1_INST(T, FT, D)                                                                              \
  template int launch_sa1_mfma<T, FT, D>(const void*, int64_t, int64_t, int64_t, const void*, int64_t, int64_t,  \
                                         int64_t, int, int, const void*, int64_t, int64_t, int64_t, const int32_t*, \
                                         const int32_t*, int, const float*, float*, hipStream_t);
DVCP_SA1_INST(float, float, 0)
DVCP_SA1_INST(float, double, 0)
DVCP_SA1_INST(double, float, 0)
DVCP_SA1_INST(double, double, 0)
DVCP_SA1_INST(float, float, 3)
DVCP_SA1_INST(float, double, 3)
DVCP_SA1_INST(double, float, 3)
DVCP_SA1_INST(double, double, 3)
#undef DVCP_SA1_INST

}  // namespace dvcp
