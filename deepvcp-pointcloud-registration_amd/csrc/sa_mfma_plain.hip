// sa_mfma_plain.hip -- the two-layer set-abstraction tables (sa2: 35-32-64, sa3: 67-64-64) without a
// workspace, dvcp_sa_group_mlp: layer 1 whole per grouped row, BN after each GEMM, centres in index
// order unless an order is given, no software pipeline (sa_mfma_common.h has the layers' layout).
// The forward runs the workspace kernels (sa_mfma_sa2.hip, sa_mfma_sa3.hip); this one is their
// unpipelined form, same arithmetic per tile and the same order.
// Input channel order per k-step s of layer 1: lane half 0 takes [x, y, z, f0 .. f(D/2-1)], half 1 takes
// [0, 0, 0, f(D/2) .. f(D-1)], so each half loads one contiguous, 16-B aligned feature run.
#include "sa_mfma_common.h"

namespace dvcp {

// LDS image of the weights in fragment order (staged once per workgroup).
template <int D, int C1, int C2>
struct SaPlainLds {
  using S = SaMfmaShape<D, C1, C2>;
  float w1[S::MT][S::KS][64];       // A fragment of layer 1: [tile][k-step][lane]
  float wx[S::MT][2][64];           // never written or read (without it the LDS size and offsets change)
  bf16x8 w2s[S::CT][S::KB][3][64];  // B fragment of layer 2 as three bf16 pieces: [tile][k-step][piece][lane]
  float b1[S::MT][2][16];           // layer-1 bias / BN scale / BN shift by [tile][lane half][register]
  float s1[S::MT][2][16];
  float t1[S::MT][2][16];
};

// channel (index into [xyz, features]) feeding k-step s of lane half h, or -1 (zero)
template <int D>
__device__ __forceinline__ int sa_in_channel(int s, int h) {
  if (s < 3) return h == 0 ? s : -1;
  return 3 + h * (D / 2) + (s - 3);
}

// U, ub: unused (the workspace kernels' parameter list)
template <typename T, int D, int C1, int C2>
__global__ __launch_bounds__(kMfmaWaves * kWave) __attribute__((amdgpu_waves_per_eu(3))) void sa_plain_mfma_kernel(
    PointsView<T> pts, PointsView<T> ctr, int S, int B, const float* __restrict__ feat, int64_t fb, int64_t fn,
    const int32_t* __restrict__ count, const int32_t* __restrict__ list, int nsample,
    const float* __restrict__ params, const float* __restrict__ U, int64_t ub, const int32_t* __restrict__ order,
    float* __restrict__ out, int xcd) {
  using Sh = SaMfmaShape<D, C1, C2>;
  constexpr int C0 = Sh::C0, KS = Sh::KS, MT = Sh::MT, CT = Sh::CT;
  __shared__ SaPlainLds<D, C1, C2> L;
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
  for (int i = tid; i < MT * KS * 64; i += blockDim.x) {
    const int l = i % 64, s = (i / 64) % KS, mt = i / (64 * KS);
    const int ch = sa_in_channel<D>(s, l >> 5);
    L.w1[mt][s][l] = ch < 0 ? 0.0f : W1[(32 * mt + (l & 31)) * C0 + ch];
  }
  // k-step s, lane half hh, element j <-> layer-1 channel 32 (s / 2) + acc_row(8 (s % 2) + j, hh): the
  // layer-1 accumulator registers 8 (s % 2) .. + 7 of tile s / 2 are the A fragment as they stand
  for (int i = tid; i < CT * Sh::KB * 64; i += blockDim.x) {
    const int l = i % 64, s = (i / 64) % Sh::KB, ct = i / (64 * Sh::KB);
    const int o = 32 * ct + (l & 31);
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      w[j] = W2[o * C1 + 32 * (s / 2) + acc_row(8 * (s % 2) + j, l >> 5)];
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
  }
  __syncthreads();

  // ---- one centre per wave, grid-strided over the centre index space (sa_mfma_common.h) ------
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
  // The wave's centres are ql = q0, q0 + qs, ...: their metadata (order, count, centre) is
  // loaded 64 centres at a time, one per lane, and read back by readlane, so a centre's first
  // tile waits for neither.
  for (int64_t qc = q0; qc < total; qc += 64 * qs) {
    const int64_t qm = qc + lane * qs;
    int m_b = 0, m_rows = 0;  // rows 0: no hit (the centre's output is 0)
    int64_t m_fc = 0;
    T m_cx = T(0), m_cy = T(0), m_cz = T(0);
    sa_centre_meta(qm, total, xcd, xo, S, order, count, nsample, ctr, m_b, m_rows, m_fc, m_cx, m_cy, m_cz);
    const int ncen = static_cast<int>(min<int64_t>(64, (total - qc + qs - 1) / qs));
    // list entry of this lane's point in the next tile to run (centre j, tile n0)
    auto list_entry = [&](int j, int n0) {
      const int64_t fcj = lane_bcast(m_fc, j);
      const int rj = lane_bcast(m_rows, j);
      const int row = n0 + r32;
      return rj == 0 ? 0 : list[fcj * nsample + (row < rj ? row : 0)];
    };
    // The first list row of the next centre is fetched one tile ahead; a centre without hits
    // runs no tile, so "next" is the next centre with hits (lane mask of the batch).
    const uint64_t live_c = __ballot(lane < ncen && m_rows > 0);
    auto next_live = [&](int j) {  // the first centre after j with hits, or 64
      const uint64_t m = j >= 63 ? 0ull : (live_c & (~0ull << (j + 1)));
      return m ? static_cast<int>(__builtin_ctzll(m)) : 64;
    };
    int n_next = 0;
    {
      const int j0 = (live_c & 1ull) ? 0 : next_live(0);
      if (j0 < ncen) n_next = list_entry(j0, 0);
    }
    for (int j = 0; j < ncen; ++j) {
      const int b = lane_bcast(m_b, j);
      const int64_t fc = lane_bcast(m_fc, j);
      const int rows = lane_bcast(m_rows, j);
      const T cx = lane_bcast(m_cx, j), cy = lane_bcast(m_cy, j), cz = lane_bcast(m_cz, j);
      float mx[CT];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) mx[ct] = 0.0f;  // post-ReLU values are >= +0

      for (int n0 = 0; n0 < rows; n0 += 32) {
        // An opaque zero added to every LDS weight index: the fragments are re-read per tile
        // (one ds_read per MFMA) instead of being hoisted out of the loop into ~100 registers,
        // which would cap occupancy at 2 waves per SIMD.
        int zo = 0;
        asm volatile("" : "+v"(zo));
        // B fragment of layer 1: this lane's point (r32) and its half of the input channels
        const int n = n_next;
        if (n0 + 32 < rows)
          n_next = list_entry(j, n0 + 32);
        else if (next_live(j) < ncen)
          n_next = list_entry(next_live(j), 0);
        f32x16 acc1[MT];
        float x[KS];
        if (h == 0) {
          x[0] = static_cast<float>(pts.at(b, 0, n) - cx);
          x[1] = static_cast<float>(pts.at(b, 1, n) - cy);
          x[2] = static_cast<float>(pts.at(b, 2, n) - cz);
        } else {
          x[0] = x[1] = x[2] = 0.0f;
        }
        const float4* fr = reinterpret_cast<const float4*>(feat + b * fb + static_cast<int64_t>(n) * fn + h * (D / 2));
#pragma unroll
        for (int v = 0; v < D / 8; ++v) {
          const float4 f = fr[v];
          x[3 + 4 * v] = f.x;
          x[4 + 4 * v] = f.y;
          x[5 + 4 * v] = f.z;
          x[6 + 4 * v] = f.w;
        }
        // layer 1 (transposed): acc1[mt] rows = output channels, columns = points
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc1[mt][r] = L.b1[mt][h][r + zo];
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc1[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(L.w1[mt][s][lane + zo], x[s], acc1[mt], 0, 0, 0);
        // BN (eval) + ReLU in place
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float v = acc1[mt][r] * L.s1[mt][h][r + zo] + L.t1[mt][h][r + zo];
            acc1[mt][r] = v > 0.0f ? v : 0.0f;
          }
        // layer 2: A operand = the layer-1 registers, B = W2^T fragments
        f32x16 acc2[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc2[ct][r] = b2[ct];
#pragma unroll
        for (int s = 0; s < Sh::KB; ++s) {
          float x[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) x[j] = acc1[s / 2][8 * (s % 2) + j];
          const Split3 a = split3(x);
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
            acc2[ct] = mfma_split3(a, L.w2s[ct][s][0][lane + zo], L.w2s[ct][s][1][lane + zo], L.w2s[ct][s][2][lane + zo],
                                   acc2[ct]);
        }
        // BN + ReLU, then max over this tile's points (registers)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float v = acc2[ct][r] * s2[ct] + t2[ct];
            mx[ct] = fmaxf(mx[ct], v > 0.0f ? v : 0.0f);
          }
      }
      // the two lane halves hold different points of the same channel
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        float m = fmaxf(mx[ct], __shfl_xor(mx[ct], 32, kWave));
        if (h == 0) out[fc * C2 + 32 * ct + r32] = m;
      }
    }
  }
}

template <typename T, int D, int C1, int C2>
void launch_sa_plain_mfma(const SaTableArgs<T>& a, hipStream_t st) {
  const SaGrid g(a.B, a.S);
  hipLaunchKernelGGL((sa_plain_mfma_kernel<T, D, C1, C2>), dim3(g.grid), dim3(kMfmaWaves * kWave), 0, st, a.pts, a.ctr,
                     a.S, a.B, a.feat, a.fb, a.fn, a.count, a.list, a.nsample, a.params, nullptr, 0, a.order, a.out,
                     g.xcd);
}
template void launch_sa_plain_mfma<float, 32, 32, 64>(const SaTableArgs<float>&, hipStream_t);
template void launch_sa_plain_mfma<double, 32, 32, 64>(const SaTableArgs<double>&, hipStream_t);
template void launch_sa_plain_mfma<float, 64, 64, 64>(const SaTableArgs<float>&, hipStream_t);
template void launch_sa_plain_mfma<double, 64, 64, 64>(const SaTableArgs<double>&, hipStream_t);

}  // namespace dvcp
