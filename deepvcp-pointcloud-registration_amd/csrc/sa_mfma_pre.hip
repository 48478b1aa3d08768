// sa_mfma_pre.hip -- what runs ahead of the two-layer set-abstraction tables when they have a
// workspace (sa_mfma_common.h): the per-point half of layer 1 and the centres' visiting order.
#include "morton.h"
#include "sa_mfma_common.h"

namespace dvcp {

// The per-point half of the decomposed layer 1 (sa_layer1_xyz in sa_mfma_common.h has the other):
// U[n] = W1f f_n + b1 with BN1 folded, once per input point.
// The per-point pass is a plain GEMM on the fp32 matrix cores (U = F . W1f'^T + b1'): one wave
// per 32 input points, v_mfma_f32_32x32x2_f32 with k-step s taking input channels s (lane half 0)
// and s + D/2 (half 1), so each lane reads one contiguous half of its point's feature row; the
// BN-folded weights are staged once per workgroup as B fragments; bound by its 82 MB (sa3, C3).
// The accumulation is a k-ordered fp32 chain (the MFMA adds its two k-products per step).
// (Round 4 had a row-per-thread VALU form of this pass, float4 FMA chains that hipcc packed into
// v_pk_fma_f32.  With a second process on the GPU, single fp32 lanes of its accumulators came out
// different -- the round-4 two-rank test failure -- so it was removed.  The cause is not proven:
// DESIGN.md section 5 names the one distinctive sequence, a v_mov-written register broadcast into
// a packed FMA one instruction later, which no shipped kernel contains.)
template <int D, int C1>
__global__ __launch_bounds__(256) void sa_pre_mfma_kernel(const float* __restrict__ feat, int64_t fb, int64_t fn, int N,
                                                          int B, const float* __restrict__ params,
                                                          float* __restrict__ U, const int64_t* __restrict__ rows,
                                                          int Nf) {
  constexpr int C0 = 3 + D, MT = C1 / 32, KS = D / 2;
  static_assert(D % 8 == 0 && C1 % 32 == 0, "MFMA tiling");
  __shared__ float wf[MT][KS][64];  // B fragment: lane (o, h) of k-step s -> s1_o W1[o][3 + s + h D/2]
  __shared__ float bias[C1];         // folded bias (the accumulators' channel is the lane)
  const float* W1 = params;
  const float* pb1 = W1 + C1 * C0;
  const float* ps1 = pb1 + C1;
  const float* pt1 = ps1 + C1;
  for (int i = threadIdx.x; i < MT * KS * 64; i += blockDim.x) {
    const int l = i % 64, s = (i / 64) % KS, mt = i / (64 * KS), o = 32 * mt + (l & 31);
    wf[mt][s][l] = W1[o * C0 + 3 + s + (l >> 5) * (D / 2)] * ps1[o];
  }
  for (int c = threadIdx.x; c < C1; c += blockDim.x)
    bias[c] = static_cast<float>(static_cast<double>(pb1[c]) * ps1[c] + static_cast<double>(pt1[c]));
  __syncthreads();
  const int lane = threadIdx.x & 63, h = lane >> 5, r32 = lane & 31;
  const int64_t total = static_cast<int64_t>(B) * N;
  const int64_t ntiles = (total + 31) / 32;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); t < ntiles;
       t += static_cast<int64_t>(gridDim.x) * 4) {
    // this lane's point (row r32 of the tile) and its half of the feature row
    const int64_t i = t * 32 + r32;
    const int64_t ic = i < total ? i : total - 1;
    const int b = static_cast<int>(ic / N), n = static_cast<int>(ic % N);
    int64_t src = n;
    if (rows) {
      const int64_t r = rows[ic];
      src = r < 0 ? 0 : (r >= Nf ? Nf - 1 : r);
    }
    const float4* fr = reinterpret_cast<const float4*>(feat + b * fb + src * fn + h * (D / 2));
    float x[KS];
#pragma unroll
    for (int v = 0; v < KS / 4; ++v) {
      const float4 q = fr[v];
      x[4 * v] = q.x;
      x[4 * v + 1] = q.y;
      x[4 * v + 2] = q.z;
      x[4 * v + 3] = q.w;
    }
    int zo = 0;  // opaque zero: the fragments are read per tile, not hoisted into registers
    asm volatile("" : "+v"(zo));
    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const float bc = bias[32 * mt + r32 + zo];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][r] = bc;
    }
    // H (32 points x C1): A = the feature rows (lane = point), B = the weight fragments (lane = channel)
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[s], wf[mt][s][lane + zo], acc[mt], 0, 0, 0);
    // D[point][channel]: lane = channel, register r = point acc_row(r, h)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t ip = t * 32 + acc_row(r, h);
      if (ip < total)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) U[ip * C1 + 32 * mt + r32] = acc[mt][r];
    }
  }
}

// Centres of each cloud in 12-bit Hilbert-cell order (one workgroup per cloud), for the MFMA
// kernel's visiting order.  The order changes only which wave computes which centre.
template <typename T>
__global__ __launch_bounds__(kBuildThreads) void sa_order_kernel(PointsView<T> ctr, int S, int32_t* __restrict__ order) {
  __shared__ uint32_t bins[kSortBins];
  __shared__ uint32_t wsum[16];
  __shared__ float red[2][3][16];
  const int b = blockIdx.x;
  auto get = [&](int i, float (&v)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = static_cast<float>(ctr.at(b, a, i));
  };
  float lo[3], hi[3];
  block_bbox(S, get, lo, hi, red);
  int32_t* o = order + static_cast<int64_t>(b) * S;
  morton_sort(S, get, [&](int pos, int i, const float (&)[3]) { o[pos] = i; }, lo, hi, bins, wsum);
}

template <typename T>
void launch_sa_order(PointsView<T> ctr, int S, int B, int32_t* order, hipStream_t st) {
  hipLaunchKernelGGL((sa_order_kernel<T>), dim3(B), dim3(kBuildThreads), 0, st, ctr, S, order);
}
template void launch_sa_order<float>(PointsView<float>, int, int, int32_t*, hipStream_t);
template void launch_sa_order<double>(PointsView<double>, int, int, int32_t*, hipStream_t);

template <int D, int C1>
void launch_sa_pre(const float* feat, int64_t fb, int64_t fn, int N, int B, const float* params, float* U,
                   const int64_t* rows, int Nf, hipStream_t st) {
  const int64_t wgs = (static_cast<int64_t>(B) * N + 127) / 128;  // four 32-point tiles per workgroup
  hipLaunchKernelGGL((sa_pre_mfma_kernel<D, C1>), dim3(static_cast<unsigned>(wgs < 2048 ? wgs : 2048)), dim3(256), 0,
                     st, feat, fb, fn, N, B, params, U, rows, Nf);
}
template void launch_sa_pre<32, 32>(const float*, int64_t, int64_t, int, int, const float*, float*, const int64_t*, int,
                                    hipStream_t);
template void launch_sa_pre<64, 64>(const float*, int64_t, int64_t, int, int, const float*, float*, const int64_t*, int,
                                    hipStream_t);

}  // namespace dvcp
