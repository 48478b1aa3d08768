// paper_wl_train.hip -- training of the paper's weighting layer (Sec. 3.2; paper-faithful mode, NOT
// reference parity, like paper.hip): its backward with BatchNorm in eval mode, and the statistics,
// forward and backward passes under batch-statistics BatchNorm (training mode).
//
// The eval path folds BN into the linear layers, (W s) x + (b s + h), on the pack
//   W1 (16 x 32) | b1 | W2 (8 x 16) | b2 | W3 (8) | b3                 (WlPack<0>, the forward is
// weighting_kernel, csrc/head_topk.hip).  That cannot express xhat when gamma = 0 and rounds
// differently from (W x + b) s + h, so the batch-statistics entry points share one arithmetic of
// their own: y = (acc + b) * scale + shift per BN layer (linear_sgpr's chain, then a multiply and an
// add, no fma), a = y > 0 ? y : 0, on the pack
//   W1 (16 x 32) | b1 | scale1 | shift1 | W2 (8 x 16) | b2 | scale2 | shift2 | W3 (8) | b3   (WlPack<1>).
//
//   wbn_stats_kernel<L>   per-channel sum z and sum z^2 of layer L's linear output over the P rows
//                         (layer 1 below it evaluated with the scale | shift already in the pack):
//                         a row per lane, fp64 accumulators per lane fed with the single entries, a
//                         wave sum, one partial row per workgroup.
//   wbn_forward_kernel    the scores.
//   wbn_bwd_kernel<MODE>  the backward.  Every pass recomputes the forward exactly, a row per lane,
//                         with the forward's own fma chain (linear_sgpr) and `> 0` test, so the ReLU
//                         masks are the forward's; softplus' derivative is the logistic of the
//                         pre-activation (1 on the forward's v > 20 branch).
//                         MODE 0 and kWbnEval: d feat and the gradients of W1 b1 W2 b2 W3 b3.  The
//                         rows of a 64-row tile are staged in LDS and every lane adds its 8 + 2 + 1
//                         weights' terms row by row; one partial row per workgroup, folded in index
//                         order in fp64 (fold_rows, fold.hip).
//                         kWbnEval: the folded pack, dz = g_a.  MODE >= 0: torch's batch-norm
//                         backward, dz = scale (g_a - A/M - xhat B/M), xhat and the mean terms
//                         evaluated in fp64 from fp64 statistics.  MODE 2 / 1: A = sum g_a and
//                         B = sum g_a xhat of that layer (fp64, as the statistics), given the layers above.
//
// No atomics anywhere: two identical calls give identical bits.
#include "common.h"

namespace dvcp {

// Parameter offsets.  BN = 0: the folded pack (and the gradient row) W1 | b1 | W2 | b2 | W3 | b3;
// BN = 1: the train-mode pack, scale | shift (S1, S2) after each BN layer.
template <int BN>
struct WlPack {
  static constexpr int W1 = 0, S1 = 16 * 32 + 16, W2 = S1 + BN * 32, S2 = W2 + 8 * 16 + 8, W3 = S2 + BN * 16;
  static constexpr int N = W3 + 8 + 1;
};
constexpr int kWbnW1 = WlPack<1>::W1, kWbnS1 = WlPack<1>::S1, kWbnW2 = WlPack<1>::W2, kWbnS2 = WlPack<1>::S2;
constexpr int kWbnW3 = WlPack<1>::W3;
constexpr int kWbnPack = WlPack<1>::N;   // 721: the train-mode pack
constexpr int kWbnGrads = WlPack<0>::N;  // 673: PaperWeighting.packed_params()
static_assert(kWbnPack == 721 && kWbnGrads == 673, "the two packs");
constexpr int kWbnStat2 = 4 * 16;  // bnstat: mean | rstd | A/M | B/M of bn1 (4 x 16), then of bn2 (4 x 8)
constexpr int kWbnRows = 64;       // rows per tile: one per lane
constexpr int kWbnRow = 81;        // x 32 | dz1 16 | a1 16 | dz2 8 | a2 8 | d v 1 (odd: no bank conflicts)
constexpr int kWbnMaxGrid = 256;
constexpr int kWbnSumRow = 32;     // doubles per partial row of sums: 2 x 16 at the most

static int wbn_grid(int P) {
  const int tiles = (P + kWbnRows - 1) / kWbnRows;
  return tiles < kWbnMaxGrid ? tiles : kWbnMaxGrid;
}

__device__ __forceinline__ void wbn_load_row(const float* __restrict__ x, int64_t i, float (&f)[32]) {
  const float4* sp = reinterpret_cast<const float4*>(x + i * 32);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float4 v = sp[q];
    f[4 * q] = v.x;
    f[4 * q + 1] = v.y;
    f[4 * q + 2] = v.z;
    f[4 * q + 3] = v.w;
  }
}

// y = z * scale + shift (two roundings), a = y > 0 ? y : 0: the one BN arithmetic of this file
// (BN = false, the folded pack: y = z)
template <int C, bool BN = true>
__device__ __forceinline__ void wbn_norm_relu(const float (&z)[C], const float* __restrict__ ss, float (&y)[C],
                                              float (&a)[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    y[c] = BN ? z[c] * ss[c] + ss[C + c] : z[c];
    a[c] = y[c] > 0.0f ? y[c] : 0.0f;
  }
}


// ------------------------------------------------------------------------------------ statistics
template <int LAYER>
__global__ __launch_bounds__(kWbnRows) void wbn_stats_kernel(const float* __restrict__ x, int P,
                                                             const float* __restrict__ params,
                                                             double* __restrict__ partial) {
  constexpr int C = LAYER == 1 ? 16 : 8;
  const int lane = threadIdx.x;
  double s[C], q[C];
#pragma unroll
  for (int c = 0; c < C; ++c) s[c] = q[c] = 0.0;
  const int tiles = (P + kWbnRows - 1) / kWbnRows;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t i = static_cast<int64_t>(t) * kWbnRows + lane;
    if (i >= P) continue;
    float f[32], z1[16];
    wbn_load_row(x, i, f);
    linear_sgpr<32, 16>(f, z1, params + kWbnW1);
    if constexpr (LAYER == 1) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double zd = static_cast<double>(z1[c]);
        s[c] += zd;
        q[c] += zd * zd;
      }
    } else {
      float y1[16], a1[16], z2[8];
      wbn_norm_relu<16>(z1, params + kWbnS1, y1, a1);
      linear_sgpr<16, 8>(a1, z2, params + kWbnW2);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double zd = static_cast<double>(z2[c]);
        s[c] += zd;
        q[c] += zd * zd;
      }
    }
  }
  double* o = partial + static_cast<int64_t>(blockIdx.x) * kWbnSumRow;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double sw = wave_sum(s[c]), qw = wave_sum(q[c]);
    if (lane == 0) {
      o[c] = sw;
      o[C + c] = qw;
    }
  }
}

// --------------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(256) void wbn_forward_kernel(const float* __restrict__ x, int P,
                                                          const float* __restrict__ params,
                                                          float* __restrict__ score) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= P) return;
  float f[32], z1[16], y1[16], a1[16], z2[8], y2[8], a2[8], p3[1];
  wbn_load_row(x, i, f);
  linear_sgpr<32, 16>(f, z1, params + kWbnW1);
  wbn_norm_relu<16>(z1, params + kWbnS1, y1, a1);
  linear_sgpr<16, 8>(a1, z2, params + kWbnW2);
  wbn_norm_relu<8>(z2, params + kWbnS2, y2, a2);
  linear_sgpr<8, 1>(a2, p3, params + kWbnW3);
  const float v = p3[0];
  score[i] = v > 20.0f ? v : log1pf(expf(v));  // torch.nn.Softplus(beta=1, threshold=20)
}

// -------------------------------------------------------------------------------------- backward
constexpr int kWbnEval = -1;  // wbn_bwd_kernel's eval mode: the folded pack, no statistics

template <int MODE>
__global__ __launch_bounds__(kWbnRows) void wbn_bwd_kernel(const float* __restrict__ x, int P,
                                                           const float* __restrict__ params,
                                                           const double* __restrict__ bnstat,
                                                           const float* __restrict__ g, float* __restrict__ gx,
                                                           float* __restrict__ partial,
                                                           double* __restrict__ sum_partial) {
  constexpr bool kBn = MODE != kWbnEval;  // batch statistics
  constexpr bool kGrad = MODE <= 0;       // the gradient pass
  using L = WlPack<kBn ? 1 : 0>;
  __shared__ float st[kGrad ? kWbnRows : 1][kWbnRow];
  const int lane = threadIdx.x;
  const float* w1 = params + L::W1;
  const float* w2 = params + L::W2;
  const float* w3 = params + L::W3;
  const float* sc1 = params + L::S1;       // kBn only
  const float* sc2 = params + L::S2;
  const double* bs1 = bnstat;              // mean | rstd | A/M | B/M, 16 each
  const double* bs2 = bnstat + kWbnStat2;  // the same, 8 each
  // the gradient pass: this lane's weights, fc1.W[c1][8 q1 .. + 8], fc2.W[o2][2 q2 .. + 2], fc3.W[0][q2] (lanes < 8)
  const int c1 = lane >> 2, q1 = lane & 3, o2 = lane >> 3, q2 = lane & 7;
  float dW1[8], dW2[2] = {0.f, 0.f}, dW3 = 0.f, db1 = 0.f, db2 = 0.f, db3 = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) dW1[k] = 0.f;
  constexpr int CS = MODE == 1 ? 16 : 8;  // MODE 2 / 1: the layer's channels
  double sa[CS], sb[CS];
#pragma unroll
  for (int c = 0; c < CS; ++c) sa[c] = sb[c] = 0.0;
  const int tiles = (P + kWbnRows - 1) / kWbnRows;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t i = static_cast<int64_t>(t) * kWbnRows + lane;
    const int nrows = P - t * kWbnRows < kWbnRows ? P - t * kWbnRows : kWbnRows;
    if constexpr (kGrad) __syncthreads();  // the previous tile's readers are done
    if (i < P) {
      // the forward, as wbn_forward_kernel (kWbnEval: weighting_kernel) writes it
      float f[32], z1[16], y1[16], a1[16], z2[8], y2[8], a2[8], p3[1];
      wbn_load_row(x, i, f);
      linear_sgpr<32, 16>(f, z1, w1);
      wbn_norm_relu<16, kBn>(z1, sc1, y1, a1);
      linear_sgpr<16, 8>(a1, z2, w2);
      wbn_norm_relu<8, kBn>(z2, sc2, y2, a2);
      linear_sgpr<8, 1>(a2, p3, w3);
      const float v = p3[0];
      // softplus'(v) = 1 / (1 + exp(-v)); the forward's v > 20 branch is the identity
      const float gvv = g[i] * (v > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-v)));
      // xhat and the mean terms in fp64: with few rows g_a - A/M and xhat B/M cancel (M = 2: to
      // eps / var of their size), which fp32 statistics would not survive
      float g2[8];
      double xh2[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        g2[c] = y2[c] > 0.0f ? w3[c] * gvv : 0.0f;
        if constexpr (kBn) xh2[c] = (static_cast<double>(z2[c]) - bs2[c]) * bs2[8 + c];
      }
      if constexpr (MODE == 2) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          sa[c] += static_cast<double>(g2[c]);
          sb[c] += static_cast<double>(g2[c]) * xh2[c];
        }
      } else {
        float dz2[8], g1[16];
        double xh1[16];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          if constexpr (kBn)
            dz2[c] = static_cast<float>(static_cast<double>(sc2[c]) *
                                        ((static_cast<double>(g2[c]) - bs2[16 + c]) - xh2[c] * bs2[24 + c]));
          else
            dz2[c] = g2[c];
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          float acc = 0.f;
#pragma unroll
          for (int o = 0; o < 8; ++o) acc = __fmaf_rn(w2[o * 16 + c], dz2[o], acc);
          g1[c] = y1[c] > 0.0f ? acc : 0.0f;
          if constexpr (kBn) xh1[c] = (static_cast<double>(z1[c]) - bs1[c]) * bs1[16 + c];
        }
        if constexpr (MODE == 1) {
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            sa[c] += static_cast<double>(g1[c]);
            sb[c] += static_cast<double>(g1[c]) * xh1[c];
          }
        } else {
          float dz1[16];
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            if constexpr (kBn)
              dz1[c] = static_cast<float>(static_cast<double>(sc1[c]) *
                                          ((static_cast<double>(g1[c]) - bs1[32 + c]) - xh1[c] * bs1[48 + c]));
            else
              dz1[c] = g1[c];
          }
          if (gx) {
            float4* dp = reinterpret_cast<float4*>(gx + i * 32);
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              float r[4];
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < 16; ++c) acc = __fmaf_rn(w1[c * 32 + 4 * q + j], dz1[c], acc);
                r[j] = acc;
              }
              dp[q] = make_float4(r[0], r[1], r[2], r[3]);
            }
          }
          float* s = st[lane];
#pragma unroll
          for (int k = 0; k < 32; ++k) s[k] = f[k];
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            s[32 + k] = dz1[k];
            s[48 + k] = a1[k];
          }
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            s[64 + k] = dz2[k];
            s[72 + k] = a2[k];
          }
          s[80] = gvv;
        }
      }
    }
    if constexpr (kGrad) {
      __syncthreads();
      // the tile's rows in order: dW = sum_rows (d out) (in)^T, db = sum_rows d out
      for (int r = 0; r < nrows; ++r) {
        const float* s = st[r];
        const float a = s[32 + c1];
        db1 += a;
#pragma unroll
        for (int k = 0; k < 8; ++k) dW1[k] = __fmaf_rn(a, s[8 * q1 + k], dW1[k]);
        const float b = s[64 + o2];
        db2 += b;
#pragma unroll
        for (int k = 0; k < 2; ++k) dW2[k] = __fmaf_rn(b, s[48 + 2 * q2 + k], dW2[k]);
        const float c = s[80];
        db3 += c;
        dW3 = __fmaf_rn(c, s[72 + q2], dW3);
      }
    }
  }
  if constexpr (kGrad) {
    float* o = partial + static_cast<int64_t>(blockIdx.x) * kWbnGrads;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[c1 * 32 + 8 * q1 + k] = dW1[k];
    if (q1 == 0) o[16 * 32 + c1] = db1;
    float* p2o = o + 16 * 32 + 16;
#pragma unroll
    for (int k = 0; k < 2; ++k) p2o[o2 * 16 + 2 * q2 + k] = dW2[k];
    if (q2 == 0) p2o[8 * 16 + o2] = db2;
    float* p3o = p2o + 8 * 16 + 8;
    if (lane < 8) p3o[lane] = dW3;
    if (lane == 0) p3o[8] = db3;
  } else {
    double* o = sum_partial + static_cast<int64_t>(blockIdx.x) * kWbnSumRow;
#pragma unroll
    for (int c = 0; c < CS; ++c) {
      const double aw = wave_sum(sa[c]), bw = wave_sum(sb[c]);
      if (lane == 0) {
        o[c] = aw;
        o[CS + c] = bw;
      }
    }
  }
}

}  // namespace dvcp

extern "C" int64_t dvcp_weighting_backward_workspace_bytes(int P) {  // one gradient row per workgroup
  if (P <= 0) return 0;
  return static_cast<int64_t>(dvcp::wbn_grid(P)) * dvcp::kWbnGrads * 4;
}

extern "C" int dvcp_weighting_backward(const float* feat, int P, const float* params, const float* grad_score,
                                       float* grad_feat, void* workspace, int64_t ws_bytes, float* grad_params,
                                       void* stream) {
  DVCP_REQUIRE(P >= 0, "dvcp_weighting_backward: P=%d is negative", P);
  DVCP_REQUIRE(params && grad_params, "dvcp_weighting_backward: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (P == 0) {
    if (hipMemsetAsync(grad_params, 0, dvcp::kWbnGrads * 4, st) != hipSuccess)
      return dvcp::launch_status("dvcp_weighting_backward(empty)");
    return DVCP_OK;
  }
  DVCP_REQUIRE(feat && grad_score && workspace, "dvcp_weighting_backward: null pointer");
  const int64_t need = dvcp_weighting_backward_workspace_bytes(P);
  DVCP_REQUIRE(ws_bytes >= need, "dvcp_weighting_backward: workspace of %lld bytes is short of %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(need));
  const int grid = dvcp::wbn_grid(P);
  float* ws = static_cast<float*>(workspace);
  hipLaunchKernelGGL(dvcp::wbn_bwd_kernel<dvcp::kWbnEval>, dim3(grid), dim3(dvcp::kWbnRows), 0, st, feat, P, params,
                     nullptr, grad_score, grad_feat, ws, nullptr);
  if (int e = dvcp::launch_status("dvcp_weighting_backward")) return e;
  dvcp::fold_rows(ws, grid, dvcp::kWbnGrads, dvcp::kWbnGrads, grad_params, st);
  return dvcp::launch_status("dvcp_weighting_backward(sum)");
}

extern "C" int dvcp_weighting_bn_nparams(void) { return dvcp::kWbnPack; }

extern "C" int64_t dvcp_weighting_bn_stats_workspace_bytes(int P) {
  if (P <= 0) return 0;
  return static_cast<int64_t>(dvcp::wbn_grid(P)) * dvcp::kWbnSumRow * 8;
}

extern "C" int dvcp_weighting_bn_stats(const float* feat, int P, const float* params, int layer, void* workspace,
                                       int64_t ws_bytes, double* sums, void* stream) {
  DVCP_REQUIRE(P >= 0, "dvcp_weighting_bn_stats: P=%d is negative", P);
  DVCP_REQUIRE(layer == 1 || layer == 2, "dvcp_weighting_bn_stats: layer %d out of range (1, 2)", layer);
  DVCP_REQUIRE(params && sums, "dvcp_weighting_bn_stats: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int C = layer == 1 ? 16 : 8;
  if (P == 0) {
    if (hipMemsetAsync(sums, 0, 2 * C * sizeof(double), st) != hipSuccess)
      return dvcp::launch_status("dvcp_weighting_bn_stats(empty)");
    return DVCP_OK;
  }
  DVCP_REQUIRE(feat && workspace, "dvcp_weighting_bn_stats: null pointer");
  const int64_t need = dvcp_weighting_bn_stats_workspace_bytes(P);
  DVCP_REQUIRE(ws_bytes >= need, "dvcp_weighting_bn_stats: workspace of %lld bytes is short of %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(need));
  const int grid = dvcp::wbn_grid(P);
  double* ws = static_cast<double*>(workspace);
  if (layer == 1)
    hipLaunchKernelGGL(dvcp::wbn_stats_kernel<1>, dim3(grid), dim3(dvcp::kWbnRows), 0, st, feat, P, params, ws);
  else
    hipLaunchKernelGGL(dvcp::wbn_stats_kernel<2>, dim3(grid), dim3(dvcp::kWbnRows), 0, st, feat, P, params, ws);
  if (int e = dvcp::launch_status("dvcp_weighting_bn_stats")) return e;
  dvcp::fold_rows(ws, grid, dvcp::kWbnSumRow, 2 * C, sums, st);
  return dvcp::launch_status("dvcp_weighting_bn_stats(sum)");
}

extern "C" int64_t dvcp_weighting_bn_forward_workspace_bytes(int) { return 0; }  // a row per lane, nothing shared

extern "C" int dvcp_weighting_bn_forward(const float* feat, int P, const float* params, float* score, void* stream) {
  DVCP_REQUIRE(P >= 0, "dvcp_weighting_bn_forward: P=%d is negative", P);
  DVCP_REQUIRE(params, "dvcp_weighting_bn_forward: null pointer");
  if (P == 0) return DVCP_OK;
  DVCP_REQUIRE(feat && score, "dvcp_weighting_bn_forward: null pointer");
  hipLaunchKernelGGL(dvcp::wbn_forward_kernel, dim3(dvcp::ceil_div(P, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), feat, P, params, score);
  return dvcp::launch_status("dvcp_weighting_bn_forward");
}

extern "C" int64_t dvcp_weighting_bn_backward_workspace_bytes(int P) {
  if (P <= 0) return 0;
  // one partial row per workgroup: 673 floats (mode 0) or 32 doubles (modes 2, 1), whichever is larger
  static_assert(dvcp::kWbnGrads * 4 >= dvcp::kWbnSumRow * 8, "the gradient row is the larger one");
  return dvcp_weighting_backward_workspace_bytes(P);
}

extern "C" int dvcp_weighting_bn_backward(const float* feat, int P, const float* params, const double* bnstat,
                                          const float* grad_score, int mode, float* grad_feat, void* workspace,
                                          int64_t ws_bytes, double* sums, float* grad_params, void* stream) {
  DVCP_REQUIRE(P >= 0, "dvcp_weighting_bn_backward: P=%d is negative", P);
  DVCP_REQUIRE(mode >= 0 && mode <= 2, "dvcp_weighting_bn_backward: mode %d out of range (0..2)", mode);
  DVCP_REQUIRE(params && bnstat && (mode == 0 ? grad_params != nullptr : sums != nullptr),
               "dvcp_weighting_bn_backward: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int C = mode == 1 ? 16 : 8;
  if (P == 0) {
    const hipError_t e = mode == 0 ? hipMemsetAsync(grad_params, 0, dvcp::kWbnGrads * 4, st)
                                   : hipMemsetAsync(sums, 0, 2 * C * sizeof(double), st);
    if (e != hipSuccess) return dvcp::launch_status("dvcp_weighting_bn_backward(empty)");
    return DVCP_OK;
  }
  DVCP_REQUIRE(feat && grad_score && workspace, "dvcp_weighting_bn_backward: null pointer");
  const int64_t need = dvcp_weighting_bn_backward_workspace_bytes(P);
  DVCP_REQUIRE(ws_bytes >= need, "dvcp_weighting_bn_backward: workspace of %lld bytes is short of %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(need));
  const int grid = dvcp::wbn_grid(P);
  float* wf = static_cast<float*>(workspace);
  double* wd = static_cast<double*>(workspace);
  if (mode == 0) {
    hipLaunchKernelGGL(dvcp::wbn_bwd_kernel<0>, dim3(grid), dim3(dvcp::kWbnRows), 0, st, feat, P, params, bnstat,
                       grad_score, grad_feat, wf, wd);
    if (int e = dvcp::launch_status("dvcp_weighting_bn_backward")) return e;
    dvcp::fold_rows(wf, grid, dvcp::kWbnGrads, dvcp::kWbnGrads, grad_params, st);
    return dvcp::launch_status("dvcp_weighting_bn_backward(sum)");
  }
  if (mode == 1)
    hipLaunchKernelGGL(dvcp::wbn_bwd_kernel<1>, dim3(grid), dim3(dvcp::kWbnRows), 0, st, feat, P, params, bnstat,
                       grad_score, nullptr, wf, wd);
  else
    hipLaunchKernelGGL(dvcp::wbn_bwd_kernel<2>, dim3(grid), dim3(dvcp::kWbnRows), 0, st, feat, P, params, bnstat,
                       grad_score, nullptr, wf, wd);
  if (int e = dvcp::launch_status("dvcp_weighting_bn_backward")) return e;
  dvcp::fold_rows(wd, grid, dvcp::kWbnSumRow, 2 * C, sums, st);
  return dvcp::launch_status("dvcp_weighting_bn_backward(sum)");
}
