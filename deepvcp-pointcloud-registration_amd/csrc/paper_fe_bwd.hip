// paper_fe_bwd.hip -- the paper-faithful mode's extractor backward (DeepVCP paper, Lu et al. ICCV 2019;
// NOT reference parity, like paper.hip): the two links that carry d loss from the stage heads to the
// per-point feature extractor's parameters.
//
//   fp_bwd_kernel         backward of fp_kernel (csrc/paper.hip).  Nothing is saved by the forward:
//                         a tile of 32 rows recomputes the 3-NN and the weights exactly as fp_kernel
//                         does (same fp_key order, expansion_d2(dot3_blas(...)), 1 / (d + 1e-8) summed
//                         in the same order, the N2 == 1 repeat) and then the layer chain with the
//                         forward's arithmetic (the __fmaf_rn order, (acc + b) * scale + shift, the
//                         > 0 test), so the ReLU masks are the forward's own.  Every layer's input and
//                         pre-BN value stay in LDS; the layers are then walked back:
//                           g_a = g_h [a > 0] (g_h where the layer has no ReLU), dbeta += g_a,
//                           dgamma += g_a (z - mean) rstd, g_z = g_a scale, dW += g_z x^T, db += g_z,
//                           g_x = W^T g_z.
//                         Coordinates carry no gradient, so the interpolation weights are constants.
//                         Parameter gradients stay in registers (thread (o, kq) owns dW[o][kq + 4 j])
//                         while min(tiles, 256) workgroups walk tiles t, t + grid, ...; one partial row
//                         per workgroup, folded in index order in fp64 by fold_rows (fold.hip).
//                         grad_p1 has one writer per element.  grad_p2 is a scatter over the three
//                         neighbours: entry e = (b N1 + n) 3 + i gets the key b N2 + idx_i (the
//                         sentinel for i >= min(N2, 3)) and the row w_i g_x[D1..], and segment_sum
//                         (segsum.hip) adds the rows per target point in entry order.
//                         The kernel is a template over four modes (kFbEval: the above, today's bits;
//                         kFbStats / kFbSums / kFbGrad: the batch-statistics passes of training mode,
//                         see the constants below).
//   group_rows_keys_kernel  backward of group_rows_kernel: slot `slot` of centre (b, q) routes its 32
//                         feature columns to point list[bq ns_list + (slot < cnt ? slot : 0)] (padded
//                         slots add to the first hit's row; cnt <= 0 routes nothing).  The kernel only
//                         writes the keys; segment_sum_strided reads the contributions in place from
//                         d rows (35 floats per slot, features at column 3).
//
// No float atomics: two identical calls give identical bits.
#include "common.h"
#include "fp_common.h"

namespace dvcp {

int64_t segment_sum_workspace_bytes(int64_t E, int64_t nrows);
int segment_sum(const uint32_t* keys, const float* contrib, int64_t E, int64_t nrows, int ncol, float* out, void* ws,
                hipStream_t st);
int segment_sum_strided(const uint32_t* keys, const float* contrib, int64_t stride, int64_t offset, int64_t E,
                        int64_t nrows, int ncol, float* out, void* ws, hipStream_t st);

namespace {

constexpr int64_t kFbAlign = 256;
int64_t fb_align(int64_t x) { return (x + kFbAlign - 1) / kFbAlign * kFbAlign; }

constexpr int kFbMaxGrid = 256;        // workgroups (partial rows): one per CU
constexpr int kFbLdX = kFpMaxC + 1;    // row stride of the layer-0 input and of the gradient rows
constexpr int kFbLdH = kFpMaxCo + 1;   // row stride of a layer output
constexpr int kFbLdW = kFpMaxC + 1;    // widest padded weight row
constexpr int kFbNk0 = kFpMaxC / 4;    // dW elements per thread, layer 0 (input up to 128 wide)
constexpr int kFbNk = kFpMaxCo / 4;    // ... layers 1..3 (input up to 64 wide)
static_assert(kFpThreads == 4 * kFpMaxCo, "thread (o, kq): o = tid & 63 output channel, kq = tid >> 6");
static_assert((kFpTile + 8) * 4 == kFpRows * kFbLdX, "the gradient rows reuse the 3-NN tile's LDS");

int64_t fb_tiles(int B, int N1) { return static_cast<int64_t>(B) * ceil_div(N1, kFpRows); }
int fb_grid(int64_t tiles) { return static_cast<int>(tiles < kFbMaxGrid ? tiles : kFbMaxGrid); }
int fb_nparams(int nlayer, const int* chans) {
  int P = 0;
  for (int l = 0; l < nlayer; ++l) P += chans[l] * chans[l + 1] + 3 * chans[l + 1];
  return P;
}

// One layer's parameter-gradient terms of a tile, rows in order.  Thread (o, kq) owns dW[o][kq + 4 j].
template <int NK>
__device__ __forceinline__ void fb_accumulate(float (&dW)[NK], float& db, float& dg, float& dbe,
                                              const float* __restrict__ gA, const float* __restrict__ gZ,
                                              const float* __restrict__ zl, const float* __restrict__ xin, int ldx,
                                              int ci, float mean, float rstd, int o, int kq) {
  for (int rr = 0; rr < kFpRows; ++rr) {
    const float ga = gA[rr * kFbLdX + o];
    const float g = gZ[rr * kFbLdH + o];
    dbe += ga;
    dg = __fmaf_rn(ga, (zl[rr * kFbLdH + o] - mean) * rstd, dg);
    db += g;
    const float* x = xin + rr * ldx + kq;
#pragma unroll
    for (int j = 0; j < NK; ++j)
      if (kq + 4 * j < ci) dW[j] = __fmaf_rn(g, x[4 * j], dW[j]);
  }
}

template <int NK>
__device__ __forceinline__ void fb_store(const float (&dW)[NK], float db, float dg, float dbe, float* __restrict__ o_l,
                                         int ci, int co, int o, int kq) {
  if (o >= co) return;
#pragma unroll
  for (int j = 0; j < NK; ++j)
    if (kq + 4 * j < ci) o_l[o * ci + kq + 4 * j] = dW[j];
  if (kq == 0) {
    o_l[ci * co + o] = db;
    o_l[ci * co + co + o] = dg;
    o_l[ci * co + 2 * co + o] = dbe;
  }
}

// fp_bwd_kernel's modes.  kFbEval: eval-mode BN (running statistics), the gradient pass.  The other
// three are the batch-statistics passes (training mode; torch's batch-norm backward,
// dz_l = scale_l (g_a - A_l/M - xhat_l B_l/M), xhat = (z - mean) rstd, A_l = sum g_a, B_l = sum g_a xhat):
// kFbStats: sum z | sum z^2 of layer kl's conv output over the B N1 rows (the forward chain up to kl);
// kFbSums: A | B of layer kl, given those of the layers above; kFbGrad: the gradient pass, given all.
// Every such sum is taken in fp64 from the single entries: thread (o, kq) owns channel o over the rows
// kq, kq + 4, ... of every tile its workgroup walks; one partial row per (workgroup, kq), folded in
// index order by fb_fold_sums_kernel.  xhat and the mean terms are evaluated in fp64 from fp64
// statistics (bn64: per layer mean | rstd | A/M | B/M; 0 | 1 | 0 | 0 for a fused fc, a plain layer).
constexpr int kFbEval = -1, kFbGrad = 0, kFbSums = 1, kFbStats = 2;
constexpr int kFbSumRow = 2 * kFpMaxCo;  // doubles per partial row of sums

// the walked layer's mean | rstd | A/M | B/M (batch-statistics modes only: no LDS in the eval kernel)
__device__ __forceinline__ double* fb_bn_vectors() {
  __shared__ double v[4 * kFpMaxCo];
  return v;
}

// out[e], e < 2 co: sum over the n partial rows, k ascending (first co entries, then those at kFpMaxCo)
__global__ __launch_bounds__(128) void fb_fold_sums_kernel(const double* __restrict__ part, int n, int co,
                                                           double* __restrict__ out) {
  const int e = threadIdx.x;
  if (e >= 2 * co) return;
  const int src = e < co ? e : kFpMaxCo + (e - co);
  double acc = 0.0;
  for (int k = 0; k < n; ++k) acc += part[static_cast<int64_t>(k) * kFbSumRow + src];
  out[e] = acc;
}

template <int MODE>
__global__ __launch_bounds__(kFpThreads) void fp_bwd_kernel(
    PointsView<float> xyz1, int N1, PointsView<float> xyz2, int N2, int B, const float* __restrict__ p1, int64_t p1b,
    int64_t p1d, int64_t p1n, int D1, const float* __restrict__ p2, int64_t p2b, int64_t p2n, int D2, FpLayers lay,
    const float* __restrict__ params, const float* __restrict__ bnstat, const float* __restrict__ gout,
    float* __restrict__ gp1, uint32_t* __restrict__ keys, float* __restrict__ contrib, int nparams,
    float* __restrict__ partial, const double* __restrict__ bn64, int kl, double* __restrict__ sum_partial) {
  __shared__ float4 tile[kFpTile + 8];                      // 3-NN scan; afterwards the gradient rows gA
  __shared__ float x0[kFpRows * kFbLdX];                    // layer-0 input rows
  __shared__ float hb[kFpMaxL - 1][kFpRows * kFbLdH];       // inputs of layers 1..L-1
  __shared__ float zb[kFpMaxL][kFpRows * kFbLdH];           // acc + b of every layer
  __shared__ float gZ[kFpRows * kFbLdH];                    // g_z of the layer being walked
  __shared__ float wsh[kFpMaxCo * kFbLdW];                  // W (co x ci), rows padded by one
  __shared__ float bsh[3][kFpMaxCo];
  __shared__ int nidx[kFpRows][3];
  __shared__ float nwt[kFpRows][3];
  float* gA = reinterpret_cast<float*>(tile);               // (32, kFbLdX): g_a of a layer, then g_x

  const int tid = threadIdx.x;
  const int row = tid >> 3, part = tid & 7;
  const int o = tid & 63, kq = tid >> 6;
  const int L = lay.L, C0 = D1 + D2;
  const int nk = N2 < 3 ? N2 : 3;
  const int tpb = (N1 + kFpRows - 1) / kFpRows;
  const int tiles = B * tpb;

  float dW0[kFbNk0], dW1[kFbNk], dW2[kFbNk], dW3[kFbNk];
  float db[kFpMaxL], dg[kFpMaxL], dbe[kFpMaxL];
#pragma unroll
  for (int j = 0; j < kFbNk0; ++j) dW0[j] = 0.f;
#pragma unroll
  for (int j = 0; j < kFbNk; ++j) dW1[j] = dW2[j] = dW3[j] = 0.f;
#pragma unroll
  for (int l = 0; l < kFpMaxL; ++l) db[l] = dg[l] = dbe[l] = 0.f;
  double sumA = 0.0, sumB = 0.0;             // kFbStats: sum z, sum z^2; kFbSums: A, B (channel o, rows kq + 4 j)
  const int Lf = MODE == kFbStats ? kl : L;  // layers of the forward chain this pass needs

  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int b = t / tpb, r0 = (t % tpb) * kFpRows;
    const int n = r0 + row;
    // ---- the 3-NN and the weights, as fp_kernel computes them
    float cx = 0.f, cy = 0.f, cz = 0.f;
    if (n < N1) {
      cx = xyz1.at(b, 0, n);
      cy = xyz1.at(b, 1, n);
      cz = xyz1.at(b, 2, n);
    }
    const float ssc = sumsq3(cx, cy, cz);
    uint64_t k3[3] = {~0ull, ~0ull, ~0ull};
    for (int t0 = 0; t0 < N2; t0 += kFpTile) {
      const int nt = min(kFpTile, N2 - t0);
      __syncthreads();  // the previous tile's readers (of gA too) are done
      for (int j = tid; j < nt; j += kFpThreads) {
        const float x = xyz2.at(b, 0, t0 + j), y = xyz2.at(b, 1, t0 + j), z = xyz2.at(b, 2, t0 + j);
        tile[j] = make_float4(x, y, z, sumsq3(x, y, z));
      }
      __syncthreads();
      for (int j = part; j < nt; j += 8) {
        const float4 p = tile[j];
        top3_insert(k3, fp_key(expansion_d2(dot3_blas(cx, cy, cz, p.x, p.y, p.z), ssc, p.w), t0 + j));
      }
    }
#pragma unroll
    for (int off = 1; off < 8; off <<= 1) {
      uint64_t ok[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) ok[i] = __shfl_xor(k3[i], off, kWave);
#pragma unroll
      for (int i = 0; i < 3; ++i) top3_insert(k3, ok[i]);
    }
    if (part == 0) {
      float w[3] = {0.f, 0.f, 0.f};
      int id[3] = {0, 0, 0};
      if (N2 == 1) {
        w[0] = 1.0f;
      } else {
        float rc[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          id[i] = i < nk ? static_cast<int>(k3[i] & 0xFFFFFFFFull) : 0;
          rc[i] = i < nk ? 1.0f / (fp_key_d2(k3[i]) + 1e-8f) : 0.f;
        }
        float norm = rc[0] + rc[1];
        if (nk > 2) norm = norm + rc[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) w[i] = i < nk ? rc[i] / norm : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        nidx[row][i] = id[i];
        nwt[row][i] = w[i];
      }
    }
    __syncthreads();
    // ---- layer-0 rows: [points1, interpolated]
    const float* q2 = p2 + b * p2b;
    for (int e = tid; e < kFpRows * C0; e += kFpThreads) {
      const int rr = e / C0, c = e % C0, nn = r0 + rr;
      float v = 0.f;
      if (nn < N1) {
        if (c < D1) {
          v = p1[b * p1b + c * p1d + nn * p1n];
        } else {
          const int cc = c - D1;
          v = q2[nidx[rr][0] * p2n + cc] * nwt[rr][0];
          if (nk > 1) v = v + q2[nidx[rr][1] * p2n + cc] * nwt[rr][1];
          if (nk > 2) v = v + q2[nidx[rr][2] * p2n + cc] * nwt[rr][2];
        }
      }
      x0[rr * kFbLdX + c] = v;
    }
    // ---- the layer chain, the forward's arithmetic; the last layer turns grad_out into its g_a
    const float* P = params;
    for (int l = 0; l < Lf; ++l) {
      const int ci = lay.ch[l], co = lay.ch[l + 1];
      const float* in = l == 0 ? x0 : hb[l - 1];
      const int ldi = l == 0 ? kFbLdX : kFbLdH;
      __syncthreads();
      for (int e = tid; e < ci * co; e += kFpThreads) wsh[(e / ci) * (ci + 1) + e % ci] = P[e];
      for (int e = tid; e < co; e += kFpThreads) {
        bsh[0][e] = P[ci * co + e];
        bsh[1][e] = P[ci * co + co + e];
        bsh[2][e] = P[ci * co + 2 * co + e];
      }
      __syncthreads();
      for (int e = tid; e < kFpRows * co; e += kFpThreads) {
        const int rr = e / co, oc = e % co;
        float acc = 0.f;
        for (int k = 0; k < ci; ++k) acc = __fmaf_rn(wsh[oc * (ci + 1) + k], in[rr * ldi + k], acc);
        const float z = acc + bsh[0][oc];
        float v = z * bsh[1][oc] + bsh[2][oc];
        zb[l][rr * kFbLdH + oc] = z;
        if (l < L - 1) {
          if (lay.relu[l]) v = v > 0.f ? v : 0.f;
          hb[l][rr * kFbLdH + oc] = v;
        } else if constexpr (MODE != kFbStats) {
          const int nn = r0 + rr;
          float g = nn < N1 ? gout[(static_cast<int64_t>(b) * N1 + nn) * co + oc] : 0.f;
          if (lay.relu[l] && !(v > 0.f)) g = 0.f;
          gA[rr * kFbLdX + oc] = g;
        }
      }
      if (l < L - 1) P += ci * co + 3 * co;
    }
    if constexpr (MODE == kFbStats) {  // layer kl's z over the tile's real rows; nothing is walked back
      __syncthreads();
      if (o < lay.ch[kl]) {
        for (int rr = kq; rr < kFpRows && r0 + rr < N1; rr += 4) {
          const double zd = static_cast<double>(zb[kl - 1][rr * kFbLdH + o]);
          sumA += zd;
          sumB += zd * zd;
        }
      }
      continue;
    }
    // ---- the walk back; P points at layer l's parameters, wsh / bsh hold layer L - 1's
    const bool want_x = gp1 || contrib;
    int soff = 0;
    for (int l = 0; l < L - 1; ++l) soff += 2 * lay.ch[l + 1];
    for (int l = L - 1; l >= 0; --l) {
      const int ci = lay.ch[l], co = lay.ch[l + 1];
      __syncthreads();  // gA (this layer's g_a) is complete
      if (l < L - 1) {
        for (int e = tid; e < ci * co; e += kFpThreads) wsh[(e / ci) * (ci + 1) + e % ci] = P[e];
        for (int e = tid; e < co; e += kFpThreads) bsh[1][e] = P[ci * co + co + e];
        __syncthreads();
      }
      if constexpr (MODE == kFbEval) {
        for (int e = tid; e < kFpRows * co; e += kFpThreads) {
          const int rr = e / co, oc = e % co;
          gZ[rr * kFbLdH + oc] = gA[rr * kFbLdX + oc] * bsh[1][oc];
        }
      } else {
        double* bnv = fb_bn_vectors();
        for (int e = tid; e < 4 * co; e += kFpThreads) bnv[(e / co) * kFpMaxCo + e % co] = bn64[2 * soff + e];
        __syncthreads();
        if (MODE == kFbSums && l == kl - 1) {  // this layer's A | B, then on to the next tile
          if (o < co) {
            for (int rr = kq; rr < kFpRows; rr += 4) {
              const double ga = static_cast<double>(gA[rr * kFbLdX + o]);
              const double xh = (static_cast<double>(zb[l][rr * kFbLdH + o]) - bnv[o]) * bnv[kFpMaxCo + o];
              sumA += ga;
              sumB += ga * xh;
            }
          }
          break;
        }
        for (int e = tid; e < kFpRows * co; e += kFpThreads) {
          const int rr = e / co, oc = e % co;
          float gz = 0.f;  // rows past N1 are no entries of the batch
          if (r0 + rr < N1) {
            const double xh = (static_cast<double>(zb[l][rr * kFbLdH + oc]) - bnv[oc]) * bnv[kFpMaxCo + oc];
            gz = static_cast<float>(static_cast<double>(bsh[1][oc]) *
                                    ((static_cast<double>(gA[rr * kFbLdX + oc]) - bnv[2 * kFpMaxCo + oc]) -
                                     xh * bnv[3 * kFpMaxCo + oc]));
          }
          gZ[rr * kFbLdH + oc] = gz;
        }
      }
      __syncthreads();
      if (MODE != kFbSums && o < co) {
        // (kFbGrad: the fp32 dgamma / dbeta are by-products; the caller takes B and A of the sums passes)
        const float mean = MODE == kFbEval ? bnstat[soff + o] : static_cast<float>(bn64[2 * soff + o]);
        const float rstd = MODE == kFbEval ? bnstat[soff + co + o] : static_cast<float>(bn64[2 * soff + co + o]);
        switch (l) {
          case 0:
            fb_accumulate<kFbNk0>(dW0, db[0], dg[0], dbe[0], gA, gZ, zb[0], x0, kFbLdX, ci, mean, rstd, o, kq);
            break;
          case 1:
            fb_accumulate<kFbNk>(dW1, db[1], dg[1], dbe[1], gA, gZ, zb[1], hb[0], kFbLdH, ci, mean, rstd, o, kq);
            break;
          case 2:
            fb_accumulate<kFbNk>(dW2, db[2], dg[2], dbe[2], gA, gZ, zb[2], hb[1], kFbLdH, ci, mean, rstd, o, kq);
            break;
          default:
            fb_accumulate<kFbNk>(dW3, db[3], dg[3], dbe[3], gA, gZ, zb[3], hb[2], kFbLdH, ci, mean, rstd, o, kq);
            break;
        }
      }
      __syncthreads();  // gA's readers are done: it now takes g_x = W^T g_z
      if (l > 0 || want_x) {
        for (int e = tid; e < kFpRows * ci; e += kFpThreads) {
          const int rr = e / ci, k = e % ci;
          float acc = 0.f;
          for (int oc = 0; oc < co; ++oc) acc = __fmaf_rn(wsh[oc * (ci + 1) + k], gZ[rr * kFbLdH + oc], acc);
          if (l > 0 && lay.relu[l - 1] && !(hb[l - 1][rr * kFbLdH + k] > 0.f)) acc = 0.f;  // the layer below's mask
          gA[rr * kFbLdX + k] = acc;
        }
      }
      if (l > 0) {
        P -= lay.ch[l - 1] * ci + 3 * ci;
        soff -= 2 * ci;
      }
    }
    __syncthreads();
    if constexpr (MODE == kFbSums) continue;
    // ---- d points1 (one writer per element) and the three neighbours' entries of d points2
    if (gp1) {
      for (int e = tid; e < kFpRows * D1; e += kFpThreads) {
        const int rr = e / D1, c = e % D1, nn = r0 + rr;
        if (nn < N1) gp1[(static_cast<int64_t>(b) * N1 + nn) * D1 + c] = gA[rr * kFbLdX + c];
      }
    }
    if (contrib) {
      const uint32_t sentinel = static_cast<uint32_t>(B) * static_cast<uint32_t>(N2);
      for (int e = tid; e < kFpRows * 3; e += kFpThreads) {
        const int rr = e / 3, i = e % 3, nn = r0 + rr;
        if (nn < N1)
          keys[(static_cast<int64_t>(b) * N1 + nn) * 3 + i] =
              i < nk ? static_cast<uint32_t>(b) * static_cast<uint32_t>(N2) + static_cast<uint32_t>(nidx[rr][i])
                     : sentinel;
      }
      for (int e = tid; e < kFpRows * 3 * D2; e += kFpThreads) {
        const int rr = e / (3 * D2), i = (e / D2) % 3, cc = e % D2, nn = r0 + rr;
        if (nn < N1 && i < nk)
          contrib[((static_cast<int64_t>(b) * N1 + nn) * 3 + i) * D2 + cc] = nwt[rr][i] * gA[rr * kFbLdX + D1 + cc];
      }
    }
  }
  if constexpr (MODE == kFbStats || MODE == kFbSums) {
    double* so = sum_partial + (static_cast<int64_t>(blockIdx.x) * 4 + kq) * kFbSumRow;
    so[o] = sumA;
    so[kFpMaxCo + o] = sumB;
    return;
  }
  // ---- this workgroup's partial row: per layer dW | db | dgamma | dbeta
  float* po = partial + static_cast<int64_t>(blockIdx.x) * nparams;
  fb_store<kFbNk0>(dW0, db[0], dg[0], dbe[0], po, lay.ch[0], lay.ch[1], o, kq);
  po += lay.ch[0] * lay.ch[1] + 3 * lay.ch[1];
  if (L > 1) {
    fb_store<kFbNk>(dW1, db[1], dg[1], dbe[1], po, lay.ch[1], lay.ch[2], o, kq);
    po += lay.ch[1] * lay.ch[2] + 3 * lay.ch[2];
  }
  if (L > 2) {
    fb_store<kFbNk>(dW2, db[2], dg[2], dbe[2], po, lay.ch[2], lay.ch[3], o, kq);
    po += lay.ch[2] * lay.ch[3] + 3 * lay.ch[3];
  }
  if (L > 3) fb_store<kFbNk>(dW3, db[3], dg[3], dbe[3], po, lay.ch[3], lay.ch[4], o, kq);
}

// key[e] of slot e = (bq, slot) of d rows: the point its feature columns were gathered from.
__global__ __launch_bounds__(256) void group_rows_keys_kernel(const int32_t* __restrict__ count,
                                                              const int32_t* __restrict__ list, int ns_list,
                                                              int ns_out, int Q, int N, int64_t total,
                                                              uint32_t sentinel, uint32_t* __restrict__ keys) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int slot = static_cast<int>(i % ns_out);
  const int64_t bq = i / ns_out;
  const int cnt = count[bq];
  uint32_t key = sentinel;
  if (cnt > 0) {
    const int n = list[bq * ns_list + (slot < cnt && slot < ns_list ? slot : 0)];
    if (n >= 0 && n < N) key = static_cast<uint32_t>(bq / Q) * static_cast<uint32_t>(N) + static_cast<uint32_t>(n);
  }
  keys[i] = key;
}

}  // namespace
}  // namespace dvcp

extern "C" int64_t dvcp_feature_propagation_backward_workspace_bytes(int B, int N1, int N2, int D2, int nlayer,
                                                                     const int* chans, int want_p2) {
  if (B < 0 || N1 < 0 || N2 < 1 || D2 < 1 || !chans || nlayer < 1 || nlayer > dvcp::kFpMaxL) return -1;
  const int64_t tiles = dvcp::fb_tiles(B, N1);
  if (tiles == 0) return 0;
  int64_t need = dvcp::fb_align(static_cast<int64_t>(dvcp::fb_grid(tiles)) * dvcp::fb_nparams(nlayer, chans) * 4);
  if (want_p2) {
    const int64_t E = static_cast<int64_t>(B) * N1 * 3;
    const int64_t seg = dvcp::segment_sum_workspace_bytes(E, static_cast<int64_t>(B) * N2);
    if (seg < 0) return -1;
    need += dvcp::fb_align(E * 4) + dvcp::fb_align(E * D2 * 4) + seg;
  }
  return need;
}

extern "C" int dvcp_feature_propagation_backward(
    const float* xyz1, int64_t x1b, int64_t x1c, int64_t x1n, int N1, const float* xyz2, int64_t x2b, int64_t x2c,
    int64_t x2n, int N2, int B, const float* p1, int64_t p1b, int64_t p1d, int64_t p1n, int D1, const float* p2,
    int64_t p2b, int64_t p2n, int D2, int nlayer, const int* chans, const int* relu, const float* params,
    const float* bnstat, const float* grad_out, float* grad_p1, float* grad_p2, void* workspace, int64_t ws_bytes,
    float* grad_params, void* stream) {
  DVCP_REQUIRE(chans && relu && params && bnstat && grad_params, "dvcp_feature_propagation_backward: null pointer");
  DVCP_REQUIRE(N1 >= 0 && N2 >= 1 && B >= 0 && B <= 65535 && D1 >= 0 && D2 >= 1,
               "dvcp_feature_propagation_backward: bad sizes N1=%d N2=%d B=%d D1=%d D2=%d", N1, N2, B, D1, D2);
  DVCP_REQUIRE(N2 != 2, "dvcp_feature_propagation_backward: N2 = 2 (refused like the forward: the reference's "
               "weight.view(B, N, 3, 1), pointnet2_utils.py:303, fails for two interpolation points)");
  DVCP_REQUIRE(nlayer >= 1 && nlayer <= dvcp::kFpMaxL, "dvcp_feature_propagation_backward: 1..%d layers",
               dvcp::kFpMaxL);
  DVCP_REQUIRE(chans[0] == D1 + D2, "dvcp_feature_propagation_backward: chans[0]=%d != D1 + D2", chans[0]);
  dvcp::FpLayers lay{};
  lay.L = nlayer;
  for (int l = 0; l <= nlayer; ++l) {
    DVCP_REQUIRE(chans[l] >= 1 && chans[l] <= (l == 0 ? dvcp::kFpMaxC : dvcp::kFpMaxCo),
                 "dvcp_feature_propagation_backward: layer width %d out of range", chans[l]);
    lay.ch[l] = chans[l];
  }
  for (int l = 0; l < nlayer; ++l) lay.relu[l] = relu[l] != 0;
  DVCP_REQUIRE(!grad_p2 || D2 == 32 || D2 == 64,
               "dvcp_feature_propagation_backward: grad_p2 with D2=%d (segment_sum takes 32 or 64 columns)", D2);
  const int64_t E = static_cast<int64_t>(B) * N1 * 3;
  DVCP_REQUIRE(E <= 0x7FFFFFFF && static_cast<int64_t>(B) * N2 <= 0x7FFFFFFF,
               "dvcp_feature_propagation_backward: B N1 3 and B N2 must stay below 2^31");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int np = dvcp::fb_nparams(nlayer, chans);
  const int64_t tiles = dvcp::fb_tiles(B, N1);
  if (tiles == 0) {  // no row: zero parameter gradients, no neighbour entry
    if (hipMemsetAsync(grad_params, 0, static_cast<size_t>(np) * 4, st) != hipSuccess ||
        (grad_p2 && B > 0 && hipMemsetAsync(grad_p2, 0, static_cast<size_t>(B) * N2 * D2 * 4, st) != hipSuccess))
      return dvcp::launch_status("dvcp_feature_propagation_backward(empty)");
    return DVCP_OK;
  }
  DVCP_REQUIRE(xyz1 && xyz2 && p2 && (D1 == 0 || p1) && grad_out && workspace,
               "dvcp_feature_propagation_backward: null pointer");
  const int64_t need =
      dvcp_feature_propagation_backward_workspace_bytes(B, N1, N2, D2, nlayer, chans, grad_p2 != nullptr);
  DVCP_REQUIRE(need >= 0, "dvcp_feature_propagation_backward: workspace size query failed");
  DVCP_REQUIRE(ws_bytes >= need, "dvcp_feature_propagation_backward: workspace of %lld bytes is short of %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(need));
  const int grid = dvcp::fb_grid(tiles);
  char* w = static_cast<char*>(workspace);
  float* partial = reinterpret_cast<float*>(w);
  w += dvcp::fb_align(static_cast<int64_t>(grid) * np * 4);
  uint32_t* keys = nullptr;
  float* contrib = nullptr;
  if (grad_p2) {
    keys = reinterpret_cast<uint32_t*>(w);
    w += dvcp::fb_align(E * 4);
    contrib = reinterpret_cast<float*>(w);
    w += dvcp::fb_align(E * D2 * 4);
  }
  hipLaunchKernelGGL(dvcp::fp_bwd_kernel<dvcp::kFbEval>, dim3(grid), dim3(dvcp::kFpThreads), 0, st,
                     dvcp::PointsView<float>{xyz1, x1b, x1c, x1n}, N1, dvcp::PointsView<float>{xyz2, x2b, x2c, x2n}, N2,
                     B, p1, p1b, p1d, p1n, D1, p2, p2b, p2n, D2, lay, params, bnstat, grad_out, grad_p1, keys, contrib,
                     np, partial, nullptr, 0, nullptr);
  if (int e = dvcp::launch_status("dvcp_feature_propagation_backward")) return e;
  dvcp::fold_rows(partial, grid, np, np, grad_params, st);
  if (int e = dvcp::launch_status("dvcp_feature_propagation_backward(sum)")) return e;
  if (grad_p2) return dvcp::segment_sum(keys, contrib, E, static_cast<int64_t>(B) * N2, D2, grad_p2, w, st);
  return DVCP_OK;
}

// ------------------------------------------------- feature propagation under batch statistics
static int fb_bn_layers(const char* who, int N1, int N2, int B, int D1, int D2, int nlayer, const int* chans,
                        const int* relu, dvcp::FpLayers* lay) {
  DVCP_REQUIRE(chans && relu, "%s: null pointer", who);
  DVCP_REQUIRE(N1 >= 0 && N2 >= 1 && B >= 0 && B <= 65535 && D1 >= 0 && D2 >= 1,
               "%s: bad sizes N1=%d N2=%d B=%d D1=%d D2=%d", who, N1, N2, B, D1, D2);
  DVCP_REQUIRE(N2 != 2, "%s: N2 = 2 (refused like the forward: the reference's weight.view(B, N, 3, 1), "
               "pointnet2_utils.py:303, fails for two interpolation points)", who);
  DVCP_REQUIRE(nlayer >= 1 && nlayer <= dvcp::kFpMaxL, "%s: 1..%d layers", who, dvcp::kFpMaxL);
  DVCP_REQUIRE(chans[0] == D1 + D2, "%s: chans[0]=%d != D1 + D2", who, chans[0]);
  lay->L = nlayer;
  for (int l = 0; l <= nlayer; ++l) {
    DVCP_REQUIRE(chans[l] >= 1 && chans[l] <= (l == 0 ? dvcp::kFpMaxC : dvcp::kFpMaxCo),
                 "%s: layer width %d out of range", who, chans[l]);
    lay->ch[l] = chans[l];
  }
  for (int l = 0; l < nlayer; ++l) lay->relu[l] = relu[l] != 0;
  DVCP_REQUIRE(static_cast<int64_t>(B) * N1 * 3 <= 0x7FFFFFFF && static_cast<int64_t>(B) * N2 <= 0x7FFFFFFF,
               "%s: B N1 3 and B N2 must stay below 2^31", who);
  return DVCP_OK;
}

static int64_t fb_sum_bytes(int64_t tiles) {
  return dvcp::fb_align(static_cast<int64_t>(dvcp::fb_grid(tiles)) * 4 * dvcp::kFbSumRow * 8);
}

extern "C" int64_t dvcp_feature_propagation_bn_stats_workspace_bytes(int B, int N1) {
  if (B < 0 || N1 < 0) return -1;
  const int64_t tiles = dvcp::fb_tiles(B, N1);
  return tiles == 0 ? 0 : fb_sum_bytes(tiles);
}

extern "C" int dvcp_feature_propagation_bn_stats(
    const float* xyz1, int64_t x1b, int64_t x1c, int64_t x1n, int N1, const float* xyz2, int64_t x2b, int64_t x2c,
    int64_t x2n, int N2, int B, const float* p1, int64_t p1b, int64_t p1d, int64_t p1n, int D1, const float* p2,
    int64_t p2b, int64_t p2n, int D2, int nlayer, const int* chans, const int* relu, const float* params, int layer,
    void* workspace, int64_t ws_bytes, double* sums, void* stream) {
  const char* who = "dvcp_feature_propagation_bn_stats";
  dvcp::FpLayers lay{};
  if (int e = fb_bn_layers(who, N1, N2, B, D1, D2, nlayer, chans, relu, &lay)) return e;
  DVCP_REQUIRE(params && sums, "%s: null pointer", who);
  DVCP_REQUIRE(layer >= 1 && layer <= nlayer, "%s: layer %d of %d", who, layer, nlayer);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int co = chans[layer];
  const int64_t tiles = dvcp::fb_tiles(B, N1);
  if (tiles == 0) {
    if (hipMemsetAsync(sums, 0, 2 * co * sizeof(double), st) != hipSuccess)
      return dvcp::launch_status("dvcp_feature_propagation_bn_stats(empty)");
    return DVCP_OK;
  }
  DVCP_REQUIRE(xyz1 && xyz2 && p2 && (D1 == 0 || p1) && workspace, "%s: null pointer", who);
  const int64_t need = fb_sum_bytes(tiles);
  DVCP_REQUIRE(ws_bytes >= need, "%s: workspace of %lld bytes is short of %lld", who, static_cast<long long>(ws_bytes),
               static_cast<long long>(need));
  const int grid = dvcp::fb_grid(tiles);
  double* sp = static_cast<double*>(workspace);
  hipLaunchKernelGGL(dvcp::fp_bwd_kernel<dvcp::kFbStats>, dim3(grid), dim3(dvcp::kFpThreads), 0, st,
                     dvcp::PointsView<float>{xyz1, x1b, x1c, x1n}, N1, dvcp::PointsView<float>{xyz2, x2b, x2c, x2n}, N2,
                     B, p1, p1b, p1d, p1n, D1, p2, p2b, p2n, D2, lay, params, nullptr, nullptr, nullptr, nullptr,
                     nullptr, 0, nullptr, nullptr, layer, sp);
  if (int e = dvcp::launch_status(who)) return e;
  hipLaunchKernelGGL(dvcp::fb_fold_sums_kernel, dim3(1), dim3(128), 0, st, sp, grid * 4, co, sums);
  return dvcp::launch_status("dvcp_feature_propagation_bn_stats(sum)");
}

extern "C" int64_t dvcp_feature_propagation_bn_backward_workspace_bytes(int B, int N1, int N2, int D2, int nlayer,
                                                                        const int* chans, int want_p2) {
  const int64_t need = dvcp_feature_propagation_backward_workspace_bytes(B, N1, N2, D2, nlayer, chans, want_p2);
  if (need <= 0) return need;
  return need + fb_sum_bytes(dvcp::fb_tiles(B, N1));
}

extern "C" int dvcp_feature_propagation_bn_backward(
    const float* xyz1, int64_t x1b, int64_t x1c, int64_t x1n, int N1, const float* xyz2, int64_t x2b, int64_t x2c,
    int64_t x2n, int N2, int B, const float* p1, int64_t p1b, int64_t p1d, int64_t p1n, int D1, const float* p2,
    int64_t p2b, int64_t p2n, int D2, int nlayer, const int* chans, const int* relu, const float* params,
    const double* bnstat, const float* grad_out, int mode, float* grad_p1, float* grad_p2, void* workspace,
    int64_t ws_bytes, double* sums, float* grad_params, void* stream) {
  const char* who = "dvcp_feature_propagation_bn_backward";
  dvcp::FpLayers lay{};
  if (int e = fb_bn_layers(who, N1, N2, B, D1, D2, nlayer, chans, relu, &lay)) return e;
  DVCP_REQUIRE(mode >= 0 && mode <= nlayer, "%s: mode %d of %d", who, mode, nlayer);
  DVCP_REQUIRE(params && bnstat && (mode == 0 ? grad_params != nullptr : sums != nullptr), "%s: null pointer", who);
  if (mode != 0) grad_p1 = grad_p2 = nullptr;
  DVCP_REQUIRE(!grad_p2 || D2 == 32 || D2 == 64, "%s: grad_p2 with D2=%d (segment_sum takes 32 or 64 columns)", who,
               D2);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int np = dvcp::fb_nparams(nlayer, chans);
  const int64_t tiles = dvcp::fb_tiles(B, N1);
  if (tiles == 0) {
    bool ok = true;
    if (mode != 0) {
      ok = hipMemsetAsync(sums, 0, 2 * chans[mode] * sizeof(double), st) == hipSuccess;
    } else {
      ok = hipMemsetAsync(grad_params, 0, static_cast<size_t>(np) * 4, st) == hipSuccess &&
           (!grad_p2 || B == 0 ||
            hipMemsetAsync(grad_p2, 0, static_cast<size_t>(B) * N2 * D2 * 4, st) == hipSuccess);
    }
    return ok ? DVCP_OK : dvcp::launch_status("dvcp_feature_propagation_bn_backward(empty)");
  }
  DVCP_REQUIRE(xyz1 && xyz2 && p2 && (D1 == 0 || p1) && grad_out && workspace, "%s: null pointer", who);
  const int64_t need =
      dvcp_feature_propagation_bn_backward_workspace_bytes(B, N1, N2, D2, nlayer, chans, grad_p2 != nullptr);
  DVCP_REQUIRE(need >= 0, "%s: workspace size query failed", who);
  DVCP_REQUIRE(ws_bytes >= need, "%s: workspace of %lld bytes is short of %lld", who, static_cast<long long>(ws_bytes),
               static_cast<long long>(need));
  const int grid = dvcp::fb_grid(tiles);
  const int64_t E = static_cast<int64_t>(B) * N1 * 3;
  char* w = static_cast<char*>(workspace);
  double* sp = reinterpret_cast<double*>(w);
  w += fb_sum_bytes(tiles);
  float* partial = reinterpret_cast<float*>(w);
  w += dvcp::fb_align(static_cast<int64_t>(grid) * np * 4);
  uint32_t* keys = nullptr;
  float* contrib = nullptr;
  if (grad_p2) {
    keys = reinterpret_cast<uint32_t*>(w);
    w += dvcp::fb_align(E * 4);
    contrib = reinterpret_cast<float*>(w);
    w += dvcp::fb_align(E * D2 * 4);
  }
  const dvcp::PointsView<float> v1{xyz1, x1b, x1c, x1n}, v2{xyz2, x2b, x2c, x2n};
  if (mode != 0) {
    hipLaunchKernelGGL(dvcp::fp_bwd_kernel<dvcp::kFbSums>, dim3(grid), dim3(dvcp::kFpThreads), 0, st, v1, N1, v2, N2, B,
                       p1, p1b, p1d, p1n, D1, p2, p2b, p2n, D2, lay, params, nullptr, grad_out, nullptr, nullptr,
                       nullptr, np, nullptr, bnstat, mode, sp);
    if (int e = dvcp::launch_status(who)) return e;
    hipLaunchKernelGGL(dvcp::fb_fold_sums_kernel, dim3(1), dim3(128), 0, st, sp, grid * 4, chans[mode], sums);
    return dvcp::launch_status("dvcp_feature_propagation_bn_backward(sum)");
  }
  hipLaunchKernelGGL(dvcp::fp_bwd_kernel<dvcp::kFbGrad>, dim3(grid), dim3(dvcp::kFpThreads), 0, st, v1, N1, v2, N2, B,
                     p1, p1b, p1d, p1n, D1, p2, p2b, p2n, D2, lay, params, nullptr, grad_out, grad_p1, keys, contrib,
                     np, partial, bnstat, 0, nullptr);
  if (int e = dvcp::launch_status(who)) return e;
  dvcp::fold_rows(partial, grid, np, np, grad_params, st);
  if (int e = dvcp::launch_status("dvcp_feature_propagation_bn_backward(fold)")) return e;
  if (grad_p2) return dvcp::segment_sum(keys, contrib, E, static_cast<int64_t>(B) * N2, D2, grad_p2, w, st);
  return DVCP_OK;
}

extern "C" int64_t dvcp_group_rows_backward_workspace_bytes(int B, int Q, int N, int ns_out) {
  if (B < 0 || Q < 0 || N < 0 || ns_out < 1) return -1;
  const int64_t E = static_cast<int64_t>(B) * Q * ns_out;
  if (E == 0 || N == 0) return 0;
  const int64_t seg = dvcp::segment_sum_workspace_bytes(E, static_cast<int64_t>(B) * N);
  if (seg < 0) return -1;
  return dvcp::fb_align(E * 4) + seg;
}

extern "C" int dvcp_group_rows_backward(const int32_t* count, const int32_t* list, int ns_list, int ns_out, int Q,
                                        int N, int D, int B, const float* grad_rows, float* grad_feat,
                                        void* workspace, int64_t ws_bytes, void* stream) {
  DVCP_REQUIRE(D == 32, "dvcp_group_rows_backward: D=%d (32 feature columns only)", D);
  DVCP_REQUIRE(Q >= 0 && B >= 0 && N >= 0 && ns_list >= 1 && ns_out >= 1,
               "dvcp_group_rows_backward: bad sizes Q=%d B=%d N=%d ns=%d/%d", Q, B, N, ns_list, ns_out);
  const int64_t E = static_cast<int64_t>(B) * Q * ns_out, nrows = static_cast<int64_t>(B) * N;
  DVCP_REQUIRE(E <= 0x7FFFFFFF && nrows <= 0x7FFFFFFF,
               "dvcp_group_rows_backward: B Q ns and B N must stay below 2^31");
  if (nrows == 0) return DVCP_OK;
  DVCP_REQUIRE(grad_feat, "dvcp_group_rows_backward: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (E == 0) {  // no centre: nothing routed
    if (hipMemsetAsync(grad_feat, 0, static_cast<size_t>(nrows) * D * 4, st) != hipSuccess)
      return dvcp::launch_status("dvcp_group_rows_backward(empty)");
    return DVCP_OK;
  }
  DVCP_REQUIRE(count && list && grad_rows && workspace, "dvcp_group_rows_backward: null pointer");
  const int64_t need = dvcp_group_rows_backward_workspace_bytes(B, Q, N, ns_out);
  DVCP_REQUIRE(need >= 0, "dvcp_group_rows_backward: workspace size query failed");
  DVCP_REQUIRE(ws_bytes >= need, "dvcp_group_rows_backward: workspace of %lld bytes is short of %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(need));
  char* w = static_cast<char*>(workspace);
  uint32_t* keys = reinterpret_cast<uint32_t*>(w);
  w += dvcp::fb_align(E * 4);
  hipLaunchKernelGGL(dvcp::group_rows_keys_kernel, dim3(dvcp::ceil_div(E, 256)), dim3(256), 0, st, count, list, ns_list,
                     ns_out, Q, N, E, static_cast<uint32_t>(nrows), keys);
  if (int e = dvcp::launch_status("dvcp_group_rows_backward")) return e;
  return dvcp::segment_sum_strided(keys, grad_rows, 3 + D, 3, E, nrows, D, grad_feat, w, st);
}
