// cpg_tiled_bwd.hip -- backward of corresponding point generation (cpg.py:27-60) for candidate
// grids of any side 1 <= G <= 32: the training counterpart of cpg_tiled.hip.
//
// The mathematics is cpg_bwd.hip's (see its header): softmax / weighted-mean backward, the three
// convolutions' data and weight gradients with zero padding, and the cost volume's derivative under
// the Q11 scramble.  cpg_bwd.hip keeps a key point's whole grid in LDS (G <= 11); here the grid is
// cut into blocks of at most 8^3 cells (per axis nb = ceil(G / 8) blocks of ceil(G / nb) cells) and
// every stage goes through an HBM workspace, so a kernel needs its input on the block plus ONE cell
// only: the gradient of the stage before is complete in the workspace, halo cells included.
// Per chunk of key points (74 C floats each, plus the blocks' partial sums):
//   0-2. the forward's own launches (ct_forward_chunk): target in Q11 order, h1, logits.
//   3. softmax over the key point's C logits (global maximum subtracted), A = sum w cand, S = sum w,
//      sum_u w_u dL/dw_u, then dL/dlg for every cell and db3.  One workgroup per key point.
//   4. h2 = conv2(h1) per block (the forward fuses conv2 and conv3 and never writes h2): 4 C floats.
//   5. conv3 backward: dL/dh2 on the block, the block's part of dW3.
//   6. conv2 backward: dL/dh1 on the block, the block's part of dW2 and db2.
//   7. conv1 data backward and the cost's derivative: dL/dtgt written in place (Q11: element
//      l = 32 g + f' of the (32, C) view is the contiguous gradient's flat offset), the block's part
//      of dL/dsrc.
//   8. conv1 weight backward: the block's part of dW1 and db1, the cost rebuilt 8 channels at a time.
//   9. the blocks' parts summed in block order: parameter partials per key point (outside the
//      chunk's region, all P of them) and dL/dsrc.
// and after the last chunk the partials are summed over the key points in fp64, in key-point order
// (fold_rows, as the single-tile backward).  No atomics: every sum has a fixed order, which does not depend on
// how the key points were chunked.
//
// A cell outside the grid is 0 in every LDS image: for an activation (cost, h1, h2) that is the
// convolution's zero padding, for a gradient it drops the taps that leave the grid.  A halo cell
// inside the grid is the neighbour block's real value, read from the workspace.
// Arithmetic: plain fp32 FMA everywhere, conv1's two backward products included (weights
// transposed into LDS and read as wave-uniform broadcasts); no matrix-core instructions.
#include "cpg_tiled.h"

namespace dvcp {

constexpr int kTbE = 8;                  // block edge
constexpr int kTbN = kTbE * kTbE * kTbE;  // cells of a block
constexpr int kTbPV = 10 * 10 * 10;      // cells of a block with its one-cell halo
// packed parameter layout (= cpg.packed_params()): W1, b1, W2, b2, W3, b3
constexpr int kTbOffB1 = 16 * 32 * 27;
constexpr int kTbOffW2 = kTbOffB1 + 16;
constexpr int kTbOffB2 = kTbOffW2 + 4 * 16 * 27;
constexpr int kTbOffW3 = kTbOffB2 + 4;
constexpr int kTbOffB3 = kTbOffW3 + 4 * 27;
constexpr int kTbParams = kTbOffB3 + 1;
constexpr int kTbPart = kTbParams + 32;  // a block's partial sums: the parameters, then dL/dsrc

inline int tb_nblk(int G) {
  const int nb = ct_blocks(G, kTbE);
  return nb * nb * nb;
}
// floats of the chunk region per key point (a multiple of 4: every array starts 16-byte aligned)
inline int64_t tb_ws_per_point(int G) {
  const int64_t C = int64_t(G) * G * G;
  return (74 * C + int64_t(tb_nblk(G)) * kTbPart + 1 + 3) / 4 * 4;
}
inline int64_t tb_ws_partials(int P) { return (int64_t(P) * kTbParams + 3) / 4 * 4; }

// A block with its one-cell halo: sizes, divisions, and the grid cell of a haloed cell
struct TbGeo {
  CtBlock B;
  int G, PX, PXY, PV, n;
  FastDiv dPX, dPXY, dBX, dBXY;
  __device__ __forceinline__ TbGeo(int blk, int G_, int nb, int bs, const CtMagic& k)
      : B(blk, G_, nb, bs),
        G(G_),
        PX(B.bx + 2),
        PXY(PX * (B.by + 2)),
        PV(PXY * (B.bz + 2)),
        n(B.bx * B.by * B.bz),
        dPX(B.row(k, 1)),
        dPXY(B.plane(k, 1)),
        dBX(B.row(k, 0)),
        dBXY(B.plane(k, 0)) {}
  // grid cell of haloed cell h < PV, or -1 outside the grid
  __device__ __forceinline__ int halo_cell(int h) const {
    const uint32_t hz = dPXY.div(h), r = h - hz * dPXY.d, hy = dPX.div(r), hx = r - hy * dPX.d;
    const int gx = B.ox + static_cast<int>(hx) - 1, gy = B.oy + static_cast<int>(hy) - 1,
              gz = B.oz + static_cast<int>(hz) - 1;
    const bool in = gx >= 0 && gx < G && gy >= 0 && gy < G && gz >= 0 && gz < G;
    return in ? (gz * G + gy) * G + gx : -1;
  }
  // block cell v < n: its haloed address and its grid cell
  __device__ __forceinline__ void cell(int v, int& hc, int& g) const {
    const uint32_t z = dBXY.div(v), r = v - z * dBXY.d, y = dBX.div(r), x = r - y * dBX.d;
    hc = static_cast<int>((z + 1) * PXY + (y + 1) * PX + (x + 1));
    g = ((B.oz + static_cast<int>(z)) * G + B.oy + static_cast<int>(y)) * G + B.ox + static_cast<int>(x);
  }
  __device__ __forceinline__ int tap(int t) const { return (t / 9 - 1) * PXY + ((t / 3) % 3 - 1) * PX + (t % 3 - 1); }
  // haloed address of block cell (z, y, x)
  __device__ __forceinline__ int at(int z, int y, int x) const { return (z + 1) * PXY + (y + 1) * PX + (x + 1); }
};

// Launch 3: dL/dlg of every cell of a key point, and db3 = its sum
__global__ __launch_bounds__(kCtThreads) void cpg_tb_softmax_kernel(const float* __restrict__ logit,
                                                                    const float* __restrict__ cand,
                                                                    const float* __restrict__ gvcp, int C,
                                                                    float* __restrict__ dlg, float* __restrict__ db3) {
  __shared__ float red[32];
  const int p = blockIdx.x, tid = threadIdx.x;
  const float* lg = logit + static_cast<int64_t>(p) * C;
  const float* cq = cand + static_cast<int64_t>(p) * C * 3;
  float lmax = -__builtin_huge_valf();
  for (int g = tid; g < C; g += kCtThreads) lmax = fmaxf(lmax, lg[g]);
  const float m = block_max_f(lmax, red);
  float se = 0.f;
  for (int g = tid; g < C; g += kCtThreads) se += expf(lg[g] - m);
  const float inv = 1.0f / block_sum(se, red);
  float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
  for (int g = tid; g < C; g += kCtThreads) {
    const float w = expf(lg[g] - m) * inv;
    sw += w;
    sx += w * cq[g * 3 + 0];
    sy += w * cq[g * 3 + 1];
    sz += w * cq[g * 3 + 2];
  }
  sw = block_sum(sw, red);
  sx = block_sum(sx, red);
  sy = block_sum(sy, red);
  sz = block_sum(sz, red);
  const float g0 = gvcp[static_cast<int64_t>(p) * 3 + 0], g1 = gvcp[static_cast<int64_t>(p) * 3 + 1],
              g2 = gvcp[static_cast<int64_t>(p) * 3 + 2];
  const float gS = -(g0 * sx + g1 * sy + g2 * sz) / (sw * sw);
  float dot = 0.f;
  for (int g = tid; g < C; g += kCtThreads) {
    const float w = expf(lg[g] - m) * inv;
    const float gw = (g0 * cq[g * 3 + 0] + g1 * cq[g * 3 + 1] + g2 * cq[g * 3 + 2]) / sw + gS;
    dot += w * gw;
  }
  dot = block_sum(dot, red);
  float gls = 0.f;
  for (int g = tid; g < C; g += kCtThreads) {
    const float w = expf(lg[g] - m) * inv;
    const float gw = (g0 * cq[g * 3 + 0] + g1 * cq[g * 3 + 1] + g2 * cq[g * 3 + 2]) / sw + gS;
    const float v = w * (gw - dot);
    dlg[static_cast<int64_t>(p) * C + g] = v;
    gls += v;
  }
  gls = block_sum(gls, red);
  if (tid == 0) db3[p] = gls;
}

// Launch 4: h2 = conv2(h1) on one block of one key point -> h2 (chunk x C x 4, bias added)
__global__ __launch_bounds__(kCtThreads) void cpg_tb_h2_kernel(const float* __restrict__ h1, int G, int nb, int bs,
                                                               CtMagic magic, const float* __restrict__ params,
                                                               float* __restrict__ h2) {
  __shared__ __attribute__((aligned(16))) float h1s[16 * kTbPV];     // [ci][haloed cell]
  __shared__ __attribute__((aligned(16))) float w2a[16 * 27 * 4];    // [ci][t][co]
  const int p = blockIdx.y, tid = threadIdx.x;
  const int C = G * G * G;
  const TbGeo T(blockIdx.x, G, nb, bs, magic);
  const float* P2 = params + kTbOffW2;
  for (int i = tid; i < 4 * 16 * 27; i += kCtThreads) {
    const int co = i / 432, r = i - co * 432;  // r = ci 27 + t
    w2a[r * 4 + co] = P2[i];
  }
  const float4* in = reinterpret_cast<const float4*>(h1 + static_cast<int64_t>(p) * C * 16);
  for (int h = tid; h < T.PV; h += kCtThreads) {
    const int g = T.halo_cell(h);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 v = g >= 0 ? in[static_cast<int64_t>(g) * 4 + k] : make_float4(0.f, 0.f, 0.f, 0.f);
      h1s[(4 * k + 0) * T.PV + h] = v.x;
      h1s[(4 * k + 1) * T.PV + h] = v.y;
      h1s[(4 * k + 2) * T.PV + h] = v.z;
      h1s[(4 * k + 3) * T.PV + h] = v.w;
    }
  }
  __syncthreads();
  if (tid < T.n) {
    int hc, g;
    T.cell(tid, hc, g);
    float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int ci = 0; ci < 16; ++ci)
#pragma unroll
      for (int t = 0; t < 27; ++t) {
        const float x = h1s[ci * T.PV + hc + T.tap(t)];
        const float4 w = *reinterpret_cast<const float4*>(&w2a[(ci * 27 + t) * 4]);
        a[0] = __fmaf_rn(w.x, x, a[0]);
        a[1] = __fmaf_rn(w.y, x, a[1]);
        a[2] = __fmaf_rn(w.z, x, a[2]);
        a[3] = __fmaf_rn(w.w, x, a[3]);
      }
    const float* b2 = params + kTbOffB2;
    reinterpret_cast<float4*>(h2 + static_cast<int64_t>(p) * C * 4)[g] =
        make_float4(a[0] + b2[0], a[1] + b2[1], a[2] + b2[2], a[3] + b2[3]);
  }
}

// Launch 5: conv3 backward on one block: dL/dh2 (chunk x C x 4) and the block's part of dW3
__global__ __launch_bounds__(kCtThreads) void cpg_tb_conv3_kernel(const float* __restrict__ dlg,
                                                                  const float* __restrict__ h2, int G, int nb, int bs,
                                                                  CtMagic magic, const float* __restrict__ params,
                                                                  float* __restrict__ dh2, float* __restrict__ gpb) {
  __shared__ float gls[kTbPV];       // dL/dlg, haloed
  __shared__ float h2s[4 * kTbPV];   // [ci][haloed cell]
  __shared__ float w3[4 * 27];
  __shared__ float scr[108 * kTbE];
  const int p = blockIdx.y, tid = threadIdx.x;
  const int C = G * G * G;
  const TbGeo T(blockIdx.x, G, nb, bs, magic);
  if (tid < 108) w3[tid] = params[kTbOffW3 + tid];
  const float4* in = reinterpret_cast<const float4*>(h2 + static_cast<int64_t>(p) * C * 4);
  for (int h = tid; h < T.PV; h += kCtThreads) {
    const int g = T.halo_cell(h);
    const float4 v = g >= 0 ? in[g] : make_float4(0.f, 0.f, 0.f, 0.f);
    gls[h] = g >= 0 ? dlg[static_cast<int64_t>(p) * C + g] : 0.f;
    h2s[0 * T.PV + h] = v.x;
    h2s[1 * T.PV + h] = v.y;
    h2s[2 * T.PV + h] = v.z;
    h2s[3 * T.PV + h] = v.w;
  }
  __syncthreads();
  if (tid < T.n) {
    int hc, g;
    T.cell(tid, hc, g);
    float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 27; ++t) {
      const float x = gls[hc - T.tap(t)];
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) a[ci] = __fmaf_rn(w3[ci * 27 + t], x, a[ci]);
    }
    reinterpret_cast<float4*>(dh2 + static_cast<int64_t>(p) * C * 4)[g] = make_float4(a[0], a[1], a[2], a[3]);
  }
  // dW3[ci][t] = sum over the block's cells v of dL/dlg[v] h2[ci][v + off_t]: one z plane per thread
  if (tid < 108 * kTbE) {
    const int o = tid % 108, z = tid / 108, ci = o / 27, t = o - ci * 27;
    const float* hin = h2s + ci * T.PV + T.tap(t);
    float s = 0.f;
    if (z < T.B.bz)
      for (int y = 0; y < T.B.by; ++y)
        for (int x = 0; x < T.B.bx; ++x) {
          const int hc = T.at(z, y, x);
          s = __fmaf_rn(gls[hc], hin[hc], s);
        }
    scr[tid] = s;
  }
  __syncthreads();
  if (tid < 108) {
    float s = 0.f;
    for (int z = 0; z < kTbE; ++z) s += scr[z * 108 + tid];
    gpb[(static_cast<int64_t>(p) * gridDim.x + blockIdx.x) * kTbPart + kTbOffW3 + tid] = s;
  }
}

// Launch 6: conv2 backward on one block: dL/dh1 (chunk x C x 16) and the block's part of dW2, db2
__global__ __launch_bounds__(kCtThreads) void cpg_tb_conv2_kernel(const float* __restrict__ dh2,
                                                                  const float* __restrict__ h1, int G, int nb, int bs,
                                                                  CtMagic magic, const float* __restrict__ params,
                                                                  float* __restrict__ dh1, float* __restrict__ gpb) {
  __shared__ __attribute__((aligned(16))) float g2s[4 * kTbPV];    // dL/dh2 [co][haloed cell]
  __shared__ __attribute__((aligned(16))) float h1s[16 * kTbPV];   // [ci][haloed cell]
  __shared__ __attribute__((aligned(16))) float w2b[4 * 27 * 16];  // [co][t][ci]
  __shared__ float scr[864 * 4];
  __shared__ float red[4 * kTbE];
  const int p = blockIdx.y, tid = threadIdx.x;
  const int C = G * G * G;
  const TbGeo T(blockIdx.x, G, nb, bs, magic);
  const float* P2 = params + kTbOffW2;
  for (int i = tid; i < 4 * 16 * 27; i += kCtThreads) {
    const int co = i / 432, r = i - co * 432, ci = r / 27, t = r - ci * 27;
    w2b[(co * 27 + t) * 16 + ci] = P2[i];
  }
  const float4* in1 = reinterpret_cast<const float4*>(h1 + static_cast<int64_t>(p) * C * 16);
  const float4* in2 = reinterpret_cast<const float4*>(dh2 + static_cast<int64_t>(p) * C * 4);
  for (int h = tid; h < T.PV; h += kCtThreads) {
    const int g = T.halo_cell(h);
    const float4 d = g >= 0 ? in2[g] : make_float4(0.f, 0.f, 0.f, 0.f);
    g2s[0 * T.PV + h] = d.x;
    g2s[1 * T.PV + h] = d.y;
    g2s[2 * T.PV + h] = d.z;
    g2s[3 * T.PV + h] = d.w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 v = g >= 0 ? in1[static_cast<int64_t>(g) * 4 + k] : make_float4(0.f, 0.f, 0.f, 0.f);
      h1s[(4 * k + 0) * T.PV + h] = v.x;
      h1s[(4 * k + 1) * T.PV + h] = v.y;
      h1s[(4 * k + 2) * T.PV + h] = v.z;
      h1s[(4 * k + 3) * T.PV + h] = v.w;
    }
  }
  __syncthreads();
  // dL/dh1[ci][u] = sum_co sum_t W2[co][ci][t] dL/dh2[co][u - off_t]: a cell's 16 channels on two
  // threads, 8 each (the half is wave-uniform: the weights are LDS broadcasts)
  {
    const int v = tid & (kTbN - 1), half = tid >> 9;
    if (v < T.n) {
      int hc, g;
      T.cell(v, hc, g);
      float a[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) a[k] = 0.f;
#pragma unroll 1
      for (int co = 0; co < 4; ++co)
#pragma unroll 3
        for (int t = 0; t < 27; ++t) {
          const float x = g2s[co * T.PV + hc - T.tap(t)];
          const float4 wa = *reinterpret_cast<const float4*>(&w2b[(co * 27 + t) * 16 + 8 * half]);
          const float4 wb = *reinterpret_cast<const float4*>(&w2b[(co * 27 + t) * 16 + 8 * half + 4]);
          a[0] = __fmaf_rn(wa.x, x, a[0]);
          a[1] = __fmaf_rn(wa.y, x, a[1]);
          a[2] = __fmaf_rn(wa.z, x, a[2]);
          a[3] = __fmaf_rn(wa.w, x, a[3]);
          a[4] = __fmaf_rn(wb.x, x, a[4]);
          a[5] = __fmaf_rn(wb.y, x, a[5]);
          a[6] = __fmaf_rn(wb.z, x, a[6]);
          a[7] = __fmaf_rn(wb.w, x, a[7]);
        }
      float4* out = reinterpret_cast<float4*>(dh1 + static_cast<int64_t>(p) * C * 16) + static_cast<int64_t>(g) * 4;
      out[2 * half + 0] = make_float4(a[0], a[1], a[2], a[3]);
      out[2 * half + 1] = make_float4(a[4], a[5], a[6], a[7]);
    }
  }
  // dW2[co][ci][t] = sum over the block's cells v of dL/dh2[co][v] h1[ci][v + off_t]: thread
  // (ci, t) with the four co, the z planes in two halves summed in order
  if (tid < 864) {
    const int o = tid % 432, sl = tid / 432, ci = o / 27, t = o - ci * 27;
    const float* hin = h1s + ci * T.PV + T.tap(t);
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int z = (sl * T.B.bz) / 2; z < ((sl + 1) * T.B.bz) / 2; ++z)
      for (int y = 0; y < T.B.by; ++y)
        for (int x = 0; x < T.B.bx; ++x) {
          const int hc = T.at(z, y, x);
          const float xin = hin[hc];
#pragma unroll
          for (int co = 0; co < 4; ++co) a[co] = __fmaf_rn(g2s[co * T.PV + hc], xin, a[co]);
        }
#pragma unroll
    for (int co = 0; co < 4; ++co) scr[tid * 4 + co] = a[co];
  } else if (tid < 864 + 4 * kTbE) {  // db2[co]: one z plane per thread
    const int k = tid - 864, co = k & 3, z = k >> 2;
    float s = 0.f;
    if (z < T.B.bz)
      for (int y = 0; y < T.B.by; ++y)
        for (int x = 0; x < T.B.bx; ++x) s += g2s[co * T.PV + T.at(z, y, x)];
    red[k] = s;
  }
  __syncthreads();
  float* gp = gpb + (static_cast<int64_t>(p) * gridDim.x + blockIdx.x) * kTbPart;
  if (tid < 432) {
#pragma unroll
    for (int co = 0; co < 4; ++co) gp[kTbOffW2 + co * 432 + tid] = scr[tid * 4 + co] + scr[(tid + 432) * 4 + co];
  } else if (tid < 432 + 4) {
    const int co = tid - 432;
    float s = 0.f;
    for (int z = 0; z < kTbE; ++z) s += red[z * 4 + co];
    gp[kTbOffB2 + co] = s;
  }
}

// Launch 7: conv1 data backward on one block and the cost's derivative: dL/dtgt in place, the
// block's part of dL/dsrc.  tl: the target blocks in Q11 order, tl_p floats apart.
constexpr int kTbR = kTbN * 33 > 16 * kTbPV ? kTbN * 33 : 16 * kTbPV;
__global__ __launch_bounds__(kCtThreads) void cpg_tb_conv1d_kernel(const float* __restrict__ src,
                                                                   const float* __restrict__ tl, int64_t tl_p,
                                                                   const float* __restrict__ dh1, int G, int nb,
                                                                   int bs, CtMagic magic,
                                                                   const float* __restrict__ params,
                                                                   float* __restrict__ gtgt, float* __restrict__ gpb) {
  __shared__ __attribute__((aligned(16))) float w1b[16 * 27 * 32];  // [co][t][ci]
  __shared__ __attribute__((aligned(16))) float R[kTbR];  // dL/dh1 [co][haloed cell], later dL/dcost [cell][33]
  __shared__ float sv[32];
  __shared__ float red[32 * kTbE];
  const int p = blockIdx.y, tid = threadIdx.x;
  const int C = G * G * G;
  const TbGeo T(blockIdx.x, G, nb, bs, magic);
  if (tid < 32) sv[tid] = src[static_cast<int64_t>(p) * 32 + tid];
  for (int i = tid; i < 16 * 32 * 27; i += kCtThreads) {
    const int co = i / 864, r = i - co * 864, ci = r / 27, t = r - ci * 27;
    w1b[(co * 27 + t) * 32 + ci] = params[i];
  }
  const float4* in = reinterpret_cast<const float4*>(dh1 + static_cast<int64_t>(p) * C * 16);
  for (int h = tid; h < T.PV; h += kCtThreads) {
    const int g = T.halo_cell(h);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 v = g >= 0 ? in[static_cast<int64_t>(g) * 4 + k] : make_float4(0.f, 0.f, 0.f, 0.f);
      R[(4 * k + 0) * T.PV + h] = v.x;
      R[(4 * k + 1) * T.PV + h] = v.y;
      R[(4 * k + 2) * T.PV + h] = v.z;
      R[(4 * k + 3) * T.PV + h] = v.w;
    }
  }
  __syncthreads();
  // dL/dcost[ci][u] = sum_co sum_t W1[co][ci][t] dL/dh1[co][u - off_t]: a cell's 32 channels on two
  // threads, 16 each
  const int v = tid & (kTbN - 1), half = tid >> 9;
  float a[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) a[k] = 0.f;
  if (v < T.n) {
    int hc, g;
    T.cell(v, hc, g);
#pragma unroll 1
    for (int co = 0; co < 16; ++co)
#pragma unroll 3
      for (int t = 0; t < 27; ++t) {
        const float x = R[co * T.PV + hc - T.tap(t)];
        const float4* w = reinterpret_cast<const float4*>(&w1b[(co * 27 + t) * 32 + 16 * half]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float4 wk = w[k];
          a[4 * k + 0] = __fmaf_rn(wk.x, x, a[4 * k + 0]);
          a[4 * k + 1] = __fmaf_rn(wk.y, x, a[4 * k + 1]);
          a[4 * k + 2] = __fmaf_rn(wk.z, x, a[4 * k + 2]);
          a[4 * k + 3] = __fmaf_rn(wk.w, x, a[4 * k + 3]);
        }
      }
  }
  __syncthreads();  // every dL/dh1 value read; dL/dcost overwrites them
  if (v < T.n)
#pragma unroll
    for (int k = 0; k < 16; ++k) R[v * 33 + 16 * half + k] = a[k];
  __syncthreads();
  // the cost's derivative, walking l = 32 g + f' (consecutive addresses of the target and of its
  // gradient): dL/dT[l] = -2 (src[f'] - T[l]) dL/dcost, dL/dsrc[f'] = sum_g 2 (src[f'] - T[l]) dL/dcost
  const float* Tq = tl + static_cast<int64_t>(p) * tl_p;
  float* gT = gtgt + static_cast<int64_t>(p) * 32 * C;
  for (int i = tid; i < 32 * T.n; i += kCtThreads) {
    const int c = i >> 5, f = i & 31;
    int hc, g;
    T.cell(c, hc, g);
    const int l = 32 * g + f;
    const float d = sv[f] - Tq[l];
    const float gd = 2.0f * d * R[c * 33 + f];
    gT[l] = -gd;
    R[c * 33 + f] = gd;
  }
  __syncthreads();
  if (tid < 32 * kTbE) {
    const int f = tid & 31, z = tid >> 5, pl = T.B.bx * T.B.by;
    float s = 0.f;
    if (z < T.B.bz)
      for (int c = z * pl; c < (z + 1) * pl; ++c) s += R[c * 33 + f];
    red[tid] = s;
  }
  __syncthreads();
  if (tid < 32) {
    float s = 0.f;
    for (int z = 0; z < kTbE; ++z) s += red[z * 32 + tid];
    gpb[(static_cast<int64_t>(p) * gridDim.x + blockIdx.x) * kTbPart + kTbParams + tid] = s;
  }
}

// Launch 8: conv1 weight backward on one block: dW1[co][ci][t] = sum over the block's cells v of
// dL/dh1[co][v] cost[ci][v + off_t], and db1.  The cost is rebuilt 8 channels at a time on the block
// plus one cell; thread (channel, tap) holds the 16 co, the z planes in four groups summed in order.
__global__ __launch_bounds__(kCtThreads) void cpg_tb_conv1w_kernel(const float* __restrict__ src,
                                                                   const float* __restrict__ tl, int64_t tl_p,
                                                                   const float* __restrict__ dh1, int G, int nb,
                                                                   int bs, CtMagic magic, float* __restrict__ gpb) {
  __shared__ __attribute__((aligned(16))) float g1s[kTbN * 16];  // dL/dh1 [cell][co]
  __shared__ __attribute__((aligned(16))) float cs[8 * kTbPV];   // cost [channel of the pass][haloed cell]
  __shared__ __attribute__((aligned(16))) float scr[864 * 16];
  __shared__ float sv[32];
  __shared__ float red[16 * kTbE];
  const int p = blockIdx.y, tid = threadIdx.x;
  const int C = G * G * G;
  const TbGeo T(blockIdx.x, G, nb, bs, magic);
  float* gp = gpb + (static_cast<int64_t>(p) * gridDim.x + blockIdx.x) * kTbPart;
  if (tid < 32) sv[tid] = src[static_cast<int64_t>(p) * 32 + tid];
  const float4* in = reinterpret_cast<const float4*>(dh1 + static_cast<int64_t>(p) * C * 16);
  for (int i = tid; i < 4 * T.n; i += kCtThreads) {
    const int c = i >> 2, k = i & 3;
    int hc, g;
    T.cell(c, hc, g);
    reinterpret_cast<float4*>(g1s)[c * 4 + k] = in[static_cast<int64_t>(g) * 4 + k];
  }
  __syncthreads();
  if (tid < 16 * kTbE) {  // db1[co]: one z plane per thread
    const int co = tid & 15, z = tid >> 4, pl = T.B.bx * T.B.by;
    float s = 0.f;
    if (z < T.B.bz)
      for (int c = z * pl; c < (z + 1) * pl; ++c) s += g1s[c * 16 + co];
    red[tid] = s;
  }
  __syncthreads();
  if (tid < 16) {
    float s = 0.f;
    for (int z = 0; z < kTbE; ++z) s += red[z * 16 + tid];
    gp[kTbOffB1 + tid] = s;
  }
  const float* Tq = tl + static_cast<int64_t>(p) * tl_p;
  const int pair = tid % 216, sl = tid / 216, c8 = pair / 27, t = pair - c8 * 27;
#pragma unroll 1
  for (int q = 0; q < 4; ++q) {
    __syncthreads();  // the previous pass has read cs and scr
    for (int i = tid; i < 8 * T.PV; i += kCtThreads) {
      const int h = i >> 3, j = i & 7;
      const int g = T.halo_cell(h);
      float cost = 0.f;
      if (g >= 0) {
        const float d = sv[8 * q + j] - Tq[32 * g + 8 * q + j];  // Q11
        cost = d * d;
      }
      cs[j * T.PV + h] = cost;
    }
    __syncthreads();
    if (tid < 864) {
      const float* cin = cs + c8 * T.PV + T.tap(t);
      float a[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) a[k] = 0.f;
      for (int z = (sl * T.B.bz) / 4; z < ((sl + 1) * T.B.bz) / 4; ++z)
        for (int y = 0; y < T.B.by; ++y)
          for (int x = 0; x < T.B.bx; ++x) {
            const float c = cin[T.at(z, y, x)];
            const float4* gv = reinterpret_cast<const float4*>(&g1s[((z * T.B.by + y) * T.B.bx + x) * 16]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const float4 gk = gv[k];
              a[4 * k + 0] = __fmaf_rn(gk.x, c, a[4 * k + 0]);
              a[4 * k + 1] = __fmaf_rn(gk.y, c, a[4 * k + 1]);
              a[4 * k + 2] = __fmaf_rn(gk.z, c, a[4 * k + 2]);
              a[4 * k + 3] = __fmaf_rn(gk.w, c, a[4 * k + 3]);
            }
          }
#pragma unroll
      for (int k = 0; k < 16; ++k) scr[tid * 16 + k] = a[k];
    }
    __syncthreads();
    for (int o = tid; o < 216 * 16; o += kCtThreads) {
      const int pr = o >> 4, co = o & 15, ci = 8 * q + pr / 27, tt = pr % 27;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) s += scr[(k * 216 + pr) * 16 + co];
      gp[(co * 32 + ci) * 27 + tt] = s;
    }
  }
}

// Launch 9: the blocks' parts of a key point summed in block order -> the key point's parameter
// partials (db3 comes from launch 3) and dL/dsrc
__global__ void cpg_tb_blocks_kernel(const float* __restrict__ gpb, const float* __restrict__ db3, int nblk,
                                     float* __restrict__ part, float* __restrict__ gsrc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, p = blockIdx.y;
  if (i >= kTbPart) return;
  float s = 0.f;
  if (i == kTbOffB3) {
    s = db3[p];
  } else {
    const float* in = gpb + static_cast<int64_t>(p) * nblk * kTbPart + i;
    for (int b = 0; b < nblk; ++b) s += in[static_cast<int64_t>(b) * kTbPart];
  }
  if (i < kTbParams)
    part[static_cast<int64_t>(p) * kTbParams + i] = s;
  else
    gsrc[static_cast<int64_t>(p) * 32 + i - kTbParams] = s;
}

}  // namespace dvcp

extern "C" int64_t dvcp_cpg_tiled_backward_workspace_bytes(int P, int G) {
  if (P <= 0 || G < 1 || G > dvcp::kCtMaxG) return 0;
  const int64_t per = dvcp::tb_ws_per_point(G) * 4;
  const int64_t chunk = dvcp::kCtWsCap / per;  // >= 19
  return dvcp::tb_ws_partials(P) * 4 + (P < chunk ? P : chunk) * per;
}

extern "C" int dvcp_cpg_tiled_backward(const float* src, const float* tgt, int64_t t_p, int64_t t_f, int64_t t_c,
                                       const float* cand, int P, int G, const float* params, const float* grad_vcp,
                                       float* grad_src, float* grad_tgt, float* ws, int64_t ws_bytes,
                                       float* grad_params, void* stream) {
  DVCP_REQUIRE(G >= 1 && G <= dvcp::kCtMaxG,
               "dvcp_cpg_tiled_backward: grid side G=%d unsupported (1 <= G <= 32, C <= 32768)", G);
  DVCP_REQUIRE(params && grad_params, "dvcp_cpg_tiled_backward: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (P <= 0) {
    dvcp::fold_rows(ws, 0, dvcp::kTbParams, dvcp::kTbParams, grad_params, s);
    return dvcp::launch_status("dvcp_cpg_tiled_backward");
  }
  DVCP_REQUIRE(src && tgt && cand && grad_vcp && grad_src && grad_tgt && ws, "dvcp_cpg_tiled_backward: null pointer");
  DVCP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0,
               "dvcp_cpg_tiled_backward: workspace must be 16-byte aligned");
  const int64_t per = dvcp::tb_ws_per_point(G), npart = dvcp::tb_ws_partials(P);
  DVCP_REQUIRE(ws_bytes >= (npart + per) * 4,
               "dvcp_cpg_tiled_backward: workspace of %lld bytes holds no key point (%lld for the partial sums, %lld "
               "each)",
               static_cast<long long>(ws_bytes), static_cast<long long>(npart * 4), static_cast<long long>(per * 4));
  const int64_t C = int64_t(G) * G * G;
  int64_t chunk = (ws_bytes / 4 - npart) / per;
  if (chunk > P) chunk = P;
  if (chunk > 32768) chunk = 32768;  // grid.y
  const int nb = dvcp::ct_blocks(G, dvcp::kTbE), bs = dvcp::ct_block_size(G, nb), nblk = nb * nb * nb;
  const dvcp::CtMagic magic = dvcp::ct_magic(G, nb, bs);
  // the partials of all P key points, then the chunk's arrays (the float4 ones first)
  float* part = ws;
  float* h1 = ws + npart;
  float* h2 = h1 + chunk * C * 16;
  float* dh2 = h2 + chunk * C * 4;
  float* dh1 = dh2 + chunk * C * 4;
  float* order = dh1 + chunk * C * 16;
  float* logit = order + chunk * C * 32;
  float* dlg = logit + chunk * C;
  float* gpb = dlg + chunk * C;
  float* db3 = gpb + chunk * nblk * dvcp::kTbPart;
  const dim3 wg(dvcp::kCtThreads);
  for (int64_t p0 = 0; p0 < P; p0 += chunk) {
    const int np = static_cast<int>(P - p0 < chunk ? P - p0 : chunk);
    const dim3 gb(nblk, np);
    const float* sp = src + p0 * 32;
    int64_t tl_p;
    const float* tl = dvcp::ct_forward_chunk(sp, tgt + p0 * t_p, t_p, t_f, t_c, cand + p0 * C * 3, np, G, params, h1,
                                             logit, order, nullptr, nullptr, &tl_p, s);
    hipLaunchKernelGGL(dvcp::cpg_tb_softmax_kernel, dim3(np), wg, 0, s, logit, cand + p0 * C * 3, grad_vcp + p0 * 3,
                       static_cast<int>(C), dlg, db3);
    hipLaunchKernelGGL(dvcp::cpg_tb_h2_kernel, gb, wg, 0, s, h1, G, nb, bs, magic, params, h2);
    hipLaunchKernelGGL(dvcp::cpg_tb_conv3_kernel, gb, wg, 0, s, dlg, h2, G, nb, bs, magic, params, dh2, gpb);
    hipLaunchKernelGGL(dvcp::cpg_tb_conv2_kernel, gb, wg, 0, s, dh2, h1, G, nb, bs, magic, params, dh1, gpb);
    hipLaunchKernelGGL(dvcp::cpg_tb_conv1d_kernel, gb, wg, 0, s, sp, tl, tl_p, dh1, G, nb, bs, magic, params,
                       grad_tgt + p0 * 32 * C, gpb);
    hipLaunchKernelGGL(dvcp::cpg_tb_conv1w_kernel, gb, wg, 0, s, sp, tl, tl_p, dh1, G, nb, bs, magic, gpb);
    hipLaunchKernelGGL(dvcp::cpg_tb_blocks_kernel, dim3(dvcp::ceil_div(dvcp::kTbPart, 256), np), dim3(256), 0, s, gpb,
                       db3, nblk, part + p0 * dvcp::kTbParams, grad_src + p0 * 32);
  }
  dvcp::fold_rows(part, P, dvcp::kTbParams, dvcp::kTbParams, grad_params, s);
  return dvcp::launch_status("dvcp_cpg_tiled_backward");
}
