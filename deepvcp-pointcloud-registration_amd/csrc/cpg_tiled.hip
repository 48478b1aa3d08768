// cpg_tiled.hip -- corresponding point generation (cpg.py:27-60) for candidate grids above the
// one-workgroup kernel's 11^3 (cpg.hip): 1 <= G <= 32.  Backward: cpg_tiled_bwd.hip, which repeats
// launches 0-2 through ct_forward_chunk (cpg_tiled.h).
//
// The grid is cut into blocks and the three convolutions are staged through an HBM workspace
// (49 C floats per key point: conv1's output h1, cell-major [g][16], the C logits, and the target
// block in Q11 order), up to four launches per chunk of key points:
//   0. the key points' (32, C) target blocks copied into Q11 order, element l = f C + c (a tiled
//      transpose of the forward's permuted (C, 32) rows; skipped when the tensor already is in that
//      order, t_f = C and t_c = 1).  Cost cell g, channel f' is element l = 32 g + f' (Q11), so
//      conv1 then reads a cell's channels from consecutive addresses: through the strides a cell's
//      32 channels lie on 32 different 128-byte lines of the permuted view.
//   1. conv1 (32 -> 16): per axis nb = ceil(G / 11) blocks of ceil(G / nb) cells (G = 12: 6 + 6,
//      G = 23: 8 + 8 + 7), one workgroup per key point and block.  The block's cost cells with a
//      one-cell halo (<= 13^3) are built in LDS one 8-channel quarter at a time as three bf16 piece
//      images, exactly as cpg.hip does, and conv1 runs on v_mfma_f32_16x16x32_bf16 with the
//      fp32-accurate split of split3.h, the four quarters accumulated in registers.  A halo cell
//      inside the grid is a real cost cell (read from the ordered target block again); one outside
//      the grid is the convolution's zero padding.
//   2. conv2 (16 -> 4) and conv3 (4 -> 1) on VALU with scalar-cache weights, as cpg.hip: per axis
//      ceil(G / 9) blocks of <= 9 logits; the block's h1 cells with a two-cell halo (<= 13^3 x 16
//      fp32, 140 KB) are loaded into LDS, conv2 covers the block's cells and a one-cell halo
//      (<= 11^3), conv3 the block.  h1 and h2 at cells outside the grid are exactly 0 (each
//      Conv3d pads its own input), not bias + partial sums.
//   3. softmax over the key point's C logits (global maximum subtracted) and the weighted mean of
//      the candidates, one workgroup per key point.
//
// Q11 (the reference's reshape of the permuted target): cost cell g, channel f' is element
// l = 32 g + f' of the (32, C) view, (f = l / C, c = l % C).  l < 2^20 is outside FastDiv's range
// (x < 2^16); launch 0 walks (f, c) and conv1 walks l, so neither divides.
#include "cpg_tiled.h"
#include "split3.h"

namespace dvcp {

constexpr int kCtB1 = 11;                        // conv1 block edge (output cells)
constexpr int kCtB2 = 9;                         // conv2/conv3 block edge (logits)
constexpr int kCtPV = 13 * 13 * 13;              // cells of a haloed block, both launches
constexpr int kCtT = (kCtB1 * kCtB1 * kCtB1 + 15) / 16;  // 16-voxel tiles of a conv1 block
constexpr int kCtW = kCtThreads / 64;
constexpr int kCtTW = (kCtT + kCtW - 1) / kCtW;  // tiles per wave

// Launch 0: out[p][f C + c] = tgt[p][f t_f + c t_c], 32 candidates x 32 features per workgroup
// through an LDS tile (reads along f, the permuted view's contiguous axis; writes along c).
__global__ __launch_bounds__(kCtThreads) void cpg_tiled_order_kernel(const float* __restrict__ tgt, int64_t t_p,
                                                                     int64_t t_f, int64_t t_c, int C,
                                                                     float* __restrict__ out) {
  __shared__ float tile[32][33];
  const int p = blockIdx.y, c0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const float* T = tgt + static_cast<int64_t>(p) * t_p;
  if (c0 + ty < C) tile[ty][tx] = T[tx * t_f + static_cast<int64_t>(c0 + ty) * t_c];
  __syncthreads();
  if (c0 + tx < C) out[static_cast<int64_t>(p) * 32 * C + static_cast<int64_t>(ty) * C + c0 + tx] = tile[tx][ty];
}

// Launch 1: conv1 of one block of one key point -> h1 (chunk x C x 16, bias added).  tl: the target
// blocks in Q11 order, tl_p floats apart.
__global__ __launch_bounds__(kCtThreads) void cpg_tiled_conv1_kernel(const float* __restrict__ src,
                                                                     const float* __restrict__ tl, int64_t tl_p, int G,
                                                                     int nb, int bs, CtMagic magic,
                                                                     const float* __restrict__ params,
                                                                     float* __restrict__ h1) {
  __shared__ __attribute__((aligned(16))) uint4 vsp[3 * kCtPV];  // [piece][cell]: 8 bf16 channels
  __shared__ __attribute__((aligned(16))) uint4 w1p[7 * 3 * 64];  // [k-step][piece][lane]
  __shared__ float sv[32];
  __shared__ float b1[16];

  const int p = blockIdx.y, tid = threadIdx.x;
  const int C = G * G * G;
  const CtBlock B(blockIdx.x, G, nb, bs);
  const int PX = B.bx + 2, PXY = PX * (B.by + 2), PV = PXY * (B.bz + 2);  // haloed block
  const int n = B.bx * B.by * B.bz, NT = (n + 15) / 16;
  // (operands < 13^3; a divisor 1 only meets 0)
  const FastDiv dPX = B.row(magic, 1), dPXY = B.plane(magic, 1), dBX = B.row(magic, 0), dBXY = B.plane(magic, 0);
  const float* P1 = params;
  const float* T = tl + static_cast<int64_t>(p) * tl_p;
  if (tid < 32) sv[tid] = src[static_cast<int64_t>(p) * 32 + tid];
  if (tid < 16) b1[tid] = P1[16 * 32 * 27 + tid];

  // conv1 as an implicit GEMM (cpg.hip): rows = 16-voxel tiles of the block's cells in block order,
  // a k-step = 4 taps x 8 channels, columns = the 16 output channels.  Wave w owns tiles w, w + 16,
  // ...; the input is haloed, so a tap is a constant address shift.
  const int lane = tid & 63, wave = tid >> 6, kg = lane >> 4, l16 = lane & 15;
  int vx[kCtTW];  // haloed address of the lane's voxel per tile (a padding row: voxel 0's cell)
#pragma unroll
  for (int i = 0; i < kCtTW; ++i) {
    const int v = 16 * (wave + kCtW * i) + l16;
    const uint32_t vv = v < n ? v : 0;
    const uint32_t z = dBXY.div(vv), r = vv - z * dBXY.d, y = dBX.div(r), x = r - y * dBX.d;
    vx[i] = static_cast<int>((z + 1) * PXY + (y + 1) * PX + (x + 1));
  }
  f32x4 acc[kCtTW];
#pragma unroll
  for (int i = 0; i < kCtTW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint16_t* vh = reinterpret_cast<uint16_t*>(vsp);
#pragma unroll 1
  for (int q = 0; q < 4; ++q) {
    __syncthreads();  // the previous quarter's MFMAs have read both images
    // this quarter's conv1 weights: k-step s, lane (co = l & 15, tap 4 s + (l >> 4)), channel j
    for (int i = tid; i < 7 * 64; i += kCtThreads) {
      const int l = i & 63, st = i >> 6, co = l & 15, tap = 4 * st + (l >> 4);
      bf16x8 w0, w1, w2;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const float w = tap < 27 ? P1[(co * 32 + 8 * q + jj) * 27 + tap] : 0.0f;
        __bf16 x0, x1, x2;
        split3(w, x0, x1, x2);
        w0[jj] = x0;
        w1[jj] = x1;
        w2[jj] = x2;
      }
      w1p[(st * 3 + 0) * 64 + l] = __builtin_bit_cast(uint4, w0);
      w1p[(st * 3 + 1) * 64 + l] = __builtin_bit_cast(uint4, w1);
      w1p[(st * 3 + 2) * 64 + l] = __builtin_bit_cast(uint4, w2);
    }
    // the quarter's cost cells over the haloed block, every (cell, channel) written once: a cell
    // outside the grid is conv1's zero padding, one inside it (halo or not) the real cost
    for (int i = tid; i < 8 * PV; i += kCtThreads) {
      const uint32_t cell = i >> 3, j = i & 7;
      const uint32_t hz = dPXY.div(cell), r = cell - hz * dPXY.d, hy = dPX.div(r), hx = r - hy * dPX.d;
      const int gx = B.ox + static_cast<int>(hx) - 1, gy = B.oy + static_cast<int>(hy) - 1,
                gz = B.oz + static_cast<int>(hz) - 1;
      float cost = 0.f;
      if (gx >= 0 && gx < G && gy >= 0 && gy < G && gz >= 0 && gz < G) {
        const uint32_t l = 32u * static_cast<uint32_t>((gz * G + gy) * G + gx) + 8u * q + j;  // Q11
        const float d = sv[8 * q + j] - T[l];
        cost = d * d;
      }
      __bf16 x0, x1, x2;
      split3(cost, x0, x1, x2);
      vh[i] = __builtin_bit_cast(uint16_t, x0);
      vh[8 * PV + i] = __builtin_bit_cast(uint16_t, x1);
      vh[16 * PV + i] = __builtin_bit_cast(uint16_t, x2);
    }
    __syncthreads();
#pragma unroll 1
    for (int st = 0; st < 7; ++st) {
      // lane's tap 4 st + kg (tap 27: zero weights, any in-range cell)
      const int tap = 4 * st + kg;
      const int off = tap < 27 ? (tap / 9 - 1) * PXY + ((tap / 3) % 3 - 1) * PX + (tap % 3 - 1) : 0;
      const bf16x8 w0 = __builtin_bit_cast(bf16x8, w1p[(st * 3 + 0) * 64 + lane]);
      const bf16x8 w1 = __builtin_bit_cast(bf16x8, w1p[(st * 3 + 1) * 64 + lane]);
      const bf16x8 w2 = __builtin_bit_cast(bf16x8, w1p[(st * 3 + 2) * 64 + lane]);
#pragma unroll
      for (int i = 0; i < kCtTW; ++i)
        if (wave + kCtW * i < NT) {  // wave-uniform
          const int cell = vx[i] + off;
          const bf16x8 a0 = __builtin_bit_cast(bf16x8, vsp[cell]);
          const bf16x8 a1 = __builtin_bit_cast(bf16x8, vsp[PV + cell]);
          const bf16x8 a2 = __builtin_bit_cast(bf16x8, vsp[2 * PV + cell]);
          acc[i] = mfma_split3(a0, a1, a2, w0, w1, w2, acc[i]);
        }
    }
  }
  // accumulator register r of lane l is voxel 16 t + 4 (l >> 4) + r, output channel l & 15: the 16
  // lanes of a voxel write its 64-byte h1 cell
  float* out = h1 + static_cast<int64_t>(p) * C * 16;
#pragma unroll
  for (int i = 0; i < kCtTW; ++i) {
    const int t = wave + kCtW * i;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int v = 16 * t + 4 * kg + r;
      if (t < NT && v < n) {
        const uint32_t z = dBXY.div(v), rr = v - z * dBXY.d, y = dBX.div(rr), x = rr - y * dBX.d;
        const int g = ((B.oz + static_cast<int>(z)) * G + B.oy + static_cast<int>(y)) * G + B.ox + static_cast<int>(x);
        out[static_cast<int64_t>(g) * 16 + l16] = acc[i][r] + b1[l16];
      }
    }
  }
}

// Launch 2: conv2 and conv3 of one block of one key point: h1 -> logits (chunk x C).
__global__ __launch_bounds__(kCtThreads) void cpg_tiled_conv23_kernel(const float* __restrict__ h1, int G, int nb,
                                                                      int bs, CtMagic magic,
                                                                      const float* __restrict__ params,
                                                                      float* __restrict__ logit) {
  __shared__ __attribute__((aligned(16))) float big[16 * kCtPV];  // h1 [co][cell], later h2 [co][cell]
  __shared__ float w3[4 * 27];
  __shared__ float bias[4 + 1];
  float* out1 = big;
  float* out2 = big;

  const int p = blockIdx.y, tid = threadIdx.x;
  const int C = G * G * G;
  const CtBlock B(blockIdx.x, G, nb, bs);
  const int LX = B.bx + 4, LXY = LX * (B.by + 4), LV = LXY * (B.bz + 4);  // h1 cells: two-cell halo
  const int MX = B.bx + 2, MXY = MX * (B.by + 2), MV = MXY * (B.bz + 2);  // h2 cells: one-cell halo
  const int n3 = B.bx * B.by * B.bz;
  const FastDiv dLX = B.row(magic, 2), dLXY = B.plane(magic, 2), dMX = B.row(magic, 1), dMXY = B.plane(magic, 1),
                dBX = B.row(magic, 0), dBXY = B.plane(magic, 0);
  const float* P2 = params + 16 * 32 * 27 + 16;
  const float* P3 = P2 + 4 * 16 * 27 + 4;
  if (tid < 4 * 27) w3[tid] = P3[tid];
  if (tid < 4) bias[tid] = P2[4 * 16 * 27 + tid];
  if (tid == 0) bias[4] = P3[4 * 27];

  // the block's h1 cells (zero outside the grid: conv2's padding)
  const float4* in = reinterpret_cast<const float4*>(h1 + static_cast<int64_t>(p) * C * 16);
  for (int cell = tid; cell < LV; cell += kCtThreads) {
    const uint32_t hz = dLXY.div(cell), r = cell - hz * dLXY.d, hy = dLX.div(r), hx = r - hy * dLX.d;
    const int gx = B.ox + static_cast<int>(hx) - 2, gy = B.oy + static_cast<int>(hy) - 2,
              gz = B.oz + static_cast<int>(hz) - 2;
    float4 v[4];
    if (gx >= 0 && gx < G && gy >= 0 && gy < G && gz >= 0 && gz < G) {
      const int64_t g = (gz * G + gy) * G + gx;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = in[g * 4 + k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      out1[(4 * k + 0) * LV + cell] = v[k].x;
      out1[(4 * k + 1) * LV + cell] = v[k].y;
      out1[(4 * k + 2) * LV + cell] = v[k].z;
      out1[(4 * k + 3) * LV + cell] = v[k].w;
    }
  }

  // conv2 on the MV <= 11^3 cells of the block and its one-cell halo, up to two per thread
  int hv[2];       // the cell's address in the h1 volume (a thread without a cell: cell 0's)
  bool inside[2];  // the cell exists and lies in the grid (else h2 is conv3's zero padding)
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const int e = tid + v * kCtThreads;
    const uint32_t ee = e < MV ? e : 0;
    const uint32_t z = dMXY.div(ee), r = ee - z * dMXY.d, y = dMX.div(r), x = r - y * dMX.d;
    hv[v] = static_cast<int>((z + 1) * LXY + (y + 1) * LX + (x + 1));
    const int gx = B.ox + static_cast<int>(x) - 1, gy = B.oy + static_cast<int>(y) - 1,
              gz = B.oz + static_cast<int>(z) - 1;
    inside[v] = e < MV && gx >= 0 && gx < G && gy >= 0 && gy < G && gz >= 0 && gz < G;
  }
  float o2[2][4];
#pragma unroll
  for (int v = 0; v < 2; ++v)
#pragma unroll
    for (int co = 0; co < 4; ++co) o2[v][co] = 0.f;
  __syncthreads();
  {
    // cpg.hip's plane loop: the 48 (ci, kd) planes in turn, a plane's 36 weights loaded at once
    // through the scalar cache; a wave runs its second voxel only when some lane has one
    const int hv0 = hv[0], hv1 = hv[1];
    auto planes = [&](auto two) {
      constexpr bool T2 = decltype(two)::value;
#pragma unroll 1
      for (int pl = 0; pl < 48; ++pl) {  // pl = 3 ci + kd
        float w[4][9];
#pragma unroll
        for (int co = 0; co < 4; ++co)
#pragma unroll
          for (int t = 0; t < 9; ++t) w[co][t] = P2[co * 16 * 27 + 9 * pl + t];
        const int ci = pl / 3, kd = pl - 3 * ci;
        const float* xin = out1 + ci * LV + (kd - 1) * LXY;
#pragma unroll
        for (int t9 = 0; t9 < 9; ++t9) {
          const int off = (t9 / 3 - 1) * LX + (t9 % 3 - 1);
          const float xa = xin[hv0 + off];
#pragma unroll
          for (int co = 0; co < 4; ++co) o2[0][co] = __fmaf_rn(w[co][t9], xa, o2[0][co]);
          if constexpr (T2) {
            const float xb = xin[hv1 + off];
#pragma unroll
            for (int co = 0; co < 4; ++co) o2[1][co] = __fmaf_rn(w[co][t9], xb, o2[1][co]);
          }
        }
      }
    };
    if (__builtin_amdgcn_readfirstlane(tid & ~63) + kCtThreads < MV)
      planes(std::true_type{});
    else
      planes(std::false_type{});
  }
  __syncthreads();  // every h1 value read; h2 overwrites them
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const int e = tid + v * kCtThreads;
    if (e < MV)
#pragma unroll
      for (int co = 0; co < 4; ++co) out2[co * MV + e] = inside[v] ? o2[v][co] + bias[co] : 0.f;
  }
  __syncthreads();

  // conv3 on the block's n3 <= 9^3 cells, one per thread
  if (tid < n3) {
    const uint32_t z = dBXY.div(tid), r = tid - z * dBXY.d, y = dBX.div(r), x = r - y * dBX.d;
    const int hc = static_cast<int>((z + 1) * MXY + (y + 1) * MX + (x + 1));
    float a = 0.f;
#pragma unroll
    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
      for (int t = 0; t < 27; ++t) {
        const int off = (t / 9 - 1) * MXY + ((t / 3) % 3 - 1) * MX + (t % 3 - 1);
        a = __fmaf_rn(w3[ci * 27 + t], out2[ci * MV + hc + off], a);
      }
    const int g = ((B.oz + static_cast<int>(z)) * G + B.oy + static_cast<int>(y)) * G + B.ox + static_cast<int>(x);
    logit[static_cast<int64_t>(p) * C + g] = a + bias[4];
  }
}

// Launch 3: softmax over the key point's C logits (torch: exp(x - max), sum, multiply by 1 / sum)
// and the weighted mean of its candidates.
__global__ __launch_bounds__(kCtThreads) void cpg_tiled_softmax_kernel(const float* __restrict__ logit,
                                                                       const float* __restrict__ cand, int C,
                                                                       float* __restrict__ vcp,
                                                                       float* __restrict__ weight) {
  __shared__ float red[32];
  const int p = blockIdx.x, tid = threadIdx.x;
  const float* lg = logit + static_cast<int64_t>(p) * C;
  float lmax = -__builtin_huge_valf();
  for (int g = tid; g < C; g += kCtThreads) lmax = fmaxf(lmax, lg[g]);
  const float m = block_max_f(lmax, red);
  float se = 0.f;
  for (int g = tid; g < C; g += kCtThreads) se += expf(lg[g] - m);
  const float inv = 1.0f / block_sum(se, red);
  const float* cq = cand + static_cast<int64_t>(p) * C * 3;
  float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
  for (int g = tid; g < C; g += kCtThreads) {
    const float w = expf(lg[g] - m) * inv;
    if (weight) weight[static_cast<int64_t>(p) * C + g] = w;
    sw += w;
    sx += w * cq[g * 3 + 0];
    sy += w * cq[g * 3 + 1];
    sz += w * cq[g * 3 + 2];
  }
  sw = block_sum(sw, red);
  sx = block_sum(sx, red);
  sy = block_sum(sy, red);
  sz = block_sum(sz, red);
  if (tid == 0) {
    vcp[static_cast<int64_t>(p) * 3 + 0] = sx / sw;
    vcp[static_cast<int64_t>(p) * 3 + 1] = sy / sw;
    vcp[static_cast<int64_t>(p) * 3 + 2] = sz / sw;
  }
}

const float* ct_forward_chunk(const float* src, const float* tgt, int64_t t_p, int64_t t_f, int64_t t_c,
                              const float* cand, int np, int G, const float* params, float* h1, float* logit,
                              float* order, float* vcp, float* weight, int64_t* tl_p, hipStream_t s) {
  const int C = G * G * G;
  const int nb1 = ct_blocks(G, kCtB1), bs1 = ct_block_size(G, nb1);
  const int nb2 = ct_blocks(G, kCtB2), bs2 = ct_block_size(G, nb2);
  const CtMagic magic1 = ct_magic(G, nb1, bs1), magic2 = ct_magic(G, nb2, bs2);
  const bool ordered = t_f == C && t_c == 1;  // already element l = f C + c
  const float* tl = ordered ? tgt : order;
  *tl_p = ordered ? t_p : int64_t(32) * C;
  if (!ordered)
    hipLaunchKernelGGL(cpg_tiled_order_kernel, dim3((C + 31) / 32, np), dim3(kCtThreads), 0, s, tgt, t_p, t_f, t_c, C,
                       order);
  hipLaunchKernelGGL(cpg_tiled_conv1_kernel, dim3(nb1 * nb1 * nb1, np), dim3(kCtThreads), 0, s, src, tl, *tl_p, G, nb1,
                     bs1, magic1, params, h1);
  hipLaunchKernelGGL(cpg_tiled_conv23_kernel, dim3(nb2 * nb2 * nb2, np), dim3(kCtThreads), 0, s, h1, G, nb2, bs2,
                     magic2, params, logit);
  if (vcp)
    hipLaunchKernelGGL(cpg_tiled_softmax_kernel, dim3(np), dim3(kCtThreads), 0, s, logit, cand, C, vcp, weight);
  return tl;
}

}  // namespace dvcp

extern "C" int64_t dvcp_cpg_tiled_workspace_bytes(int P, int G) {
  if (P <= 0 || G < 1 || G > dvcp::kCtMaxG) return 0;
  const int64_t per = dvcp::ct_ws_per_point(G);
  const int64_t chunk = dvcp::kCtWsCap / per;  // >= 41
  return (P < chunk ? P : chunk) * per;
}

extern "C" int dvcp_cpg_tiled(const float* src, const float* tgt, int64_t t_p, int64_t t_f, int64_t t_c,
                              const float* cand, int P, int G, const float* params, float* vcp, float* weight,
                              float* ws, int64_t ws_bytes, void* stream) {
  DVCP_REQUIRE(G >= 1 && G <= dvcp::kCtMaxG, "dvcp_cpg_tiled: grid side G=%d unsupported (1 <= G <= 32, C <= 32768)",
               G);
  if (P <= 0) return DVCP_OK;
  DVCP_REQUIRE(src && tgt && cand && params && vcp && ws, "dvcp_cpg_tiled: null pointer");
  const int64_t per = dvcp::ct_ws_per_point(G);
  DVCP_REQUIRE(ws_bytes >= per, "dvcp_cpg_tiled: workspace of %lld bytes holds no key point (%lld each)",
               static_cast<long long>(ws_bytes), static_cast<long long>(per));
  DVCP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0, "dvcp_cpg_tiled: workspace must be 16-byte aligned");
  const int C = G * G * G;
  int64_t chunk = ws_bytes / per;
  if (chunk > P) chunk = P;
  if (chunk > 32768) chunk = 32768;  // grid.y
  float* h1 = ws;
  float* logit = ws + chunk * C * 16;
  float* order = logit + chunk * C;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int64_t p0 = 0; p0 < P; p0 += chunk) {
    const int np = static_cast<int>(P - p0 < chunk ? P - p0 : chunk);
    int64_t tl_p;
    dvcp::ct_forward_chunk(src + p0 * 32, tgt + p0 * t_p, t_p, t_f, t_c, cand + p0 * C * 3, np, G, params, h1, logit,
                           order, vcp + p0 * 3, weight ? weight + p0 * C : nullptr, &tl_p, s);
  }
  return dvcp::launch_status("dvcp_cpg_tiled");
}
