// sa_mfma_common.h -- what the set-abstraction table kernels on the matrix cores share: the
// two-layer tables (sa2: 35-32-64, sa3: 67-64-64; pointnet2_utils.py:122-132 + :195-200 with REF-R
// R1) and the three-layer sa1 table.  One unit per kernel:
//   sa_mfma_pre.hip    the per-point pre-pass of the two-layer tables and the centres' curve order
//   sa_mfma_sa1.hip    sa1, 16-row half tiles, three chained MFMA layers
//   sa_mfma_sa2.hip    sa2 with a workspace, 16-row half tiles, two register sets
//   sa_mfma_sa3.hip    sa3 with a workspace, 32-row tiles, layer 1's registers refilled under the MFMAs
//   sa_mfma_plain.hip  sa2 and sa3 without a workspace (dvcp_sa_group_mlp), unpipelined
// A centre without hits (count < 1) gets zeros in every kernel, like the row-per-thread kernel of
// sa_mlp.hip; no list entry is read.
//
// Per centre the grouped rows form a dense batched GEMM chain, rows x C0 -> C1 -> C2 then a max
// over rows, which is what the matrix cores are for.  One wave per centre; its rows go through in
// n-tiles of 32 points (padded rows repeat the first hit, exactly the reference's padding, so
// the max is unchanged).
//   layer 1, transposed:  H1^T (C1 x 32) = W1 (C1 x C0) . X^T (C0 x 32)
//        A = W1 fragment (lane: output channel, k-half), B = X^T fragment (lane: point, k-half).
//        D has channels in registers and points on lanes...
//   layer 2:              H2 (32 x C2) = H1 (32 x C1) . W2^T (C1 x C2)
//        ...so each accumulator register of layer 1 is directly a k-step of layer 2's A operand
//        (k pair = channels c, c+4 of the register), no LDS round trip;  D has points in
//        registers and channels on lanes, so the max over points is a per-lane max over
//        registers plus one exchange between lane halves.
// Bias is the accumulator's initial value; BN (eval) is y = acc * scale + shift with scale/shift
// folded on the host side of the kernel (scale, shift of dvcp_sa_group_mlp's params); ReLU.
// Layer 1 runs on the fp32 MFMA (a k-ordered fp32 fma chain).  Layer 2 (~95 % of the flops) runs
// on the bf16 matrix cores, which are 16x the fp32 MFMA rate, with fp32 accuracy kept by a three-way
// split: every fp32 operand is the exact sum of three bf16 pieces
// x = x0 + x1 + x2 (each residual of a round-to-nearest bf16 conversion is exact in fp32), and
//   a.b ~ a0 b0 + (a0 b1 + a1 b0) + (a0 b2 + a1 b1 + a2 b0)
// drops only the terms a1 b2, a2 b1, a2 b2 (<= 2^-24 |a||b| together, the size of one fp32
// rounding of the product); the bf16 x bf16 products are exact in the fp32 accumulator.  Six
// v_mfma_f32_32x32x16_bf16 (32 cycles each) replace eight v_mfma_f32_32x32x2_f32 (64 cycles each)
// per 16 channels of k, so layer 2 costs 3/8 of the fp32 MFMA time.  The result differs from
// the fp32 chain by summation order and the dropped terms, within the fp32 tolerances of the
// parity tests (tests/test_gpu_kernels.py: rtol = atol = 1e-5; the split's own error against an
// fp64 evaluation is checked beside the fp32 path's in test_sa_split3_accuracy).
//
// Gathers.  A tile's inputs sit behind two dependent loads (list entry, then the U row and the
// point it names).  The three inference tables (sa1, sa2, sa3) walk each wave's 64-centre batch
// as one flat tile sequence whose schedule is wave-uniform scalar state, and issue tile t + 2's
// list entry and tile t + 1's gathers while tile t runs, so no tile waits for its own loads
// (tests/test_gpu_sa_pipeline.py).  The arithmetic per tile and its order
// are those of the unpipelined loop, which the kernel of sa_mfma_plain.hip still runs.
#pragma once
#include "common.h"
#include "split3.h"

namespace dvcp {

// split3 / mfma_split3: csrc/split3.h (the split written on register pairs)

constexpr int kMfmaWaves = 4;  // centres in flight per workgroup (one per SIMD)
constexpr int kSaGrid = 4096;  // workgroups of the grid-strided centre loops (a multiple of 8)

// v of lane j, j wave-uniform (v_readlane)
template <typename V>
__device__ __forceinline__ V lane_bcast(V v, int j) {
  if constexpr (sizeof(V) == 8) {
    const int64_t u = __builtin_bit_cast(int64_t, v);
    const int lo = __builtin_amdgcn_readlane(static_cast<int>(u & 0xFFFFFFFF), j);
    const int hi = __builtin_amdgcn_readlane(static_cast<int>(u >> 32), j);
    return __builtin_bit_cast(V, (static_cast<int64_t>(hi) << 32) | static_cast<uint32_t>(lo));
  } else {
    return __builtin_bit_cast(V, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
  }
}
// v of lane j, j per lane (ds_bpermute; every lane of the wave is active where this is used)
template <typename V>
__device__ __forceinline__ V lane_gather(V v, int j) {
  if constexpr (sizeof(V) == 8) {
    const int64_t u = __builtin_bit_cast(int64_t, v);
    const int lo = __builtin_amdgcn_ds_bpermute(j << 2, static_cast<int>(u & 0xFFFFFFFF));
    const int hi = __builtin_amdgcn_ds_bpermute(j << 2, static_cast<int>(u >> 32));
    return __builtin_bit_cast(V, (static_cast<int64_t>(hi) << 32) | static_cast<uint32_t>(lo));
  } else {
    return __builtin_bit_cast(V, __builtin_amdgcn_ds_bpermute(j << 2, __builtin_bit_cast(int, v)));
  }
}

// ---- the centres of a wave ---------------------------------------------------------------------

// The kernels are grid-strided over a centre index space, one centre per wave at a time: xcd == 0,
// all B*S centres; xcd != 0 (B % 8 == 0, grid a multiple of 8), workgroups reach the 8 XCDs round
// robin (blockIdx % 8), so XCD xo walks the centres of clouds xo, xo + 8, ... and each cloud's U
// table and point rows are fetched into one XCD's L2.  A wave's centres are index q0, q0 + qs, ...
// of the space; their metadata is loaded 64 centres at a time, one per lane, and read back by
// readlane (lane_bcast) or ds_bpermute (lane_gather), so a centre's first tile waits for neither.
// (Each kernel builds total, q0, qs, xo itself: the block as a shared function -- a struct with a
// constructor, a function returning the struct, a function on references -- changed every
// kernel's register numbering and operand order.)
//
// The metadata of this lane's centre, index qm of the space, for the two-layer tables: cloud,
// flat index cloud * S + centre (the row of count, list and out), rows to run (count clamped to
// nsample; 0: no hit, the centre's output is 0) and coordinates.  Lanes past the space keep what
// they hold (zeros).
template <typename T>
__device__ __forceinline__ void sa_centre_meta(int64_t qm, int64_t total, int xcd, int xo, int S,
                                               const int32_t* __restrict__ order, const int32_t* __restrict__ count,
                                               int nsample, const PointsView<T>& ctr, int& m_b, int& m_rows,
                                               int64_t& m_fc, T& m_cx, T& m_cy, T& m_cz) {
  if (qm < total) {
    const int64_t q = xcd ? (xo + 8 * (qm / S)) * static_cast<int64_t>(S) + qm % S : qm;
    // centre in curve order when `order` is given: consecutive waves then gather the U / point
    // rows of one spatial neighbourhood, which stay in L2 instead of being fetched again
    m_b = static_cast<int>(q / S);
    const int c = order ? order[q] : static_cast<int>(q % S);
    m_fc = static_cast<int64_t>(m_b) * S + c;
    const int r = count[m_fc];
    m_rows = r < 1 ? 0 : (r > nsample ? nsample : r);
    ctr.load3(m_b, c, m_cx, m_cy, m_cz);
  }
}

// ---- the half-tile pipeline of the packed kernels (sa1, sa2) -----------------------------------

// The half-tile walk.  A wave's 64-centre batch is one flat sequence of 32-row tiles; each tile takes the next two 16-row half tiles (centre, half) of the
// batch in order, a centre having max(1, ceil(rows / 16)) of them.  The walk is wave-uniform
// scalar state, so the tiles of steps t + 1 and t + 2 are named while tile t runs (the software
// pipeline of the kernels).  Past the batch's last tile the walk names (last centre, half 0), a
// valid half tile whose loads are issued like any other's and whose result nobody uses.
struct HalfPair {
  int jA, hA, jB, hB;  // first and second half tile; without a second one, the first again
  bool live, hasB;     // the tile exists; its second half tile exists
};
template <typename NH>
__device__ __forceinline__ HalfPair next_half_pair(int& js, int& hs, int& nhj, int ncen, NH nh_of) {
  HalfPair t;
  t.live = js < ncen;
  if (!t.live) {
    t.jA = t.jB = ncen - 1;
    t.hA = t.hB = 0;
    t.hasB = false;
    return t;
  }
  t.jA = js;
  t.hA = hs;
  if (++hs >= nhj) {
    hs = 0;
    if (++js < ncen) nhj = nh_of(js);
  }
  t.hasB = js < ncen;
  t.jB = t.hasB ? js : t.jA;
  t.hB = t.hasB ? hs : t.hA;
  if (t.hasB && ++hs >= nhj) {
    hs = 0;
    if (++js < ncen) nhj = nh_of(js);
  }
  return t;
}

// Stage 1 of the pipeline: the list entry of this lane's row (row r32 of the tile: its centre is
// the first or the second half tile's; padded rows repeat the first hit, pointnet2_utils.py:104-106).
// The centre's metadata comes by one ds_bpermute per value through the selected lane index.  A
// centre without hits reads no list entry: its lanes load the centre's own count instead (one load
// without a branch) and stage 2 takes point 0 for them (discarded).
__device__ __forceinline__ int half_pair_entry(const HalfPair& t, int64_t m_fc, int m_rows, int r32,
                                               const int32_t* __restrict__ count, const int32_t* __restrict__ list,
                                               int nsample) {
  const bool sB = r32 >= 16;
  const int jl = sB ? t.jB : t.jA;
  const int64_t fc = lane_gather(m_fc, jl);
  const int rows = lane_gather(m_rows, jl);
  const int row = 16 * (sB ? t.hB : t.hA) + (r32 & 15);
  const int32_t* e = rows == 0 ? count + fc : list + fc * nsample + (row < rows ? row : 0);
  return *e;
}

// ---- the layers --------------------------------------------------------------------------------

// ReLU of an accumulator register, max(x, +0) with a NaN giving 0 like `x > 0 ? x : 0`.  Written as
// fmaxf or as that select, the compiler puts a canonicalising v_max_f32 x, x in front of the
// v_max_f32 (it cannot see that an MFMA result is already canonical): two instructions per
// register, 32 + 32 per sa3 tile.  v_med3_f32(x, 0, +inf) is one, with the same result for every
// input (a NaN operand makes it min3, which skips the NaN: 0).
__device__ __forceinline__ float sa_relu(float x) {
  // +inf through an opaque scalar register: with both bounds visible the compiler folds the
  // median back into the two-instruction maximum
  float inf = __builtin_inff();
  asm("" : "+s"(inf));
  return __builtin_amdgcn_fmed3f(x, 0.0f, inf);
}

// output channel row of accumulator register r for lane half h (32x32 C/D map)
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

template <int D, int C1, int C2>
struct SaMfmaShape {
  static constexpr int C0 = 3 + D;
  static constexpr int KS = 3 + D / 2;  // k-steps of layer 1
  static constexpr int MT = C1 / 32;    // layer-1 output tiles
  static constexpr int CT = C2 / 32;    // layer-2 output tiles
  static constexpr int KB = MT * 2;     // k-steps of layer 2 (bf16 32x32x16, split3)
  static_assert(D % 8 == 0 && C1 % 32 == 0 && C2 % 32 == 0, "MFMA tiling");
};

// LDS image of the weights of the workspace kernels (sa2, sa3) in fragment order, staged once per
// workgroup.  They read wx and w2s only.  (Dropping the arrays they never read, and the stores
// that stage b1, s1, t1, changes their LDS size and every LDS offset, so the layout stays.)
template <int D, int C1, int C2>
struct SaMfmaLds {
  using S = SaMfmaShape<D, C1, C2>;
  float w1[1][S::KS][64];           // never written or read
  float wx[S::MT][2][64];           // decomposed layer 1: xyz columns only, k-steps (x|y), (z|0)
  bf16x8 w2s[S::CT][S::KB][3][64];  // B fragment of layer 2 as three bf16 pieces: [tile][k-step][piece][lane]
  float b1[S::MT][2][16];           // layer-1 bias / BN scale / BN shift by [tile][lane half][register]
  float s1[S::MT][2][16];
  float t1[S::MT][2][16];
};

// The U-row gather of the workspace kernels: the accumulator start of 32-channel tile mt of U row n
// of cloud b, four float4 per lane -- register r of lane half h is channel acc_row(r, h).
template <int C1>
__device__ __forceinline__ const float4* sa_u_row(const float* __restrict__ U, int64_t ub, int b, int n, int h) {
  return reinterpret_cast<const float4*>(U + b * ub + static_cast<int64_t>(n) * C1 + 4 * h);
}
__device__ __forceinline__ void sa_gather_u(const float4* ur, int mt, f32x16& u) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 q = ur[8 * mt + 2 * i];
    u[4 * i] = q.x;
    u[4 * i + 1] = q.y;
    u[4 * i + 2] = q.z;
    u[4 * i + 3] = q.w;
  }
}

// Layer 1 of the workspace kernels.  Layer 1 is linear in its input row [p - c, f]:
//   W1 [p - c; f] + b1 = W1x (p - c) + (W1f f + b1)
// and the second term depends only on the neighbour point, not on the centre.  sa_pre_mfma_kernel
// evaluates U[n] = W1f f_n + b1 once per input point (N rows instead of S x nsample), and the
// grouped kernel starts each layer-1 accumulator from the gathered U row and adds the xyz part
// with two MFMA k-steps, (x|y) and (z|0) on the lane halves, then the ReLU (BN is folded into U
// and W1x).  Only the summation order changes (features first, then xyz); the local
// coordinates are still formed per (centre, point) pair, so no cancellation is introduced.
// wx[mt][s][l]: this lane's element of the A fragment of k-step s, W1's xyz columns times BN1's scale.
template <int MT, typename T>
__device__ __forceinline__ void sa_layer1_xyz(f32x16 (&acc1)[MT], T px, T py, T pz, T cx, T cy, T cz, int h,
                                              const float (&wx)[MT][2][64], int l) {
  const float dx = static_cast<float>(px - cx);
  const float dy = static_cast<float>(py - cy);
  const float dz = static_cast<float>(pz - cz);
  const float x0 = h == 0 ? dx : dy, x1 = h == 0 ? dz : 0.0f;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    acc1[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wx[mt][0][l], x0, acc1[mt], 0, 0, 0);
    acc1[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wx[mt][1][l], x1, acc1[mt], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[mt][r] = sa_relu(acc1[mt][r]);
  }
}

// Layer 2 of one tile on the split-3 bf16 MFMAs: acc2[ct] += H1 . W2^T over the 2 MT k-steps, the A
// operand of k-step s being layer 1's accumulator registers 8 (s % 2) .. + 7 of tile s / 2.
// Products and their order are mfma_split3's, k-step by k-step, tile ct 0 then 1, in both forms.
// w2(ct, s, piece): the B fragment; refill(mt): called once layer 1's registers of channel tile
// mt have been read for the last time.
//
// AHEAD = false (sa2): each k-step is split, then multiplied.  The compiler emits a k-step as a
// burst of ~45 VALU followed by its 12 MFMAs; the waves of a SIMD overlap each other's bursts.
//
// AHEAD = true (sa3): an MFMA holds the vector issue port for 8 of its 32 cycles, and a wave fits
// about six VALU instructions into each gap.  The split of k-step s + 1 (Split3Stages: 12 stages
// of at most 5 instructions) is placed stage by stage behind the 12 MFMAs of k-step s; a
// scheduling barrier after each MFMA keeps VALU and MFMA instructions from crossing it (LDS and
// global loads, scalar code and waits stay free to move), so only k-step 0's split runs outside
// the MFMAs' shadow.  (`sched_group_barrier` groups alone left the emitted burst / cluster order
// as it was.)  The wave raises its priority over each k-step's MFMAs, so that the other waves'
// split bursts do not delay the chain it interleaves with.  The next pieces live beside the
// current ones: 132 VGPRs, three waves per SIMD.  Measured: sa3 faster
// with both together, with neither alone; sa2 with neither (and its 4-wave form then spills).
constexpr int kSchedPinVectorAlu = 0x4 | 0x10 | 0x20 | 0x40 | 0x80 | 0x100 | 0x200;  // all but VALU, MFMA, TRANS may cross
template <int MT, int CT, bool AHEAD, typename W2, typename Refill>
__device__ __forceinline__ void sa_layer2(const f32x16 (&acc1)[MT], f32x16 (&acc2)[CT], W2 w2, Refill refill) {
  static_assert(6 * CT == Split3Stages::kStages, "one stage of the next split per MFMA of a k-step");
  constexpr int KB = 2 * MT;
  Split3Stages sp;
  auto stage = [&](int s, int i) {  // stage i of k-step s's split
    const int r = 8 * (s % 2) + 2 * (i / 3);
    sp.stage(i, acc1[s / 2][r], acc1[s / 2][r + 1]);
  };
  if (AHEAD) {
#pragma unroll
    for (int i = 0; i < Split3Stages::kStages; ++i) stage(0, i);
  }
#pragma unroll
  for (int s = 0; s < KB; ++s) {
    Split3 a;
    if (AHEAD) {
      a = sp.pieces();
    } else {
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = acc1[s / 2][8 * (s % 2) + j];
      a = split3(x);
      if (s % 2 == 1) refill(s / 2);
    }
    if (AHEAD) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const bf16x8 b0 = w2(ct, s, 0), b1 = w2(ct, s, 1), b2 = w2(ct, s, 2);
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        acc2[ct] = mfma_split3_product(m, a, b0, b1, b2, acc2[ct]);
        if (AHEAD && s + 1 < KB) {
          stage(s + 1, 6 * ct + m);
          __builtin_amdgcn_sched_barrier(kSchedPinVectorAlu);
        }
      }
    }
    if (AHEAD) __builtin_amdgcn_s_setprio(0);
    if (AHEAD && s % 2 == 0) refill(s / 2);  // k-step s + 1, the last reader of tile s / 2, is split
  }
}

// ---- the launchers, one per unit ---------------------------------------------------------------

// grid of the centre loops and whether it takes the per-XCD index space
struct SaGrid {
  int grid, xcd;
  SaGrid(int B, int S) {
    const int64_t centres = static_cast<int64_t>(B) * S;
    grid = static_cast<int>(centres < kSaGrid * kMfmaWaves ? (centres + kMfmaWaves - 1) / kMfmaWaves : kSaGrid);
    xcd = B % 8 == 0 && grid % 8 == 0 ? 1 : 0;
  }
};

// what the two-layer table kernels take (U, ub, order: the workspace, null / 0 without one)
template <typename T>
struct SaTableArgs {
  PointsView<T> pts, ctr;
  int S, B;
  const float* feat;
  int64_t fb, fn;
  const int32_t* count;
  const int32_t* list;
  int nsample;
  const float* params;
  const float* U;
  int64_t ub;
  const int32_t* order;
  float* out;
};

// Each enqueues on st; the caller reads launch_status() after the last one.
// sa_mfma_pre.hip: the centres' curve order (B x S), and U = W1f f + b1 per input point (B x N x C1)
template <typename T>
void launch_sa_order(PointsView<T> ctr, int S, int B, int32_t* order, hipStream_t st);
template <int D, int C1>
void launch_sa_pre(const float* feat, int64_t fb, int64_t fn, int N, int B, const float* params, float* U,
                   const int64_t* rows, int Nf, hipStream_t st);
// sa_mfma_sa2.hip (35-32-64), sa_mfma_sa3.hip (67-64-64): with a workspace; sa_mfma_plain.hip: both, without
template <typename T>
void launch_sa2_mfma(const SaTableArgs<T>& a, hipStream_t st);
template <typename T>
void launch_sa3_mfma(const SaTableArgs<T>& a, hipStream_t st);
template <typename T, int D, int C1, int C2>
void launch_sa_plain_mfma(const SaTableArgs<T>& a, hipStream_t st);
// sa_mfma_sa1.hip: the three-layer table (3-16-16-32, 6-16-16-32)
template <typename T, typename FT, int D>
int launch_sa1_mfma(const void* xyz, int64_t sb, int64_t sc, int64_t sn, const void* c, int64_t cb, int64_t cc,
                    int64_t cn, int S, int B, const void* feat, int64_t fb, int64_t fd, int64_t fn, const int32_t* count,
                    const int32_t* list, int nsample, const float* params, float* out, hipStream_t st);

}  // namespace dvcp
