// paper_bwd.hip -- the paper-faithful mode's 1-D CPG backward (DeepVCP paper, Lu et al. ICCV 2019; NOT
// reference parity, like paper.hip).  The weighting layer's backward is in paper_wl_train.hip.
//
//   cpg1d_bwd_kernel      backward of cpg1d_kernel (paper Sec. 3.6; csrc/paper.hip): one wave per key
//                         point recomputes the forward into LDS exactly as the forward does (cost,
//                         conv1, conv2, logits, softmax with the row maximum subtracted), then runs
//                         the softmax / weighted-mean backward and the three transposed convolutions
//                         there.  d src and d tgt have one writer per element.  The parameter
//                         gradients stay in registers (each lane owns 24 + 3 + 3 weights) while the
//                         workgroup walks key points p, p + grid, ...; one partial row per workgroup,
//                         folded in index order in fp64 (fold_rows, fold.hip).
//
// No atomics anywhere: two identical calls give identical bits.
#include "common.h"

namespace dvcp {

// ----------------------------------------------------------------------------- 1-D CPG backward
constexpr int kC1bMaxG = 64;              // cpg1d_kernel's kC1MaxG
constexpr int kC1bLd = kC1bMaxG + 2;      // column z + 1 holds candidate z; 0 and Gz + 1.. are padding
constexpr int kC1bW1 = 16 * 32 * 3, kC1bW2 = 4 * 16 * 3, kC1bW3 = 4 * 3;
constexpr int kC1bParams = kC1bW1 + 16 + kC1bW2 + 4 + kC1bW3 + 1;  // dvcp_cpg1d_nparams()
constexpr int kC1bMaxGrid = 256;          // workgroups (partial rows): one per CU

static int c1b_grid(int P) { return P < kC1bMaxGrid ? P : kC1bMaxGrid; }

__global__ __launch_bounds__(kC1bMaxG) void cpg1d_bwd_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                             const float* __restrict__ cand, int P, int Gz,
                                                             const float* __restrict__ params,
                                                             const float* __restrict__ gvcp, float* __restrict__ gsrc,
                                                             float* __restrict__ gtgt, float* __restrict__ partial) {
  __shared__ float cost[32][kC1bLd];
  __shared__ float h1[16][kC1bLd];
  __shared__ float h2[4][kC1bLd];
  __shared__ float gh1[16][kC1bLd];  // d loss / d h1, the same columns
  __shared__ float gh2[4][kC1bLd];
  __shared__ float glg[kC1bLd];      // d loss / d logit
  const int z = threadIdx.x;
  const bool in = z < Gz;
  const float* W1 = params;
  const float* b1 = W1 + kC1bW1;
  const float* W2 = b1 + 16;
  const float* b2 = W2 + kC1bW2;
  const float* W3 = b2 + 4;
  const float* b3 = W3 + kC1bW3;
  // this lane's weights: conv1.W[co1][8 q1 .. 8 q1 + 8][0..3], conv2.W[co2][ci2][0..3], and for
  // z < 4 conv3.W[0][z][0..3]; the biases with the lane of the row's first weight
  const int co1 = z >> 2, q1 = z & 3, co2 = z >> 4, ci2 = z & 15, ci3 = z & 3;
  float dW1[8][3], dW2[3], dW3[3], db1 = 0.f, db2 = 0.f;
  double db3 = 0.0;  // this lane's own logits' terms (see the softmax backward below)
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int k = 0; k < 3; ++k) dW1[c][k] = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) dW2[k] = dW3[k] = 0.f;

  for (int p = blockIdx.x; p < P; p += gridDim.x) {
    __syncthreads();  // the previous key point's readers are done
    // ---- the forward, as cpg1d_kernel writes it
    const float* sp = src + static_cast<int64_t>(p) * 32;
    const float* tp = tgt + (static_cast<int64_t>(p) * Gz + (in ? z : 0)) * 32;
    for (int f = 0; f < 32; ++f) {
      float v = 0.f;
      if (in) {
        const float d = sp[f] - tp[f];
        v = d * d;
      }
      cost[f][z + 1] = v;
      if (z == 0) cost[f][0] = 0.f;
      if (z == 0) cost[f][kC1bMaxG + 1] = 0.f;
    }
    __syncthreads();
    for (int co = 0; co < 16; ++co) {
      float acc = 0.f;
      for (int ci = 0; ci < 32; ++ci)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc = __fmaf_rn(W1[(co * 32 + ci) * 3 + k], cost[ci][z + k], acc);
      h1[co][z + 1] = in ? acc + b1[co] : 0.f;
      if (z == 0) h1[co][0] = 0.f;
      if (z == 0) h1[co][kC1bMaxG + 1] = 0.f;
    }
    __syncthreads();
    for (int co = 0; co < 4; ++co) {
      float acc = 0.f;
      for (int ci = 0; ci < 16; ++ci)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc = __fmaf_rn(W2[(co * 16 + ci) * 3 + k], h1[ci][z + k], acc);
      h2[co][z + 1] = in ? acc + b2[co] : 0.f;
      if (z == 0) h2[co][0] = 0.f;
      if (z == 0) h2[co][kC1bMaxG + 1] = 0.f;
    }
    __syncthreads();
    float lg = 0.f;
    for (int ci = 0; ci < 4; ++ci)
#pragma unroll
      for (int k = 0; k < 3; ++k) lg = __fmaf_rn(W3[ci * 3 + k], h2[ci][z + k], lg);
    lg = lg + b3[0];
    const float m = wave_max_f(in ? lg : -__builtin_huge_valf());
    const float e = in ? expf(lg - m) : 0.f;
    const float inv = 1.0f / wave_sum(e);
    const float w = e * inv;
    const float* cq = cand + (static_cast<int64_t>(p) * Gz + (in ? z : 0)) * 3;
    const float sw = wave_sum(w);
    const float vx = wave_sum(in ? w * cq[0] : 0.f) / sw;
    const float vy = wave_sum(in ? w * cq[1] : 0.f) / sw;
    const float vz = wave_sum(in ? w * cq[2] : 0.f) / sw;
    // ---- vcp = sum(w cand) / sum(w): d / d w_z = (cand_z - vcp) / sum(w); then the softmax
    const float* gv = gvcp + static_cast<int64_t>(p) * 3;
    const float gw = in ? (gv[0] * (cq[0] - vx) + gv[1] * (cq[1] - vy) + gv[2] * (cq[2] - vz)) / sw : 0.f;
    // d loss / d logit_z = w_z (gw_z - sum_j w_j gw_j), in fp64: conv3.bias' gradient is the sum of
    // these over the line, which is zero (softmax is shift invariant); in fp32 it would come out as
    // the sum of their rounding errors, growing with the number of key points
    const double wd = static_cast<double>(w);
    const double dot = wave_sum(wd * static_cast<double>(gw));
    const double gl = in ? wd * (static_cast<double>(gw) - dot) : 0.0;
    db3 += gl;
    glg[z + 1] = static_cast<float>(gl);
    if (z == 0) glg[0] = 0.f;
    if (z == 0) glg[kC1bMaxG + 1] = 0.f;
    __syncthreads();
    // ---- transposed convolutions: out[z'] read in[z' + k - 1], so in[z] collects out[z - k + 1]
    for (int ci = 0; ci < 4; ++ci) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) acc = __fmaf_rn(W3[ci * 3 + k], glg[z + 2 - k], acc);
      gh2[ci][z + 1] = in ? acc : 0.f;  // the padding columns fed nothing forward
      if (z == 0) gh2[ci][0] = 0.f;
      if (z == 0) gh2[ci][kC1bMaxG + 1] = 0.f;
    }
    __syncthreads();
    for (int ci = 0; ci < 16; ++ci) {
      float acc = 0.f;
      for (int co = 0; co < 4; ++co)
#pragma unroll
        for (int k = 0; k < 3; ++k) acc = __fmaf_rn(W2[(co * 16 + ci) * 3 + k], gh2[co][z + 2 - k], acc);
      gh1[ci][z + 1] = in ? acc : 0.f;
      if (z == 0) gh1[ci][0] = 0.f;
      if (z == 0) gh1[ci][kC1bMaxG + 1] = 0.f;
    }
    __syncthreads();
    // ---- parameter gradients: this lane's weights, the line walked in order
    for (int zz = 0; zz < Gz; ++zz) {
      const float g1 = gh1[co1][zz + 1];
      db1 += g1;
#pragma unroll
      for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) dW1[c][k] = __fmaf_rn(g1, cost[8 * q1 + c][zz + k], dW1[c][k]);
      const float g2 = gh2[co2][zz + 1];
      db2 += g2;
#pragma unroll
      for (int k = 0; k < 3; ++k) dW2[k] = __fmaf_rn(g2, h1[ci2][zz + k], dW2[k]);
      const float g3 = glg[zz + 1];
#pragma unroll
      for (int k = 0; k < 3; ++k) dW3[k] = __fmaf_rn(g3, h2[ci3][zz + k], dW3[k]);
    }
    if (!gsrc && !gtgt) continue;  // uniform
    // ---- d cost (conv1 transposed), then cost = (src - tgt)^2
    float gc[32];
#pragma unroll
    for (int ci = 0; ci < 32; ++ci) gc[ci] = 0.f;
    for (int co = 0; co < 16; ++co) {
      const float a0 = gh1[co][z + 2], a1 = gh1[co][z + 1], a2 = gh1[co][z];
#pragma unroll
      for (int ci = 0; ci < 32; ++ci) {
        const float* wk = W1 + (co * 32 + ci) * 3;
        gc[ci] = __fmaf_rn(wk[2], a2, __fmaf_rn(wk[1], a1, __fmaf_rn(wk[0], a0, gc[ci])));
      }
    }
    __syncthreads();  // every lane is done with cost: it now carries d loss / d src's terms
    float* gt = gtgt ? gtgt + (static_cast<int64_t>(p) * Gz + (in ? z : 0)) * 32 : nullptr;
#pragma unroll
    for (int ci = 0; ci < 32; ++ci) {
      float v = 0.f;
      if (in) {
        v = 2.0f * (sp[ci] - tp[ci]) * gc[ci];
        if (gt) gt[ci] = -v;
      }
      cost[ci][z + 1] = v;
    }
    __syncthreads();
    if (gsrc && z < 32) {
      float s = 0.f;
      for (int zz = 0; zz < Gz; ++zz) s += cost[z][zz + 1];
      gsrc[static_cast<int64_t>(p) * 32 + z] = s;
    }
  }
  float* o = partial + static_cast<int64_t>(blockIdx.x) * kC1bParams;
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int k = 0; k < 3; ++k) o[(co1 * 32 + 8 * q1 + c) * 3 + k] = dW1[c][k];
  if (q1 == 0) o[kC1bW1 + co1] = db1;
  float* o2 = o + kC1bW1 + 16;
#pragma unroll
  for (int k = 0; k < 3; ++k) o2[(co2 * 16 + ci2) * 3 + k] = dW2[k];
  if (ci2 == 0) o2[kC1bW2 + co2] = db2;
  float* o3 = o2 + kC1bW2 + 4;
  if (z < 4) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o3[z * 3 + k] = dW3[k];
  }
  const double db3w = wave_sum(db3);
  if (z == 0) o3[kC1bW3] = static_cast<float>(db3w);
}

}  // namespace dvcp

extern "C" int64_t dvcp_cpg1d_backward_workspace_bytes(int P) {
  if (P <= 0) return 0;
  return static_cast<int64_t>(dvcp::c1b_grid(P)) * dvcp::kC1bParams * 4;
}

extern "C" int dvcp_cpg1d_backward(const float* src, const float* tgt, const float* cand, int P, int Gz,
                                   const float* params, const float* grad_vcp, float* grad_src, float* grad_tgt,
                                   void* workspace, int64_t ws_bytes, float* grad_params, void* stream) {
  DVCP_REQUIRE(Gz >= 1 && Gz <= dvcp::kC1bMaxG && P >= 0, "dvcp_cpg1d_backward: Gz=%d unsupported (1..%d), P=%d", Gz,
               dvcp::kC1bMaxG, P);
  DVCP_REQUIRE(params && grad_params, "dvcp_cpg1d_backward: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (P == 0) {  // no key point: zero parameter gradients, nothing else to write
    if (hipMemsetAsync(grad_params, 0, dvcp::kC1bParams * 4, st) != hipSuccess)
      return dvcp::launch_status("dvcp_cpg1d_backward(empty)");
    return DVCP_OK;
  }
  DVCP_REQUIRE(src && tgt && cand && grad_vcp && workspace, "dvcp_cpg1d_backward: null pointer");
  const int64_t need = dvcp_cpg1d_backward_workspace_bytes(P);
  DVCP_REQUIRE(ws_bytes >= need, "dvcp_cpg1d_backward: workspace of %lld bytes is short of %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(need));
  const int grid = dvcp::c1b_grid(P);
  float* ws = static_cast<float*>(workspace);
  hipLaunchKernelGGL(dvcp::cpg1d_bwd_kernel, dim3(grid), dim3(dvcp::kC1bMaxG), 0, st, src, tgt, cand, P, Gz, params,
                     grad_vcp, grad_src, grad_tgt, ws);
  if (int e = dvcp::launch_status("dvcp_cpg1d_backward")) return e;
  dvcp::fold_rows(ws, grid, dvcp::kC1bParams, dvcp::kC1bParams, grad_params, st);
  return dvcp::launch_status("dvcp_cpg1d_backward(sum)");
}
