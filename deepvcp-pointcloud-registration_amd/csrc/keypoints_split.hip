// keypoints_split.hip -- source key-point stage for up to 1024 key points, cut where keypoints.hip's
// one-workgroup LDS plan stops fitting (K <= 256 there: K * 32 ball entries and distances in LDS).
//
// Same semantics and rounding as keypoints.hip steps 1-5 (REF-R):
//   deepVCP.py:44-46  (R2) keypts = index_points(fe_xyz, topk)
//   deepVCP.py:54     sample_and_group(npoint=K, radius=1, nsample=32, keypts, None, returnidx)
//                     -> FPS among the K key points (pointnet2_utils.py:63-84) and a ball query
//                        among them (:87-107); grouped = keypts[idx] - centre
//   deepVCP.py:62     src_keyfeats = fe_feat[picked]   (Q4: key-point-local indices into FE rows)
//   get_cat_feat_src.py:37-53  dist = ||(keypt - grouped) + 1e-6||, w = dist / sum_j dist,
//                     cat([grouped - keypt, feat * w])  (Q5)  -> .float() at the DFE input
//   deepVCP.py:86-91  (R3) moved = R_init @ keypts (fp64)
//
// Consecutive launches on the caller's stream, no flags, tickets or waits between workgroups:
//   1. select: one workgroup per pair.  Gathers the key points (keypts, moved, and the SoA
//      coordinates into the workspace) and runs the FPS among them: the serial part.  Each lane
//      keeps up to four key points and their running minima in registers; LDS holds the SoA
//      coordinates (the step's centre is read from it), the FPS order and one argmax slot per wave.
//   2. ball: one wave per centre slot.  The wave tests 64 key points per round (lowest indices
//      first), ranks the hits with a ballot and stops once nsample are found; the lanes past the
//      count write the first hit.  A 128-byte row of the ball lists per centre.
//   3. rows: eight key points per workgroup, one thread per (key point, entry).  Distances through
//      LDS for the sequential row sum, the 35-float rows staged in LDS and written as one
//      contiguous block with 16-byte stores; a feature row is read with eight 16-byte loads.
//   backward rows: 3.'s grid over the forward's workspace; weights recomputed, a half-wave per key
//      point walks its entries with one lane per feature column and adds the row's repeats of its
//      first entry (the padding) in registers before the float atomic.
// Workspace (caller memory, 16-byte aligned; kp_ws_layout): coordinates B x 3 x K (dtype, SoA),
// FPS order B x K int32, ball lists B x K x nsample int32, each region padded to 16 bytes.
// Kernels 3 and the backward clamp what they read from it to [0, K-1].
#include "fps_common.h"

namespace dvcp {

constexpr int kKsMaxK = 1024;
constexpr int kKsMaxNs = 32;
constexpr int kKsSelThreads = 256;  // one wave per SIMD; up to kKsMaxK / kKsSelThreads points per lane
constexpr int kKsBallThreads = 256;
constexpr int kKsBallWaves = kKsBallThreads / kWave;  // centre slots per workgroup
constexpr int kKsRowKp = 8;                           // key points per workgroup
constexpr int kKsRowThreads = kKsRowKp * kKsMaxNs;    // one thread per entry

struct KpWs {
  int64_t fidx, pidx, total;  // byte offsets (the coordinates start at 0)
};

static bool kp_ws_args_ok(int dtype, int B, int K, int ns) {
  return (dtype == DVCP_F32 || dtype == DVCP_F64) && B > 0 && K >= 1 && K <= kKsMaxK && ns >= 1 && ns <= kKsMaxNs &&
         K >= ns;
}

static KpWs kp_ws_layout(int dtype, int B, int K, int ns) {
  const int64_t es = dtype == DVCP_F64 ? 8 : 4;
  auto pad = [](int64_t v) { return (v + 15) & ~static_cast<int64_t>(15); };
  KpWs w;
  w.fidx = pad(static_cast<int64_t>(B) * 3 * K * es);
  w.pidx = w.fidx + pad(static_cast<int64_t>(B) * K * 4);
  w.total = w.pidx + pad(static_cast<int64_t>(B) * K * ns * 4);
  return w;
}

// ---------------------------------------------------------------------------------------------
// 1. select: gather + FPS among the key points.  Key point n lives in lane n % THREADS, register
// n / THREADS.
template <typename T, int THREADS, int PPL>
__global__ __launch_bounds__(THREADS) void kp_select_kernel(const T* __restrict__ fe_xyz, int S,
                                                            const int64_t* __restrict__ topk, int K,
                                                            const int64_t* __restrict__ kstart,
                                                            const double* __restrict__ R_init, int64_t r_b,
                                                            T* __restrict__ keypts, double* __restrict__ moved,
                                                            T* __restrict__ ws_xyz, int* __restrict__ ws_fidx) {
  constexpr int KP = THREADS * PPL;
  __shared__ T kx[KP], ky[KP], kz[KP];
  __shared__ int fidx[KP];
  __shared__ uint64_t slots[2][THREADS / kWave];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const T* X = fe_xyz + static_cast<int64_t>(b) * 3 * S;
  T* W = ws_xyz + static_cast<int64_t>(b) * 3 * K;
  const double* R = R_init + b * r_b;

  T px[PPL], py[PPL], pz[PPL];
  float dmin[PPL];
#pragma unroll
  for (int q = 0; q < PPL; ++q) {
    const int n = q * THREADS + tid;
    px[q] = py[q] = pz[q] = 0;
    dmin[q] = -1.0f;
    if (n < K) {
      int64_t s = topk[static_cast<int64_t>(b) * K + n];
      s = s < 0 ? 0 : (s >= S ? S - 1 : s);
      const T x = X[s], y = X[S + s], z = X[2 * S + s];
      px[q] = x;
      py[q] = y;
      pz[q] = z;
      dmin[q] = 1e10f;
      kx[n] = x;
      ky[n] = y;
      kz[n] = z;
      W[n] = x;
      W[K + n] = y;
      W[2 * K + n] = z;
      T* o = keypts + (static_cast<int64_t>(b) * K + n) * 3;
      o[0] = x;
      o[1] = y;
      o[2] = z;
      // R3: moved = R_init @ keypts, fp64, MKL dgemm rounding (fma chain over the 3 terms)
      double* m = moved + (static_cast<int64_t>(b) * K + n) * 3;
      const double dx = static_cast<double>(x), dy = static_cast<double>(y), dz = static_cast<double>(z);
#pragma unroll
      for (int a = 0; a < 3; ++a) m[a] = dot3_blas<double>(R[3 * a], R[3 * a + 1], R[3 * a + 2], dx, dy, dz);
    }
  }
  __syncthreads();

  // FPS among the K key points (fp32 running min, strict '<', first-index argmax)
  int cur = static_cast<int>(kstart[b]);
  cur = cur < 0 || cur >= K ? 0 : cur;
  for (int step = 0; step < K; ++step) {
    if (tid == 0) fidx[step] = cur;
    const T cx = kx[cur], cy = ky[cur], cz = kz[cur];
    // the lane's best: largest running minimum, lowest index among equals (q ascending, strict '>');
    // a lane without points offers -1, below every real minimum
    float best = -1.0f;
    int bidx = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < PPL; ++q) {
      const T dx = px[q] - cx, dy = py[q] - cy, dz = pz[q] - cz;
      const T d = (dx * dx + dy * dy) + dz * dz;
      if (dmin[q] >= 0.0f && d < static_cast<T>(dmin[q])) dmin[q] = static_cast<float>(d);
      if (dmin[q] > best) {
        best = dmin[q];
        bidx = q * THREADS + tid;
      }
    }
    // wave argmax on DPP: the maximum, then the lowest index that holds it (both wave-uniform)
    const float wmax = wave_maxf_dpp(best);
    const int widx = wave_mini_dpp(best == wmax ? bidx : 0x7fffffff);
    if (lane == 0) slots[step & 1][wave] = wmax >= 0.0f ? argmax_key(wmax, static_cast<uint32_t>(widx)) : 0ull;
    lds_barrier();
    uint64_t m = slots[step & 1][0];
#pragma unroll
    for (int q = 1; q < THREADS / kWave; ++q) m = slots[step & 1][q] > m ? slots[step & 1][q] : m;
    cur = static_cast<int>(key_index(m));
  }
  __syncthreads();
  int* fo = ws_fidx + static_cast<int64_t>(b) * K;
  for (int n = tid; n < K; n += THREADS) fo[n] = fidx[n];
}

// ---------------------------------------------------------------------------------------------
// 2. ball query among the key points: centre slot i = key point fidx[i]; one wave per slot.
template <typename T>
__global__ __launch_bounds__(kKsBallThreads) void kp_ball_kernel(const T* __restrict__ ws_xyz,
                                                                 const int* __restrict__ ws_fidx, int K, T r2, int ns,
                                                                 int* __restrict__ ws_pidx) {
  const int b = blockIdx.x, lane = threadIdx.x & 63;
  const int slot = blockIdx.y * kKsBallWaves + (threadIdx.x >> 6);
  if (slot >= K) return;  // whole waves; the kernel has no barrier
  const T* x = ws_xyz + static_cast<int64_t>(b) * 3 * K;
  const T* y = x + K;
  const T* z = y + K;
  int c = ws_fidx[static_cast<int64_t>(b) * K + slot];
  c = c < 0 ? 0 : (c >= K ? K - 1 : c);
  const T cx = x[c], cy = y[c], cz = z[c], ssc = sumsq3(cx, cy, cz);
  int* out = ws_pidx + (static_cast<int64_t>(b) * K + slot) * ns;
  int cnt = 0, first = K;
  for (int j0 = 0; j0 < K && cnt < ns; j0 += kWave) {
    const int j = j0 + lane;
    bool hit = false;
    if (j < K) {
      const T jx = x[j], jy = y[j], jz = z[j];
      const T d2 = expansion_d2(dot3_blas(cx, cy, cz, jx, jy, jz), ssc, sumsq3(jx, jy, jz));
      hit = !(d2 > r2);
    }
    const uint64_t mask = __ballot(hit);
    if (mask == 0) continue;
    if (cnt == 0) first = j0 + __builtin_ctzll(mask);
    const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
    if (hit && pos < ns) out[pos] = j;
    cnt += __popcll(mask);
  }
  if (lane >= cnt && lane < ns) out[lane] = first;
}

// ---------------------------------------------------------------------------------------------
// One entry of Get_Cat_Feat_Src: key point i (top-k order), ball entry p of centre c.  Returns the
// row's three coordinate columns (grouped - keypt) and dist = ||(keypt - grouped) + 1e-6||.
template <typename T>
__device__ __forceinline__ void kp_entry(const T* __restrict__ x, int K, int i, int c, int p, T& ox, T& oy, T& oz,
                                         T& dist) {
  const T* y = x + K;
  const T* z = y + K;
  const T eps = static_cast<T>(1e-6);
  const T ix = x[i], iy = y[i], iz = z[i];
  const T gx = x[p] - x[c], gy = y[p] - y[c], gz = z[p] - z[c];
  const T ex = (ix - gx) + eps, ey = (iy - gy) + eps, ez = (iz - gz) + eps;
  dist = sqrt_rn(fma_rn<T>(ez, ez, fma_rn<T>(ey, ey, ex * ex)));
  ox = gx - ix;
  oy = gy - iy;
  oz = gz - iz;
}

__device__ __forceinline__ int kp_clamp(int v, int K) { return v < 0 ? 0 : (v >= K ? K - 1 : v); }

// 3. rows of the DFE input: [grouped - keypt (3), feat * w (32)] -> fp32
template <typename T>
__global__ __launch_bounds__(kKsRowThreads) void kp_rows_kernel(const T* __restrict__ ws_xyz,
                                                                const int* __restrict__ ws_fidx,
                                                                const int* __restrict__ ws_pidx,
                                                                const float* __restrict__ fe_feat, int S, int K,
                                                                int ns, float* __restrict__ src_cat) {
  __shared__ T sdist[kKsRowThreads];
  __shared__ __attribute__((aligned(16))) float stage[kKsRowThreads * 35];

  const int b = blockIdx.x, i0 = blockIdx.y * kKsRowKp, tid = threadIdx.x;
  const int cnt = K - i0 < kKsRowKp ? K - i0 : kKsRowKp;
  const int il = tid / ns, j = tid - il * ns;
  const bool on = tid < cnt * ns;
  const T* x = ws_xyz + static_cast<int64_t>(b) * 3 * K;
  int p = 0;
  T ox = 0, oy = 0, oz = 0, dist = 0;
  if (on) {
    const int i = i0 + il;
    const int c = kp_clamp(ws_fidx[static_cast<int64_t>(b) * K + i], K);
    p = kp_clamp(ws_pidx[(static_cast<int64_t>(b) * K + i) * ns + j], K);
    kp_entry(x, K, i, c, p, ox, oy, oz, dist);
    sdist[tid] = dist;
  }
  __syncthreads();
  if (on) {
    T acc = 0;
    for (int q = 0; q < ns; ++q) acc += sdist[il * ns + q];
    const T w = dist / acc;
    float* o = stage + tid * 35;
    o[0] = static_cast<float>(ox);
    o[1] = static_cast<float>(oy);
    o[2] = static_cast<float>(oz);
    // Q4: FE row p, p a key-point-local index
    const float4* f = reinterpret_cast<const float4*>(fe_feat + (static_cast<int64_t>(b) * S + p) * 32);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float4 v = f[q];
      o[3 + 4 * q] = static_cast<float>(static_cast<T>(v.x) * w);
      o[4 + 4 * q] = static_cast<float>(static_cast<T>(v.y) * w);
      o[5 + 4 * q] = static_cast<float>(static_cast<T>(v.z) * w);
      o[6 + 4 * q] = static_cast<float>(static_cast<T>(v.w) * w);
    }
  }
  __syncthreads();
  // the workgroup's rows are one contiguous block of src_cat
  const int n = cnt * ns * 35;
  float* dst = src_cat + (static_cast<int64_t>(b) * K + i0) * ns * 35;
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    float4* d4 = reinterpret_cast<float4*>(dst);
    const float4* s4 = reinterpret_cast<const float4*>(stage);
    for (int v = tid; v < (n >> 2); v += kKsRowThreads) d4[v] = s4[v];
    for (int v = (n & ~3) + tid; v < n; v += kKsRowThreads) dst[v] = stage[v];
  } else {
    for (int v = tid; v < n; v += kKsRowThreads) dst[v] = stage[v];
  }
}

// Backward of step 3's feature product (pointnet2_utils.py:59 gather, get_cat_feat_src.py:50).
template <typename T>
__global__ __launch_bounds__(kKsRowThreads) void kp_rows_bwd_kernel(const T* __restrict__ ws_xyz,
                                                                    const int* __restrict__ ws_fidx,
                                                                    const int* __restrict__ ws_pidx, int S, int K,
                                                                    int ns, const float* __restrict__ grad_cat,
                                                                    float* __restrict__ grad_feat) {
  __shared__ T sdist[kKsRowThreads];
  __shared__ T sw[kKsRowThreads];
  __shared__ int sp[kKsRowThreads];

  const int b = blockIdx.x, i0 = blockIdx.y * kKsRowKp, tid = threadIdx.x;
  const int cnt = K - i0 < kKsRowKp ? K - i0 : kKsRowKp;
  const int il = tid / ns, j = tid - il * ns;
  const bool on = tid < cnt * ns;
  const T* x = ws_xyz + static_cast<int64_t>(b) * 3 * K;
  int p = 0;
  T ox, oy, oz, dist = 0;
  if (on) {
    const int i = i0 + il;
    const int c = kp_clamp(ws_fidx[static_cast<int64_t>(b) * K + i], K);
    p = kp_clamp(ws_pidx[(static_cast<int64_t>(b) * K + i) * ns + j], K);
    kp_entry(x, K, i, c, p, ox, oy, oz, dist);
    sdist[tid] = dist;
  }
  __syncthreads();
  if (on) {
    T acc = 0;
    for (int q = 0; q < ns; ++q) acc += sdist[il * ns + q];
    sw[tid] = dist / acc;
    sp[tid] = p;
  }
  __syncthreads();
  // half-wave h walks key point i0 + h, lane q of it feature column q.  The padded entries repeat
  // the row's first entry: their products are added to its sum, one atomic for all of them.
  const int h = tid >> 5, q = tid & 31;
  if (h >= cnt) return;
  const float* g = grad_cat + (static_cast<int64_t>(b) * K + i0 + h) * ns * 35 + 3 + q;
  float* dF = grad_feat + static_cast<int64_t>(b) * S * 32 + q;
  const int p0 = sp[h * ns];
  float acc0 = static_cast<float>(static_cast<T>(g[0]) * sw[h * ns]);
  for (int e = 1; e < ns; ++e) {
    const int pe = sp[h * ns + e];
    const float v = static_cast<float>(static_cast<T>(g[e * 35]) * sw[h * ns + e]);
    if (pe == p0)
      acc0 += v;
    else if (v != 0.f)
      atomicAdd(dF + static_cast<int64_t>(pe) * 32, v);
  }
  if (acc0 != 0.f) atomicAdd(dF + static_cast<int64_t>(p0) * 32, acc0);
}

template <typename T, int PPL>
static void launch_select(const T* fe_xyz, int S, const int64_t* topk, int B, int K, const int64_t* kstart,
                          const double* R, int64_t r_b, T* keypts, double* moved, T* ws_xyz, int* ws_fidx,
                          hipStream_t st) {
  hipLaunchKernelGGL((kp_select_kernel<T, kKsSelThreads, PPL>), dim3(B), dim3(kKsSelThreads), 0, st, fe_xyz, S, topk,
                     K, kstart, R, r_b, keypts, moved, ws_xyz, ws_fidx);
}

template <typename T>
static int launch_kp_split(const void* fe_xyz, const float* fe_feat, int S, const int64_t* topk, int B, int K,
                           const int64_t* kstart, double radius, int ns, const double* R, int64_t r_b, void* keypts,
                           float* src_cat, double* moved, char* ws, const KpWs& lay, hipStream_t st) {
  const T* X = static_cast<const T*>(fe_xyz);
  T* kp = static_cast<T*>(keypts);
  T* wx = reinterpret_cast<T*>(ws);
  int* wf = reinterpret_cast<int*>(ws + lay.fidx);
  int* wp = reinterpret_cast<int*>(ws + lay.pidx);
  if (K <= kKsSelThreads)
    launch_select<T, 1>(X, S, topk, B, K, kstart, R, r_b, kp, moved, wx, wf, st);
  else if (K <= 2 * kKsSelThreads)
    launch_select<T, 2>(X, S, topk, B, K, kstart, R, r_b, kp, moved, wx, wf, st);
  else
    launch_select<T, 4>(X, S, topk, B, K, kstart, R, r_b, kp, moved, wx, wf, st);
  const T r2 = static_cast<T>(radius * radius);
  hipLaunchKernelGGL((kp_ball_kernel<T>), dim3(B, ceil_div(K, kKsBallWaves)), dim3(kKsBallThreads), 0, st, wx, wf, K,
                     r2, ns, wp);
  hipLaunchKernelGGL((kp_rows_kernel<T>), dim3(B, ceil_div(K, kKsRowKp)), dim3(kKsRowThreads), 0, st, wx, wf, wp,
                     fe_feat, S, K, ns, src_cat);
  return launch_status("dvcp_src_keypoints_ws");
}

}  // namespace dvcp

extern "C" int64_t dvcp_src_keypoints_workspace_bytes(int dtype, int B, int K, int nsample) {
  if (!dvcp::kp_ws_args_ok(dtype, B, K, nsample)) return 0;
  return dvcp::kp_ws_layout(dtype, B, K, nsample).total;
}

extern "C" int dvcp_src_keypoints_ws(int dtype, const void* fe_xyz, const float* fe_feat, int S, const int64_t* topk,
                                     int B, int K, const int64_t* kstart, double radius, int nsample,
                                     const double* R_init, int64_t r_b, void* keypts, float* src_cat, double* moved,
                                     void* workspace, int64_t ws_bytes, void* stream) {
  DVCP_REQUIRE(K > 0 && K <= dvcp::kKsMaxK && K <= S, "dvcp_src_keypoints_ws: K=%d unsupported (1..1024, <= S=%d)", K,
               S);
  DVCP_REQUIRE(nsample > 0 && nsample <= dvcp::kKsMaxNs, "dvcp_src_keypoints_ws: nsample=%d unsupported (1..32)",
               nsample);
  // as dvcp_src_keypoints: the reference's DFE MaxPool1d(32) rejects K < nsample columns
  DVCP_REQUIRE(K >= nsample, "dvcp_src_keypoints_ws: K=%d < nsample=%d", K, nsample);
  DVCP_REQUIRE(dtype == DVCP_F32 || dtype == DVCP_F64, "dvcp_src_keypoints_ws: bad dtype %d", dtype);
  DVCP_REQUIRE(B >= 0, "dvcp_src_keypoints_ws: B=%d unsupported", B);
  if (B == 0) return DVCP_OK;
  DVCP_REQUIRE(fe_xyz && fe_feat && topk && kstart && R_init && keypts && src_cat && moved,
               "dvcp_src_keypoints_ws: null pointer");
  DVCP_REQUIRE((reinterpret_cast<uintptr_t>(fe_feat) & 15) == 0,
               "dvcp_src_keypoints_ws: fe_feat must be 16-byte aligned");
  DVCP_REQUIRE(workspace, "dvcp_src_keypoints_ws: null workspace");
  DVCP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
               "dvcp_src_keypoints_ws: workspace must be 16-byte aligned");
  const dvcp::KpWs lay = dvcp::kp_ws_layout(dtype, B, K, nsample);
  DVCP_REQUIRE(ws_bytes >= lay.total, "dvcp_src_keypoints_ws: workspace of %lld bytes, need %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(lay.total));
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  if (dtype == DVCP_F32)
    return dvcp::launch_kp_split<float>(fe_xyz, fe_feat, S, topk, B, K, kstart, radius, nsample, R_init, r_b, keypts,
                                        src_cat, moved, ws, lay, st);
  return dvcp::launch_kp_split<double>(fe_xyz, fe_feat, S, topk, B, K, kstart, radius, nsample, R_init, r_b, keypts,
                                       src_cat, moved, ws, lay, st);
}

extern "C" int dvcp_src_keypoints_backward_ws(int dtype, const void* workspace, int64_t ws_bytes, int S, int B, int K,
                                              int nsample, const float* grad_cat, float* grad_feat, void* stream) {
  DVCP_REQUIRE(K > 0 && K <= dvcp::kKsMaxK && K <= S && nsample > 0 && nsample <= dvcp::kKsMaxNs && K >= nsample,
               "dvcp_src_keypoints_backward_ws: K=%d nsample=%d unsupported (K 1..1024, <= S=%d, >= nsample <= 32)", K,
               nsample, S);
  DVCP_REQUIRE(dtype == DVCP_F32 || dtype == DVCP_F64, "dvcp_src_keypoints_backward_ws: bad dtype %d", dtype);
  DVCP_REQUIRE(B >= 0, "dvcp_src_keypoints_backward_ws: B=%d unsupported", B);
  if (B == 0) return DVCP_OK;
  DVCP_REQUIRE(grad_cat && grad_feat, "dvcp_src_keypoints_backward_ws: null pointer");
  DVCP_REQUIRE(workspace, "dvcp_src_keypoints_backward_ws: null workspace");
  DVCP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0,
               "dvcp_src_keypoints_backward_ws: workspace must be 16-byte aligned");
  const dvcp::KpWs lay = dvcp::kp_ws_layout(dtype, B, K, nsample);
  DVCP_REQUIRE(ws_bytes >= lay.total, "dvcp_src_keypoints_backward_ws: workspace of %lld bytes, need %lld",
               static_cast<long long>(ws_bytes), static_cast<long long>(lay.total));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const char* ws = static_cast<const char*>(workspace);
  const int* wf = reinterpret_cast<const int*>(ws + lay.fidx);
  const int* wp = reinterpret_cast<const int*>(ws + lay.pidx);
  const dim3 grid(B, dvcp::ceil_div(K, dvcp::kKsRowKp));
  if (dtype == DVCP_F32)
    hipLaunchKernelGGL((dvcp::kp_rows_bwd_kernel<float>), grid, dim3(dvcp::kKsRowThreads), 0, st,
                       reinterpret_cast<const float*>(ws), wf, wp, S, K, nsample, grad_cat, grad_feat);
  else
    hipLaunchKernelGGL((dvcp::kp_rows_bwd_kernel<double>), grid, dim3(dvcp::kKsRowThreads), 0, st,
                       reinterpret_cast<const double*>(ws), wf, wp, S, K, nsample, grad_cat, grad_feat);
  return dvcp::launch_status("dvcp_src_keypoints_backward_ws");
}
