// knn_tiled_slabs.hip -- exact kNN for more reference points than the tiled kernels take
// (M > kMaxTiles * kTile = 16384): dvcp_knn_slabs.  Same contract as dvcp_knn / dvcp_knn_tiled.
//
// The reference is cut into S = ceil(M / 16384) slabs that are contiguous in index, each
// L = round_up(ceil(M / S), 16) points long (the last one shorter).  The tuned tiled kernels run
// once per slab, unchanged (knn_tiled_build + knn_sel_launch / knn_insert_launch on the reference
// pointer advanced by j * L points, serially on the stream in one tiled workspace), and write the
// slab's sorted k-list of slab-local indices.  knn_slab_fold_kernel then folds that list into a
// running list per query, one lane per query:
//   * the running list is k packed keys d2_bits << 32 | global index (global = local + j * L); d2
//     is finite and non-negative, so keys order like (d2, index) and the order is total: ties go to
//     the lower index across slabs as inside one, and the union of the slabs' top-k lists holds the
//     global top k;
//   * the fold orders by d2, never by dist: sqrt_rn maps distinct d2 to one dist (1 and 1 + 2^-23
//     both give 1.0f), so a (dist, index) order would not be the (d2, index) order.  The slab
//     kernels return dist only, so d2 is recomputed from the coordinates with the scan's exact
//     form (inputs cast to fp32, dx = ref - query, (dx*dx + dy*dy) + dz*dz, no fma) from
//     (x, y, z, 0) rows of the fp32 reference packed once per call;
//   * C[i] = min(run[i], new[KT - 1 - i]) of two ascending KT-lists is bitonic and holds the KT
//     smallest keys; one KT-key bitonic merge sorts it.  Static register indices only.  Slots at or
//     above k hold the all-ones key; a slab's padding entry (inf, -1) becomes (+inf bits, 0xFFFFFFFF),
//     stays behind every real key and comes out as (inf, -1);
//   * the fold of the last slab writes dist = sqrt_rn(d2), idx and idx64 instead of the keys.  The
//     first fold never reads the running keys, so the workspace needs no initialisation.
//
// Workspace (dvcp_knn_slabs_workspace_bytes), each part rounded up to 256 bytes; it does not grow
// with the slab count:
//   dvcp_knn_tiled_workspace_bytes(B, L, Q)   the tiled workspace of one slab (L <= 16384)
//   4 * B * Q * k                             one slab's indices
//   8 * B * Q * k                             the running keys, slot-major (B x k x Q)
//   16 * B * M                                the packed fp32 reference
#include "knn_tiled_common.h"

namespace dvcp {

constexpr int kSlabPoints = kMaxTiles * kTile;  // the tiled kernels' largest M
constexpr int kSlabsMaxM = 1 << 20;             // 64 slabs; global indices stay far below 2^31
constexpr int kFoldThreads = 256;

struct SlabGeom {
  int n, len;  // slabs, points per slab (the last: M - (n - 1) * len, in 1..len)
};
inline SlabGeom slab_geom(int M) {
  const int n = M > kSlabPoints ? ceil_div(M, kSlabPoints) : 1;
  return {n, ceil_div(ceil_div(M, n), kTile) * kTile};
}

struct SlabLayout {
  int32_t* sidx;   // B x Q x k: the current slab's indices
  uint64_t* run;   // B x k x Q: the running keys
  float4* pts;     // B x M: (x, y, z, 0) fp32
};
inline SlabLayout slab_layout(void* ws, int B, int M, int Q, int k, int len) {
  char* p = static_cast<char*>(ws) + align256(dvcp_knn_tiled_workspace_bytes(B, len, Q));
  SlabLayout S;
  S.sidx = reinterpret_cast<int32_t*>(p);
  p += align256(4 * int64_t(B) * Q * k);
  S.run = reinterpret_cast<uint64_t*>(p);
  p += align256(8 * int64_t(B) * Q * k);
  S.pts = reinterpret_cast<float4*>(p);
  return S;
}

template <typename CT>
__global__ __launch_bounds__(256) void knn_slab_pack_kernel(PointsView<CT> ref, int M, int B, float4* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= static_cast<int64_t>(B) * M) return;
  const int b = static_cast<int>(i / M);
  const int64_t n = i - static_cast<int64_t>(b) * M;
  out[i] = make_float4(static_cast<float>(ref.at(b, 0, n)), static_cast<float>(ref.at(b, 1, n)),
                       static_cast<float>(ref.at(b, 2, n)), 0.0f);  // knn_cuda's .float()
}

// KT: list length in registers (16 for k <= 16, else 32).  base = j * L, the slab's first index.
template <typename CT, int KT>
__global__ __launch_bounds__(kFoldThreads) void knn_slab_fold_kernel(const float4* __restrict__ pts, int M,
                                                                     PointsView<CT> qry, int Q, int k, int base,
                                                                     const int32_t* __restrict__ sidx,
                                                                     uint64_t* __restrict__ run, int first, int last,
                                                                     float* __restrict__ dist, int32_t* __restrict__ idx,
                                                                     int64_t* __restrict__ idx64) {
  const int b = blockIdx.y;
  const int q = blockIdx.x * kFoldThreads + threadIdx.x;
  if (q >= Q) return;
  const float qx = static_cast<float>(qry.at(b, 0, q)), qy = static_cast<float>(qry.at(b, 1, q)),
              qz = static_cast<float>(qry.at(b, 2, q));
  const float4* pb = pts + static_cast<int64_t>(b) * M;
  const int64_t o = (static_cast<int64_t>(b) * Q + q) * k;
  uint64_t* rq = run + static_cast<int64_t>(b) * k * Q + q;
  uint64_t c[KT];
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    const int t = KT - 1 - i;  // the slab's list, reversed
    uint64_t nk = ~0ull;
    if (t < k) {
      const int li = sidx[o + t];
      if (li >= 0) {
        const uint32_t gi = static_cast<uint32_t>(base + li);
        const float4 p = pb[gi];
        const float dx = p.x - qx, dy = p.y - qy, dz = p.z - qz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        nk = (static_cast<uint64_t>(__float_as_uint(d2)) << 32) | gi;
      } else {
        nk = (static_cast<uint64_t>(0x7F800000u) << 32) | 0xFFFFFFFFull;  // padding: (inf, -1)
      }
    }
    const uint64_t rk = (!first && i < k) ? rq[static_cast<int64_t>(i) * Q] : ~0ull;
    c[i] = rk < nk ? rk : nk;
  }
#pragma unroll
  for (int s = KT / 2; s > 0; s >>= 1) {
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      if ((i & s) == 0) {
        const uint64_t lo = c[i] < c[i | s] ? c[i] : c[i | s];
        const uint64_t hi = c[i] < c[i | s] ? c[i | s] : c[i];
        c[i] = lo;
        c[i | s] = hi;
      }
    }
  }
  if (!last) {
#pragma unroll
    for (int i = 0; i < KT; ++i)
      if (i < k) rq[static_cast<int64_t>(i) * Q] = c[i];
    return;
  }
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    if (i < k) {
      const int gi = static_cast<int>(static_cast<uint32_t>(c[i]));  // 0xFFFFFFFF -> -1
      if (dist) dist[o + i] = sqrt_rn(__uint_as_float(static_cast<uint32_t>(c[i] >> 32)));
      if (idx) idx[o + i] = gi;
      if (idx64) idx64[o + i] = gi;
    }
  }
}

template <typename CT>
static int knn_slabs_run(const void* ref, int64_t rb, int64_t rc, int64_t rn, int M, const void* qry, int64_t qb,
                         int64_t qc, int64_t qn, int Q, int B, int k, void* workspace, float* dist, int32_t* idx,
                         int64_t* idx64, hipStream_t st) {
  constexpr int dtype = sizeof(CT) == 4 ? DVCP_F32 : DVCP_F64;
  const SlabGeom g = slab_geom(M);
  const SlabLayout S = slab_layout(workspace, B, M, Q, k, g.len);
  const PointsView<CT> rv{static_cast<const CT*>(ref), rb, rc, rn}, qv{static_cast<const CT*>(qry), qb, qc, qn};
  const int64_t total = static_cast<int64_t>(B) * M;
  hipLaunchKernelGGL((knn_slab_pack_kernel<CT>), dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, st, rv,
                     M, B, S.pts);
  if (int e = launch_status("dvcp_knn_slabs(pack)")) return e;
  const dim3 fgrid(ceil_div(Q, kFoldThreads), B);
  for (int j = 0; j < g.n; ++j) {
    const int base = j * g.len, Mj = (M - base < g.len) ? M - base : g.len;
    const CT* rj = static_cast<const CT*>(ref) + static_cast<int64_t>(base) * rn;
    const TiledLayout L = tiled_layout(workspace, B, Mj, Q);
    if (int e = knn_tiled_build(dtype, rj, rb, rc, rn, Mj, qry, qb, qc, qn, Q, B, L, st)) return e;
    if (int e = k > 16 ? knn_sel_launch(L, Mj, Q, B, k, nullptr, S.sidx, nullptr, st)
                       : knn_insert_launch(L, Mj, Q, B, k, nullptr, S.sidx, nullptr, st))
      return e;
    const int first = j == 0, last = j == g.n - 1;
    if (k > 16)
      hipLaunchKernelGGL((knn_slab_fold_kernel<CT, 32>), fgrid, dim3(kFoldThreads), 0, st, S.pts, M, qv, Q, k, base,
                         S.sidx, S.run, first, last, dist, idx, idx64);
    else
      hipLaunchKernelGGL((knn_slab_fold_kernel<CT, 16>), fgrid, dim3(kFoldThreads), 0, st, S.pts, M, qv, Q, k, base,
                         S.sidx, S.run, first, last, dist, idx, idx64);
    if (int e = launch_status("dvcp_knn_slabs(fold)")) return e;
  }
  return DVCP_OK;
}

}  // namespace dvcp

extern "C" int64_t dvcp_knn_slabs_workspace_bytes(int B, int M, int Q, int k) {
  if (B < 0 || M < 0 || Q < 0 || k < 0 || M > dvcp::kSlabsMaxM) return -1;
  const int len = dvcp::slab_geom(M > 0 ? M : 1).len;
  return dvcp::align256(dvcp_knn_tiled_workspace_bytes(B, len, Q)) + dvcp::align256(4 * int64_t(B) * Q * k) +
         dvcp::align256(8 * int64_t(B) * Q * k) + dvcp::align256(16 * int64_t(B) * M);
}

extern "C" int dvcp_knn_slabs(int dtype, const void* ref, int64_t rb, int64_t rc, int64_t rn, int M, const void* qry,
                              int64_t qb, int64_t qc, int64_t qn, int Q, int B, int k, void* workspace, float* dist,
                              int32_t* idx, int64_t* idx64, void* stream) {
  DVCP_REQUIRE(ref && qry && workspace, "dvcp_knn_slabs: null pointer");
  DVCP_REQUIRE(k > 0 && k <= 32 && M >= 1 && Q >= 0 && B >= 0 && B <= 65535, "dvcp_knn_slabs: bad sizes");
  DVCP_REQUIRE(M <= dvcp::kSlabsMaxM, "dvcp_knn_slabs: M=%d exceeds %d", M, dvcp::kSlabsMaxM);
  DVCP_REQUIRE(dtype == DVCP_F32 || dtype == DVCP_F64, "dvcp_knn_slabs: bad dtype %d", dtype);
  DVCP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "dvcp_knn_slabs: workspace must be 16-byte aligned");
  if (B == 0 || Q == 0) return DVCP_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return dtype == DVCP_F32
             ? dvcp::knn_slabs_run<float>(ref, rb, rc, rn, M, qry, qb, qc, qn, Q, B, k, workspace, dist, idx, idx64, st)
             : dvcp::knn_slabs_run<double>(ref, rb, rc, rn, M, qry, qb, qc, qn, Q, B, k, workspace, dist, idx, idx64, st);
}
