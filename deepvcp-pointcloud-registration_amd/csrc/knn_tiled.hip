// knn_tiled.hip -- exact kNN over spatially sorted reference tiles (replaces knn_cuda.KNN at
// get_cat_feat_tgt.py:45,52; same contract as dvcp_knn in knn.hip: fp32 d2 = (dx*dx + dy*dy) +
// dz*dz with dx = ref - query, ascending, ties to the lower index, dist = correctly rounded sqrt).
// This unit: the workspace size, the dispatch and the entry points (knn_tiled_common.h lists the
// other units).
//
// Why: the brute-force scan meets reference points in index order, so a lane keeps inserting into
// its sorted top-32 and the wave executes the 32-deep insertion network on almost every point.
// Here both sets are sorted by a 12-bit Morton cell, references into 16-point tiles with boxes.
// Each wave takes 64 Morton-consecutive queries (a compact box), orders the tiles by the lower
// bound of the distance between its query box and each tile box (k <= 16: a bitonic sort; k > 16:
// a counting sort into buckets of the bound, knn_wave_order), and scans tiles nearest first:
//   * tile data is wave-uniform, so points come through the scalar cache as SGPR operands;
//   * a tile is skipped when no lane's own lower bound reaches its current k-th distance;
//   * the scan stops when the next tile's bound exceeds every lane's k-th distance.
// Exactness: round-to-nearest is monotone, so a bound computed from box faces with the same
// float ops never exceeds the computed d2 of any point in the box; tiles are dropped only when the
// bound is strictly above the k-th distance, so every point that could enter or tie the top k is
// examined, and insertion orders by (d2, index) explicitly.
#include "knn_tiled_common.h"

extern "C" int64_t dvcp_knn_tiled_workspace_bytes(int B, int M, int Q) {
  if (B < 0 || M < 0 || Q < 0) return -1;
  const int64_t T = dvcp::ceil_div(M, dvcp::kTile);
  return dvcp::align256(16 * int64_t(B) * T * dvcp::kTile) + dvcp::align256(32 * int64_t(B) * T) +
         dvcp::align256(16 * int64_t(B) * Q) + dvcp::align256(dvcp::tiled_zeroed_bytes(B));
}

static int knn_tiled_impl(int dtype, const void* ref, int64_t rb, int64_t rc, int64_t rn, int M, const void* qry,
                          int64_t qb, int64_t qc, int64_t qn, int Q, int B, int k, void* workspace, float* dist,
                          int32_t* idx, int64_t* idx64, void* stream, bool insertion) {
  DVCP_REQUIRE(ref && qry && workspace, "dvcp_knn_tiled: null pointer");
  DVCP_REQUIRE(k > 0 && k <= 32 && M >= 0 && Q >= 0 && B >= 0 && B <= 65535, "dvcp_knn_tiled: bad sizes");
  DVCP_REQUIRE(M <= dvcp::kMaxTiles * dvcp::kTile, "dvcp_knn_tiled: M=%d > %d", M, dvcp::kMaxTiles * dvcp::kTile);
  DVCP_REQUIRE(dtype == DVCP_F32 || dtype == DVCP_F64, "dvcp_knn_tiled: bad dtype %d", dtype);
  if (B == 0 || Q == 0) return DVCP_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dvcp::TiledLayout L = dvcp::tiled_layout(workspace, B, M, Q);
  if (int e = dvcp::knn_tiled_build(dtype, ref, rb, rc, rn, M, qry, qb, qc, qn, Q, B, L, st)) return e;
  // k = 17..32 (the forward's 32): the buffered-selection kernel; k <= 16: per-candidate insertion
  return k > 16 && !insertion ? dvcp::knn_sel_launch(L, M, Q, B, k, dist, idx, idx64, st)
                              : dvcp::knn_insert_launch(L, M, Q, B, k, dist, idx, idx64, st);
}

extern "C" int dvcp_knn_tiled(int dtype, const void* ref, int64_t rb, int64_t rc, int64_t rn, int M, const void* qry,
                              int64_t qb, int64_t qc, int64_t qn, int Q, int B, int k, void* workspace, float* dist,
                              int32_t* idx, int64_t* idx64, void* stream) {
  return knn_tiled_impl(dtype, ref, rb, rc, rn, M, qry, qb, qc, qn, Q, B, k, workspace, dist, idx, idx64, stream, false);
}

// The same tiled scan with the per-candidate insertion network for every k (the round-2 kernel):
// kept as a second exact implementation for the parity tests and A/B timing.
extern "C" int dvcp_knn_tiled_insert(int dtype, const void* ref, int64_t rb, int64_t rc, int64_t rn, int M,
                                     const void* qry, int64_t qb, int64_t qc, int64_t qn, int Q, int B, int k,
                                     void* workspace, float* dist, int32_t* idx, int64_t* idx64, void* stream) {
  return knn_tiled_impl(dtype, ref, rb, rc, rn, M, qry, qb, qc, qn, Q, B, k, workspace, dist, idx, idx64, stream, true);
}

// Test hook: the wave box, certified bound and tile order that dvcp_knn_tiled's k = 17..32 kernel
// computes for every wave of 64 curve-ordered queries (see include/dvcp.h).
extern "C" int dvcp_knn_tiled_order_probe(int dtype, const void* ref, int64_t rb, int64_t rc, int64_t rn, int M,
                                          const void* qry, int64_t qb, int64_t qc, int64_t qn, int Q, int B,
                                          void* workspace, int32_t* info, int32_t* order, float* lb,
                                          int32_t* bucket, void* stream) {
  DVCP_REQUIRE(ref && qry && workspace && info && order && lb && bucket, "dvcp_knn_tiled_order_probe: null pointer");
  DVCP_REQUIRE(M > 0 && Q > 0 && B > 0 && B <= 65535, "dvcp_knn_tiled_order_probe: bad sizes");
  DVCP_REQUIRE(M <= dvcp::kMaxTiles * dvcp::kTile, "dvcp_knn_tiled_order_probe: M=%d > %d", M,
               dvcp::kMaxTiles * dvcp::kTile);
  DVCP_REQUIRE(dtype == DVCP_F32 || dtype == DVCP_F64, "dvcp_knn_tiled_order_probe: bad dtype %d", dtype);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dvcp::TiledLayout L = dvcp::tiled_layout(workspace, B, M, Q);
  if (int e = dvcp::knn_tiled_build(dtype, ref, rb, rc, rn, M, qry, qb, qc, qn, Q, B, L, st)) return e;
  return dvcp::knn_order_probe_launch(L, M, Q, B, info, order, lb, bucket, st);
}
