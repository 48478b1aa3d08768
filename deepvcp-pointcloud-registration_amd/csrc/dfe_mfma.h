// dfe_mfma.h -- what the units of the target-side deep feature embedding on the matrix cores share
// (get_cat_feat_tgt.py:54-96 fused with deep_feat_embedding.py:47-60).
//   dfe_tgt.hip          the collapsed kernel (default), the launcher, dvcp_dfe_tgt_f16
//   dfe_tgt_literal.hip  the layer-by-layer kernel (dvcp_dfe_tgt_literal)
//   points_pack4.hip     the (x, y, z, 0) row layout the collapsed kernel gathers fastest
//   dfe.hip              dvcp_dfe_tgt / dvcp_dfe_tgt_literal (and the row-per-thread kernels)
//
// Per candidate the 32 neighbour rows go through three 32-wide linear layers (35->32->32->32, no
// nonlinearity, Q14) and a max over the rows, one wave per candidate.  Everything before the GEMMs
// is the reference's arithmetic as in dfe_tgt_kernel (dfe.hip): dist_sum in fp64 summed in
// neighbour order, w = dist / dist_sum in fp64, coordinates differenced in the point dtype.
#pragma once
#include "common.h"

namespace dvcp {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kDfeMfmaWaves = 4;  // candidates (waves) per workgroup

// FT: the feature table's element type -- float, or _Float16 (the C5 "fp16 features" storage, the
// collapsed kernel only).  literal = false: the three linear layers collapsed into one map
// (default); true: fc1, fc2, fc3 evaluated one after the other (float only).
// Instantiated in dfe_tgt.hip for T = float, double and FT = float, _Float16.
template <typename T, typename FT>
int launch_dfe_tgt_mfma(PointsView<T> ref, const FT* feat, int M, const float* cand, const float* dist,
                        const int32_t* idx, int B, int Q, const float* params, float* out, bool literal,
                        hipStream_t st);

// dfe_tgt_literal.hip: enqueues the literal kernel for `need` workgroups' worth of candidates.
template <typename T>
void dfe_tgt_literal_launch(int64_t need, hipStream_t st, PointsView<T> ref, const float* feat, int M,
                            const float* cand, const float* dist, const int32_t* idx, int Q, int B,
                            const float* params, float* out);

}  // namespace dvcp
