// cpg_tiled.h -- what the tiled CPG's forward (cpg_tiled.hip) and backward (cpg_tiled_bwd.hip)
// share: the block geometry, FastDiv's host-side multipliers and the forward's launches for one
// chunk of key points, which the backward repeats to recompute h1 and the logits.
#pragma once
#include "common.h"
#include "cpg_grid.h"

namespace dvcp {

constexpr int kCtThreads = 1024;                 // 16 waves: LDS allows one workgroup per CU
constexpr int kCtMaxG = 32;
// Workspace cap: key points are walked in chunks whose workspace fits 256 MiB (41 key points at
// G = 32, 147 at G = 21: over a thousand conv1 workgroups per launch either way).
constexpr int64_t kCtWsCap = int64_t(256) << 20;

__host__ __device__ inline int ct_blocks(int G, int edge) { return (G + edge - 1) / edge; }
__host__ __device__ inline int ct_block_size(int G, int nb) { return (G + nb - 1) / nb; }
inline int64_t ct_ws_per_point(int G) { return int64_t(49) * G * G * G * 4; }

// FastDiv's multipliers for every row length and plane size a launch's blocks can have, formed on
// the host (in the kernel each would be a 64-bit division per thread).  An axis has two extents,
// e[0] = bs and the last block's e[1] = G - (nb - 1) bs; with a halo of h cells on each side
// (h = 0, 1, 2) a row is e[xl] + 2 h cells long and a plane (e[xl] + 2 h)(e[yl] + 2 h).
struct CtMagic {
  uint32_t row[3][2], plane[3][2][2];
};
inline CtMagic ct_magic(int G, int nb, int bs) {
  const int e[2] = {bs, G - (nb - 1) * bs};
  CtMagic k;
  for (int h = 0; h < 3; ++h)
    for (int xl = 0; xl < 2; ++xl) {
      k.row[h][xl] = FastDiv::magic(e[xl] + 2 * h);
      for (int yl = 0; yl < 2; ++yl) k.plane[h][xl][yl] = FastDiv::magic((e[xl] + 2 * h) * (e[yl] + 2 * h));
    }
  return k;
}

// The block's origin and extent along each axis (x fastest), from its index in the nb^3 blocks
struct CtBlock {
  int ox, oy, oz, bx, by, bz;
  int xl, yl;  // the block is the last one along x, y (CtMagic's indices)
  // division by the block's row length and plane size with a halo of h cells
  __device__ __forceinline__ FastDiv row(const CtMagic& k, int h) const { return FastDiv(k.row[h][xl], bx + 2 * h); }
  __device__ __forceinline__ FastDiv plane(const CtMagic& k, int h) const {
    return FastDiv(k.plane[h][xl][yl], (bx + 2 * h) * (by + 2 * h));
  }
  __device__ __forceinline__ CtBlock(int blk, int G, int nb, int bs) {
    const int iz = blk / (nb * nb), r = blk - iz * nb * nb, iy = r / nb, ix = r - iy * nb;
    xl = ix == nb - 1;
    yl = iy == nb - 1;
    ox = ix * bs;
    oy = iy * bs;
    oz = iz * bs;
    bx = min(bs, G - ox);
    by = min(bs, G - oy);
    bz = min(bs, G - oz);
  }
};

// The forward's launches for np key points (cpg_tiled.hip): the target blocks into Q11 order
// (`order`, np x 32 C; skipped when the tensor already is in that order), conv1 -> h1 (np x C x 16),
// conv2 + conv3 -> logit (np x C) and, when vcp is given, the softmax and the weighted mean.
// Returns the key points' target blocks in Q11 order and sets *tl_p to their distance in floats.
const float* ct_forward_chunk(const float* src, const float* tgt, int64_t t_p, int64_t t_f, int64_t t_c,
                              const float* cand, int np, int G, const float* params, float* h1, float* logit,
                              float* order, float* vcp, float* weight, int64_t* tl_p, hipStream_t s);

}  // namespace dvcp
