// rigid_svd.h -- the 3x3 SVD of the pose solve (rigid.hip), host + device so that a host-only
// program can check it without a GPU (tests/test_rigid_svd_host.py).  Plain C++, fp64, no HIP
// calls; compile with -ffp-contract=off like every translation unit of the library.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define DVCP_HOST_DEVICE __host__ __device__
#else
#define DVCP_HOST_DEVICE
#endif

namespace dvcp {

// One-sided Jacobi SVD of H (3x3): H V = U diag(sig), i.e. H = U diag(sig) V^T.  Returns R = V U^T
// and U, sig (the backward needs them).  V is a product of plane rotations (det V = +1).
//
// Rank-deficient H (singular directions with sig <= 1e-14 sig_max): U is completed to an
// orthonormal basis with det U = +1, so R is a proper rotation that is optimal on the range of H
// (tr(R H) = sum sig) and arbitrary off it.  sig stays as computed.
//   two good columns: the third is their cross product;
//   one good column u: the coordinate axis least aligned with u, orthogonalised against u, and the
//     cross product of the two;
//   none (H = 0, no rotation happened, V = I): U = I and R = I, which is what torch.svd gives.
DVCP_HOST_DEVICE inline void kabsch_svd(const double (&H)[3][3], double (&R)[3][3], double (&U)[3][3],
                                        double (&sig)[3]) {
  double A[3][3], V[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      A[i][j] = H[i][j];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool rotated = false;
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      double alpha = 0, beta = 0, gamma = 0;
      for (int i = 0; i < 3; ++i) {
        alpha += A[i][p] * A[i][p];
        beta += A[i][q] * A[i][q];
        gamma += A[i][p] * A[i][q];
      }
      if (fabs(gamma) <= 1e-300 || fabs(gamma) <= 1e-17 * sqrt(alpha * beta)) continue;
      rotated = true;
      const double zeta = (beta - alpha) / (2.0 * gamma);
      const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
      for (int i = 0; i < 3; ++i) {
        const double ap = A[i][p], aq = A[i][q];
        A[i][p] = c * ap - s * aq;
        A[i][q] = s * ap + c * aq;
        const double vp = V[i][p], vq = V[i][q];
        V[i][p] = c * vp - s * vq;
        V[i][q] = s * vp + c * vq;
      }
    }
    if (!rotated) break;
  }
  for (int j = 0; j < 3; ++j) sig[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
  const double smax = fmax(sig[0], fmax(sig[1], sig[2]));
  int bad = -1, good = -1, ngood = 0;
  for (int j = 0; j < 3; ++j) {
    if (sig[j] > 1e-14 * smax && sig[j] > 0) {
      for (int i = 0; i < 3; ++i) U[i][j] = A[i][j] / sig[j];
      good = j;
      ++ngood;
    } else {
      bad = j;
    }
  }
  if (ngood == 2) {  // rank 2: complete U with the cross product of the other columns
    const int a = (bad + 1) % 3, b = (bad + 2) % 3;
    U[0][bad] = U[1][a] * U[2][b] - U[2][a] * U[1][b];
    U[1][bad] = U[2][a] * U[0][b] - U[0][a] * U[2][b];
    U[2][bad] = U[0][a] * U[1][b] - U[1][a] * U[0][b];
  } else if (ngood == 1) {  // rank 1: columns (good, a, b) = (u, e, u x e), det U = +1
    const int a = (good + 1) % 3, b = (good + 2) % 3;
    const double u[3] = {U[0][good], U[1][good], U[2][good]};
    int k = 0;
    for (int i = 1; i < 3; ++i) k = fabs(u[i]) < fabs(u[k]) ? i : k;
    double e[3];
    for (int i = 0; i < 3; ++i) e[i] = (i == k ? 1.0 : 0.0) - u[k] * u[i];
    const double en = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);  // >= sqrt(2/3): |u_k| <= 1/sqrt(3)
    for (int i = 0; i < 3; ++i) U[i][a] = e[i] / en;
    U[0][b] = u[1] * U[2][a] - u[2] * U[1][a];
    U[1][b] = u[2] * U[0][a] - u[0] * U[2][a];
    U[2][b] = u[0] * U[1][a] - u[1] * U[0][a];
  } else if (ngood == 0) {  // H = 0 (or not finite: V carries the NaN into R)
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) U[i][j] = i == j ? 1.0 : 0.0;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = V[i][0] * U[j][0] + V[i][1] * U[j][1] + V[i][2] * U[j][2];
}

}  // namespace dvcp
