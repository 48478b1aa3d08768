// fold.hip -- the sum of partial rows: out[e] = sum_k part[k][e] in fp64, in a fixed order, rounded
// once to the output type.  Every backward and statistics pass writes one partial row per workgroup
// (or per wave, or per key point) and ends with one of the two folds below; no atomics, so two
// identical calls give identical bits.
//
//   fold_rows         one element per thread, k ascending: a few hundred rows at the most.
//   fold_rows_sliced  64 columns x 16 slices per workgroup for thousands of rows: slice s sums rows
//                     s, s + 16, ...; the slices are then added in order 0..15.
//
// The launchers only enqueue; the caller checks launch_status() under its own name.
#include "common.h"

namespace dvcp {

namespace {

template <typename PT, typename OT>
__global__ __launch_bounds__(256) void fold_rows_kernel(const PT* __restrict__ part, int nrows, int row_stride,
                                                        int ncols, OT* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ncols) return;
  double acc = 0.0;
  for (int k = 0; k < nrows; ++k) acc += static_cast<double>(part[static_cast<int64_t>(k) * row_stride + e]);
  out[e] = static_cast<OT>(acc);
}

template <typename PT, typename OT>
__global__ __launch_bounds__(1024) void fold_rows_sliced_kernel(const PT* __restrict__ part, int nrows, int ncols,
                                                                OT* __restrict__ out) {
  __shared__ double sl[16][64];
  const int tid = threadIdx.x, c = tid & 63, slice = tid >> 6;
  const int e = blockIdx.x * 64 + c;
  double acc = 0.0;
  if (e < ncols)
    for (int k = slice; k < nrows; k += 16) acc += static_cast<double>(part[static_cast<int64_t>(k) * ncols + e]);
  sl[slice][c] = acc;
  __syncthreads();
  if (tid < 64 && e < ncols) {
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t += sl[k][c];
    out[e] = static_cast<OT>(t);
  }
}

}  // namespace

template <typename PT, typename OT>
void fold_rows(const PT* part, int nrows, int row_stride, int ncols, OT* out, hipStream_t st) {
  hipLaunchKernelGGL((fold_rows_kernel<PT, OT>), dim3(ceil_div(ncols, 256)), dim3(256), 0, st, part, nrows, row_stride,
                     ncols, out);
}

template <typename PT, typename OT>
void fold_rows_sliced(const PT* part, int nrows, int ncols, OT* out, hipStream_t st) {
  hipLaunchKernelGGL((fold_rows_sliced_kernel<PT, OT>), dim3(ceil_div(ncols, 64)), dim3(1024), 0, st, part, nrows,
                     ncols, out);
}

// the type pairs in use
template void fold_rows<float, float>(const float*, int, int, int, float*, hipStream_t);
template void fold_rows<double, double>(const double*, int, int, int, double*, hipStream_t);
template void fold_rows_sliced<float, float>(const float*, int, int, float*, hipStream_t);
template void fold_rows_sliced<float, double>(const float*, int, int, double*, hipStream_t);
template void fold_rows_sliced<double, double>(const double*, int, int, double*, hipStream_t);
template void fold_rows_sliced<double, float>(const double*, int, int, float*, hipStream_t);

}  // namespace dvcp
