// k_multi.hip -- the generic path of spmv_execute_multi (Y = A X, K
// interleaved right-hand sides: x_j[i] = X[i*ldx + j], y_j[r] = Y[r*ldy + j]):
// the strided column copies around the plan's own single-vector kernels, and
// the zero fill of a plan with nothing stored.
//
// The fused kernels (DIA, sliced ELL / JDS; K = 2, 4, 8) are the K-templated
// bodies of k_dia.hip and k_ell.hip.  capi.cpp's multi_cut decides which
// columns take which path.
#include "device.hpp"
#include "internal.hpp"

namespace spmv {

// the k used columns of every row of Y = 0 (a plan with nothing stored)
__global__ __launch_bounds__(256) void multi_zero_kernel(int64_t m, int32_t k, double *__restrict__ Y, int64_t ldy) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m * k) return;
    const int64_t r = i / k;
    Y[r * ldy + (i - r * k)] = 0.0;
}

int launch_multi_zero(const spmv_plan_s *p, int32_t k, double *Y, int64_t ldy) {
    const int64_t total = p->m * k;
    if (total == 0) return SPMV_SUCCESS;
    hipLaunchKernelGGL(multi_zero_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, p->stream, p->m, k, Y,
                       ldy);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

// one column through the plan's own kernels: dst[i*dst_ld] = src[i*src_ld],
// ld = 1 on the contiguous side
__global__ __launch_bounds__(256) void multi_copy_kernel(int64_t len, const double *__restrict__ src, int64_t src_ld,
                                                         double *__restrict__ dst, int64_t dst_ld) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len) dst[i * dst_ld] = src[i * src_ld];
}

int launch_multi_copy(const spmv_plan_s *p, int64_t len, const double *src, int64_t src_ld, double *dst,
                      int64_t dst_ld) {
    if (len == 0) return SPMV_SUCCESS;
    hipLaunchKernelGGL(multi_copy_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, p->stream, len, src,
                       src_ld, dst, dst_ld);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

}  // namespace spmv
