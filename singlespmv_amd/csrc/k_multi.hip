// k_multi.hip -- the generic path of spmv_execute_multi (Y = A X, K
// interleaved right-hand sides: x_j[i] = X[i*ldx + j], y_j[r] = Y[r*ldy + j]):
// the strided column copies around the plan's own single-vector kernels, and
// the zero fill of a plan with nothing stored.
//
// The fused kernels (DIA, sliced ELL / JDS; K = 2, 4, 8) are the K-templated
// bodies of k_dia.hip and k_ell.hip.  capi_execute.cpp's multi_cut decides which
// columns take which path.
#include "build_util.hpp"
#include "device.hpp"
#include "internal.hpp"

namespace spmv {

// Both kernels run a grid-stride loop on a capped grid (grid_for).  One thread
// per element asks for 2^32 work-items and more from m * k = 2^32 on (m >= 2^29
// at k = 8); HIP takes the count modulo 2^32 and reports success, and all but
// the first (m * k) mod 2^32 elements kept what they held
// (tests/test_gpu_tall_y.py test_tall_multi_zero).

// the k used columns of every row of Y = 0 (a plan with nothing stored)
__global__ __launch_bounds__(256) void multi_zero_kernel(int64_t m, int32_t k, double *__restrict__ Y, int64_t ldy) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m * k; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / k;
        Y[r * ldy + (i - r * k)] = 0.0;
    }
}

int launch_multi_zero(const spmv_plan_s *p, int32_t k, double *Y, int64_t ldy) {
    const int64_t total = p->m * k;
    if (total == 0) return SPMV_SUCCESS;
    hipLaunchKernelGGL(multi_zero_kernel, dim3(grid_for(total)), dim3(256), 0, p->stream, p->m, k, Y, ldy);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

// one column through the plan's own kernels: dst[i*dst_ld] = src[i*src_ld],
// ld = 1 on the contiguous side
__global__ __launch_bounds__(256) void multi_copy_kernel(int64_t len, const double *__restrict__ src, int64_t src_ld,
                                                         double *__restrict__ dst, int64_t dst_ld) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x)
        dst[i * dst_ld] = src[i * src_ld];
}

int launch_multi_copy(const spmv_plan_s *p, int64_t len, const double *src, int64_t src_ld, double *dst,
                      int64_t dst_ld) {
    if (len == 0) return SPMV_SUCCESS;
    hipLaunchKernelGGL(multi_copy_kernel, dim3(grid_for(len)), dim3(256), 0, p->stream, len, src, src_ld, dst,
                       dst_ld);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

}  // namespace spmv
