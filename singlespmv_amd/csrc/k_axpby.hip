// k_axpby.hip -- the second pass of spmv_execute_axpby's generic path:
// y = alpha * t + beta * y over m rows, t = the row sums the plan's own
// kernels wrote into the plan's scratch (capi_execute.cpp axpby_dispatch).  The fused
// path -- the same arithmetic in the store epilogue of the one-writer-per-row
// kernels -- lives in k_csr.hip, k_ell.hip and k_dia.hip.
#include "build_util.hpp"
#include "device.hpp"
#include "internal.hpp"

namespace spmv {

// Row pairs as 16-byte accesses from y's first 16-byte boundary on (head = 1
// when y is only 8-byte aligned), a scalar head and a scalar tail around
// them.  t has y's alignment modulo 16 (axpby_dispatch offsets it inside the
// scratch), so its pairs are aligned where y's are; it is read once:
// nontemporal.  HAVE_T = false: every t[r] is +0.0 (a plan with nothing
// stored), y = alpha * (+0.0) + beta * y.  Grid-stride on a capped grid, like
// k_multi.hip's kernels.
template <bool HAVE_T>
__global__ __launch_bounds__(256) void axpby_kernel(double *__restrict__ y, const double *__restrict__ t, double alpha,
                                                    double beta, int64_t m) {
    const int64_t head = (reinterpret_cast<uintptr_t>(y) & 15) != 0 ? 1 : 0;
    const int64_t pairs = (m - head) / 2;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = gid; i < pairs; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = head + 2 * i;
        f64x2 s = {0.0, 0.0};
        if constexpr (HAVE_T) s = ld_stream2(t + r);
        f64x2 v = *reinterpret_cast<const f64x2 *>(y + r);
        v.x = axpby(alpha, s.x, beta, v.x);
        v.y = axpby(alpha, s.y, beta, v.y);
        *reinterpret_cast<f64x2 *>(y + r) = v;
    }
    if (gid == 0) {
        if (head) y[0] = axpby(alpha, HAVE_T ? ld_stream(t) : 0.0, beta, y[0]);
        const int64_t last = head + 2 * pairs;  // m - 1 where a row is left over
        if (last < m) y[last] = axpby(alpha, HAVE_T ? ld_stream(t + last) : 0.0, beta, y[last]);
    }
}

int launch_axpby(const spmv_plan_s *p, double *y, const double *t, const Axpby &ab) {
    if (p->m == 0) return SPMV_SUCCESS;
    const dim3 grid(grid_for((p->m + 1) / 2));
    if (t) hipLaunchKernelGGL(axpby_kernel<true>, grid, dim3(256), 0, p->stream, y, t, ab.alpha, ab.beta, p->m);
    else hipLaunchKernelGGL(axpby_kernel<false>, grid, dim3(256), 0, p->stream, y, t, ab.alpha, ab.beta, p->m);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

}  // namespace spmv
