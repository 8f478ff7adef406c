// k_dot.hip -- spmv_execute_dot (y = A x, dots[0] = w . y, dots[1] = y . y):
// the last launch of every path, and the generic path's second pass.
//
//   dot_rows_kernel    streams the y the plan's own kernels wrote, and w, and
//                      writes one (t, q) pair per workgroup into the plan's
//                      partials (plans without a one-writer-per-row kernel,
//                      and plans with nothing stored after their zero fill)
//   dot_finish_kernel  ONE workgroup adds the slots of either path in a fixed
//                      order and writes the two doubles
//
// The fused path -- the same terms formed in the store epilogue of the
// one-writer-per-row kernels, the same workgroup reduction (device.hpp
// dot_block_store) -- lives in k_csr.hip, k_ell.hip and k_dia.hip.  No
// floating-point atomic, no counter and no "last block" protocol anywhere:
// the order of the adds is a function of the plan and of the path alone.
#include "build_util.hpp"
#include "device.hpp"
#include "internal.hpp"

namespace spmv {

// Row pairs (2 i, 2 i + 1), whatever the pointers' alignment, so the order of
// the adds is a function of m alone: a thread adds its pairs ascending, each
// pair in row order, then thread 0 the odd row m - 1; grid-stride on a capped
// grid.  y's pair is one 16-byte load where y is 16-byte aligned, else two
// scalars, and w's likewise -- the alignment of w is its own; nothing outside
// [w, w + m) is read.
__global__ __launch_bounds__(256) void dot_rows_kernel(const double *__restrict__ y, const double *__restrict__ w,
                                                       int64_t m, double *__restrict__ part) {
    const int64_t pairs = m / 2;
    const bool have_w = w != nullptr;
    const bool y16 = (reinterpret_cast<uintptr_t>(y) & 15) == 0, w16 = (reinterpret_cast<uintptr_t>(w) & 15) == 0;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double t = 0.0, q = 0.0;
    for (int64_t i = gid; i < pairs; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = 2 * i;
        f64x2 yv, wv = {0.0, 0.0};
        if (y16) {
            yv = *reinterpret_cast<const f64x2 *>(y + r);
        } else {
            yv.x = y[r];
            yv.y = y[r + 1];
        }
        if (have_w) {
            if (w16) {
                wv = *reinterpret_cast<const f64x2 *>(w + r);
            } else {
                wv.x = w[r];
                wv.y = w[r + 1];
            }
        }
        dot_add(t, q, true, have_w, wv.x, yv.x);
        dot_add(t, q, true, have_w, wv.y, yv.y);
    }
    if (gid == 0 && (m & 1)) dot_add(t, q, true, have_w, have_w ? w[m - 1] : 0.0, y[m - 1]);
    dot_block_store(t, q, part);
}

// One workgroup of 16 waves adds the slots in the fixed order of
// dot_slots_sum (device.hpp).  slots = 0 (m = 0): +0.0, +0.0.
__global__ __launch_bounds__(kDotFinishThreads) void dot_finish_kernel(const double *__restrict__ part, int64_t slots,
                                                                      double *__restrict__ dots) {
    double t, q;
    dot_slots_sum(part, slots, t, q);
    if (threadIdx.x == 0) {
        dots[0] = t;
        dots[1] = q;
    }
}

int64_t dot_rows_blocks(int64_t m) { return m > 0 ? (int64_t)grid_for((m + 1) / 2) : 0; }

int launch_dot_rows(const spmv_plan_s *p, const double *y, const double *w, double *part) {
    if (p->m == 0) return SPMV_SUCCESS;
    hipLaunchKernelGGL(dot_rows_kernel, dim3((unsigned)dot_rows_blocks(p->m)), dim3(256), 0, p->stream, y, w, p->m,
                       part);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

int launch_dot_finish(const spmv_plan_s *p, const double *part, int64_t slots, double *dots) {
    hipLaunchKernelGGL(dot_finish_kernel, dim3(1), dim3(kDotFinishThreads), 0, p->stream, part, slots, dots);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

}  // namespace spmv
