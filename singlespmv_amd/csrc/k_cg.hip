// k_cg.hip -- the vector kernels of spmv_cg_solve (Hestenes-Stiefel conjugate
// gradients on a plan).  The SpMV q = A p and p . q are the
// plan's own dot execute (capi_execute.cpp dot_dispatch); what is here is the
// rest of an iteration:
//
//   cg_init_kernel         z = dinv (.) r, p = z, slots of r . z, r . r and b . b
//   cg_init_finish_kernel  ONE workgroup: rz, rr, bb and the whole CgState
//   cg_update_kernel       alpha = rz / pq, x += alpha p, r -= alpha q, slots of
//                          r . z and r . r
//   cg_finish_kernel       ONE workgroup: rz, rr, beta, the counter, done, status
//   cg_direction_kernel    p = z + beta p (z formed again from r and dinv)
//
// Every operation is a rounded multiply, add or divide, never an FMA.  The
// scalars live in the plan's CgState: a kernel reads them from device memory,
// the one-workgroup kernels write them with ordinary stores from one lane.
// The reductions are spmv_execute_dot's (device.hpp dot_add, dot_block_store,
// dot_slots_sum): no floating-point atomic, no counter, the order of the adds
// a function of m alone.  Once state->done is set, update, finish and direction
// return at once (a grid-uniform read): the launches left in a check interval
// move nothing.
#include <cmath>

#include "build_util.hpp"
#include "device.hpp"
#include "internal.hpp"

namespace spmv {

namespace {

// Row pairs (2 i, 2 i + 1) whatever the pointers' alignment, as in
// dot_rows_kernel: 16-byte accesses where every vector of the kernel is
// 16-byte aligned (v16, kernel-uniform), else scalars.  NT: the nontemporal
// form, for a vector the next kernel does not read again.
template <bool NT>
__device__ __forceinline__ f64x2 ld_pair(const double *v, int64_t r, bool v16) {
    f64x2 a;
    if (v16) {
        a = NT ? ld_stream2(v + r) : *reinterpret_cast<const f64x2 *>(v + r);
    } else {
        a.x = NT ? ld_stream(v + r) : v[r];
        a.y = NT ? ld_stream(v + r + 1) : v[r + 1];
    }
    return a;
}
template <bool NT>
__device__ __forceinline__ void st_pair(double *v, int64_t r, bool v16, f64x2 a) {
    if (v16) {
        if (NT) __builtin_nontemporal_store(a, reinterpret_cast<f64x2 *>(v + r));
        else *reinterpret_cast<f64x2 *>(v + r) = a;
    } else if (NT) {
        __builtin_nontemporal_store(a.x, v + r);
        __builtin_nontemporal_store(a.y, v + r + 1);
    } else {
        v[r] = a.x;
        v[r + 1] = a.y;
    }
}
__device__ __forceinline__ bool aligned16(const void *a, const void *b = nullptr, const void *c = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

// z = dinv (.) r, or r itself without a preconditioner
__device__ __forceinline__ double precond(bool have_d, double d, double r) { return have_d ? __dmul_rn(d, r) : r; }

// p . Ap <= 0, NaN or infinite: A is not positive definite on p (or the data
// is not finite).  Grid-uniform: every thread reads the same double.
__device__ __forceinline__ bool cg_breakdown(double pq) { return !(pq > 0.0) || !(pq < INFINITY); }

__global__ __launch_bounds__(256) void cg_init_kernel(const double *__restrict__ b, const double *__restrict__ r,
                                                      const double *__restrict__ dinv, double *__restrict__ p,
                                                      int64_t m, double *__restrict__ part_rz,
                                                      double *__restrict__ part_bb) {
    const bool have_d = dinv != nullptr;
    const bool v16 = aligned16(b, dinv);  // r and p are the plan's: 16-byte aligned
    const int64_t pairs = m / 2;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double rz = 0.0, rr = 0.0, unused = 0.0, bb = 0.0;
    for (int64_t i = gid; i < pairs; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = 2 * i;
        const f64x2 bv = ld_pair<true>(b, row, v16), rv = ld_pair<false>(r, row, v16);
        f64x2 dv = {0.0, 0.0}, z;
        if (have_d) dv = ld_pair<true>(dinv, row, v16);
        z.x = precond(have_d, dv.x, rv.x);
        z.y = precond(have_d, dv.y, rv.y);
        st_pair<false>(p, row, v16, z);
        dot_add(rz, rr, true, true, z.x, rv.x);
        dot_add(rz, rr, true, true, z.y, rv.y);
        dot_add(unused, bb, true, false, 0.0, bv.x);
        dot_add(unused, bb, true, false, 0.0, bv.y);
    }
    if (gid == 0 && (m & 1)) {
        const int64_t row = m - 1;
        const double rv = r[row], z = precond(have_d, have_d ? dinv[row] : 0.0, rv);
        p[row] = z;
        dot_add(rz, rr, true, true, z, rv);
        dot_add(unused, bb, true, false, 0.0, b[row]);
    }
    dot_block_store(rz, rr, part_rz);
    __syncthreads();  // thread 0 has read the waves' first pairs
    dot_block_store(unused, bb, part_bb);
}

__global__ __launch_bounds__(kDotFinishThreads) void cg_init_finish_kernel(CgState *__restrict__ st,
                                                                          const double *__restrict__ part,
                                                                          int64_t slots, double rtol2,
                                                                          int32_t max_iters) {
    double rz, rr, unused, bb;
    dot_slots_sum(part, slots, rz, rr);
    __syncthreads();
    dot_slots_sum(part + 2 * slots, slots, unused, bb);
    if (threadIdx.x == 0) {
        const bool converged = rr <= __dmul_rn(rtol2, bb);
        st->dots[0] = 0.0;
        st->dots[1] = 0.0;
        st->rz = rz;
        st->rr = rr;
        st->bb = bb;
        st->pq = 0.0;
        st->beta = 0.0;
        st->rtol2 = rtol2;
        st->iterations = 0;
        st->max_iters = max_iters;
        st->done = converged || max_iters == 0 ? 1 : 0;
        st->status = converged ? SPMV_CG_CONVERGED : SPMV_CG_MAX_ITERS;
    }
}

__global__ __launch_bounds__(256) void cg_update_kernel(const CgState *__restrict__ st, double *__restrict__ x,
                                                        const double *__restrict__ p, double *__restrict__ r,
                                                        const double *__restrict__ q,
                                                        const double *__restrict__ dinv, int64_t m,
                                                        double *__restrict__ part) {
    if (st->done) return;
    const double pq = st->dots[0];
    if (cg_breakdown(pq)) return;  // no single row moves; cg_finish_kernel reports it
    const double alpha = __ddiv_rn(st->rz, pq);
    const bool have_d = dinv != nullptr;
    const bool v16 = aligned16(x, dinv);  // p, r and q are the plan's: 16-byte aligned
    const int64_t pairs = m / 2;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double rz = 0.0, rr = 0.0;
    for (int64_t i = gid; i < pairs; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = 2 * i;
        f64x2 xv = ld_pair<true>(x, row, v16), rv = ld_pair<false>(r, row, v16);
        const f64x2 pv = ld_pair<false>(p, row, v16), qv = ld_pair<true>(q, row, v16);
        f64x2 dv = {0.0, 0.0};
        if (have_d) dv = ld_pair<false>(dinv, row, v16);
        xv.x = __dadd_rn(xv.x, __dmul_rn(alpha, pv.x));
        xv.y = __dadd_rn(xv.y, __dmul_rn(alpha, pv.y));
        rv.x = __dsub_rn(rv.x, __dmul_rn(alpha, qv.x));
        rv.y = __dsub_rn(rv.y, __dmul_rn(alpha, qv.y));
        st_pair<true>(x, row, v16, xv);
        st_pair<false>(r, row, v16, rv);
        dot_add(rz, rr, true, true, precond(have_d, dv.x, rv.x), rv.x);
        dot_add(rz, rr, true, true, precond(have_d, dv.y, rv.y), rv.y);
    }
    if (gid == 0 && (m & 1)) {
        const int64_t row = m - 1;
        x[row] = __dadd_rn(x[row], __dmul_rn(alpha, p[row]));
        const double rv = __dsub_rn(r[row], __dmul_rn(alpha, q[row]));
        r[row] = rv;
        dot_add(rz, rr, true, true, precond(have_d, have_d ? dinv[row] : 0.0, rv), rv);
    }
    dot_block_store(rz, rr, part);
}

__global__ __launch_bounds__(kDotFinishThreads) void cg_finish_kernel(CgState *__restrict__ st,
                                                                     const double *__restrict__ part,
                                                                     int64_t slots) {
    if (st->done) return;
    const double pq = st->dots[0], rz_old = st->rz;
    if (cg_breakdown(pq)) {  // the update moved nothing: the counter stays
        if (threadIdx.x == 0) {
            st->pq = pq;
            st->status = SPMV_CG_BREAKDOWN;
            st->done = 1;
        }
        return;
    }
    double rz, rr;
    dot_slots_sum(part, slots, rz, rr);  // a barrier: every thread has read done by now
    if (threadIdx.x == 0) {
        const int32_t it = st->iterations + 1;
        const bool converged = rr <= __dmul_rn(st->rtol2, st->bb);
        st->pq = pq;
        st->beta = __ddiv_rn(rz, rz_old);
        st->rz = rz;
        st->rr = rr;
        st->iterations = it;
        if (converged || it == st->max_iters) {
            st->status = converged ? SPMV_CG_CONVERGED : SPMV_CG_MAX_ITERS;
            st->done = 1;
        }
    }
}

__global__ __launch_bounds__(256) void cg_direction_kernel(const CgState *__restrict__ st,
                                                           const double *__restrict__ r,
                                                           const double *__restrict__ dinv, double *__restrict__ p,
                                                           int64_t m) {
    if (st->done) return;
    const double beta = st->beta;
    const bool have_d = dinv != nullptr;
    const bool v16 = aligned16(dinv);  // r and p are the plan's: 16-byte aligned
    const int64_t pairs = m / 2;
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = gid; i < pairs; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = 2 * i;
        const f64x2 rv = ld_pair<false>(r, row, v16);
        f64x2 pv = ld_pair<false>(p, row, v16), dv = {0.0, 0.0};
        if (have_d) dv = ld_pair<false>(dinv, row, v16);
        pv.x = __dadd_rn(precond(have_d, dv.x, rv.x), __dmul_rn(beta, pv.x));
        pv.y = __dadd_rn(precond(have_d, dv.y, rv.y), __dmul_rn(beta, pv.y));
        st_pair<false>(p, row, v16, pv);
    }
    if (gid == 0 && (m & 1)) {
        const int64_t row = m - 1;
        p[row] = __dadd_rn(precond(have_d, have_d ? dinv[row] : 0.0, r[row]), __dmul_rn(beta, p[row]));
    }
}

}  // namespace

int64_t cg_blocks(int64_t m) { return m > 0 ? (int64_t)grid_for((m + 1) / 2) : 0; }

int launch_cg_init(const spmv_plan_s *p, const double *b, const double *dinv, double rtol2, int32_t max_iters) {
    const CgWork &w = p->cg;
    const int64_t slots = cg_blocks(p->m);
    hipLaunchKernelGGL(cg_init_kernel, dim3((unsigned)slots), dim3(256), 0, p->stream, b, (const double *)w.r, dinv,
                       w.p, p->m, w.part, w.part + 2 * slots);
    SPMV_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cg_init_finish_kernel, dim3(1), dim3(kDotFinishThreads), 0, p->stream, w.state,
                       (const double *)w.part, slots, rtol2, max_iters);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

int launch_cg_update(const spmv_plan_s *p, double *x, const double *dinv) {
    const CgWork &w = p->cg;
    hipLaunchKernelGGL(cg_update_kernel, dim3((unsigned)cg_blocks(p->m)), dim3(256), 0, p->stream,
                       (const CgState *)w.state, x, (const double *)w.p, w.r, (const double *)w.q, dinv, p->m, w.part);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

int launch_cg_finish(const spmv_plan_s *p) {
    const CgWork &w = p->cg;
    hipLaunchKernelGGL(cg_finish_kernel, dim3(1), dim3(kDotFinishThreads), 0, p->stream, w.state,
                       (const double *)w.part, cg_blocks(p->m));
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

int launch_cg_direction(const spmv_plan_s *p, const double *dinv) {
    const CgWork &w = p->cg;
    hipLaunchKernelGGL(cg_direction_kernel, dim3((unsigned)cg_blocks(p->m)), dim3(256), 0, p->stream,
                       (const CgState *)w.state, (const double *)w.r, dinv, w.p, p->m);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

}  // namespace spmv
