// k_ell.hip -- sliced ELL SpMV for gfx950: the opt_ell hot loop
// (src/opt_ell.cpp:75-89, y[r] += x[col] * val over the row's slots)
// re-laid out for wave64.
//
// One wave = one slice of 64 consecutive rows, one lane = one row.  Slots are
// interleaved by 4 (see EllDev): at step q a lane issues one 16-byte load of
// 4 column indices and two 16-byte loads of 4 values (slots 0-1 from the
// quad's first KiB of values, 2-3 from its second) -- every wave instruction
// reads 1 KiB contiguous -- then 4 x gathers.  The slice width is
// wave-uniform, so the loop has no divergence.  Each row is summed
// sequentially in slot order with a rounded multiply + rounded add, i.e. the
// same arithmetic as opt_crs/opt_ell (bit-exact against oracle/).  Padding
// slots carry val = 0 and repeat a real column of the row.  With PERM the
// slices hold rows sorted by length (JDS, src/opt_jds.cpp:29-71, 91-103) and
// y is written through the permutation.
//
// O32 (x below 4 GB, a slice below 2 GB): the wave's slice base is
// wave-uniform (SGPR) and every load addresses it, or x, plus a 32-bit byte
// offset (the global_load saddr form), instead of 64-bit per-lane addresses.
//
// K right-hand sides (spmv_execute_multi, K = 2, 4, 8: x_j[i] = X[i*ldx + j],
// y_j[r] = Y[r*ldy + j], rows 16-byte aligned) run the same body with K
// accumulators per row, so the slots are streamed once for K vectors: each
// gathered column c fetches the K contiguous doubles of X row c (K/2 16-byte
// loads from one or two lines the single-vector gather pulls anyway).  Every
// column is summed exactly as the single vector is -- column j of Y is bit
// for bit what spmv_execute gives for column j of X.
#include "device.hpp"
#include "internal.hpp"

#include <type_traits>

namespace spmv {

template <bool O32>
__device__ __forceinline__ const char *ell_at(const void *base, int64_t byte_off) {
    if constexpr (O32) return (const char *)base + (uint32_t)byte_off;
    else return (const char *)base + byte_off;
}

// UNROLL quads per iteration: 4 UNROLL K doubles of gathers in flight per lane
//
// AB (K = 1, spmv_execute_axpby): the store writes alpha * sum + beta * y0
// (device.hpp axpby); y0 = Y[row], through perm for JDS, is loaded before the
// slots like the perm entry itself.
//
// DOT (K = 1, spmv_execute_dot): the lane's terms w[row] * y[row] and y[row]^2
// of the sum it stores (w through perm for JDS, loaded where y0 is) go into
// the workgroup's slot of `part` (device.hpp dot_block_store): no wave leaves
// early -- a slice past the last one has no slots and no rows, and still meets
// the reduction and its barrier.
template <int K, int UNROLL, bool PERM, bool O32, bool AB = false, bool DOT = false>
__device__ __forceinline__ void ell_slice_body(int64_t m, int64_t n_slices, const int32_t *__restrict__ perm,
                                               const int64_t *__restrict__ slice_off,
                                               const int32_t *__restrict__ col, const double *__restrict__ val,
                                               const double *__restrict__ X, int64_t ldx, double *__restrict__ Y,
                                               int64_t ldy, double alpha = 0.0, double beta = 0.0,
                                               const double *__restrict__ w = nullptr,
                                               double *__restrict__ part = nullptr) {
    static_assert(!AB || K == 1, "the axpby epilogue is single-vector");
    static_assert(!DOT || (K == 1 && !AB), "the dot epilogue is single-vector, without alpha and beta");
    const int64_t slice = (int64_t)blockIdx.x * (blockDim.x / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if constexpr (!DOT) {
        if (slice >= n_slices) return;
    }
    const bool dead = DOT && slice >= n_slices;  // wave-uniform
    const int64_t srow = dead ? m : slice * 64 + lane;
    // JDS: the matrix row, loaded before the slots so its latency hides
    // behind them instead of trailing the wave
    const int64_t row = PERM ? (srow < m ? (int64_t)perm[srow] : 0) : srow;
    double y0 = 0.0;
    if constexpr (AB) {
        if (srow < m) y0 = ld_stream(Y + row * ldy);
    }
    double wr = 0.0;
    if constexpr (DOT) {
        if (w != nullptr && srow < m) wr = w[row];
    }
    const int64_t base = slice_off[dead ? 0 : slice];
    const int64_t quads = dead ? 0 : (slice_off[slice + 1] - base) >> 8;  // (width/4)
    const int32_t *cs = col + base;  // wave-uniform slice bases
    const double *vs = val + base;
    auto ldc = [&](int64_t q) { return ld_stream4((const int32_t *)ell_at<O32>(cs, (q * 256 + lane * 4) * 4)); };
    auto ldv = [&](int64_t q, int h) {
        return ld_stream2((const double *)ell_at<O32>(vs, (q * 256 + h * 128 + lane * 2) * 8));
    };
    const uint32_t ldx8 = O32 ? (uint32_t)ldx * 8u : 0u;
    auto ldxr = [&](int c, double (&g)[K]) {  // x gathers: plain cached loads (x is the re-used operand)
        if constexpr (O32) ld_row<K>((const double *)((const char *)X + (uint32_t)c * ldx8), g);
        else ld_row<K>(X + (int64_t)c * ldx, g);
    };
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    auto add = [&](double v, const double (&g)[K]) {
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] = madd(v, g[j], acc[j]);
    };
    int64_t q = 0;
    for (; q + UNROLL <= quads; q += UNROLL) {
        i32x4 c[UNROLL];
        f64x2 a[UNROLL], b[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            c[u] = ldc(q + u);
            a[u] = ldv(q + u, 0);
            b[u] = ldv(q + u, 1);
        }
        double g[UNROLL][4][K];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            ldxr(c[u].x, g[u][0]);
            ldxr(c[u].y, g[u][1]);
            ldxr(c[u].z, g[u][2]);
            ldxr(c[u].w, g[u][3]);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            add(a[u].x, g[u][0]);
            add(a[u].y, g[u][1]);
            add(b[u].x, g[u][2]);
            add(b[u].y, g[u][3]);
        }
    }
    for (; q < quads; ++q) {
        const i32x4 c = ldc(q);
        const f64x2 a = ldv(q, 0);
        const f64x2 b = ldv(q, 1);
        double g[4][K];
        ldxr(c.x, g[0]);
        ldxr(c.y, g[1]);
        ldxr(c.z, g[2]);
        ldxr(c.w, g[3]);
        add(a.x, g[0]);
        add(a.y, g[1]);
        add(b.x, g[2]);
        add(b.y, g[3]);
    }
    if constexpr (AB) acc[0] = axpby(alpha, acc[0], beta, y0);
    if (srow < m) st_row<K>(Y + row * ldy, acc);
    if constexpr (DOT) {
        double t = 0.0, q = 0.0;
        dot_add(t, q, srow < m, w != nullptr, wr, acc[0]);
        dot_block_store(t, q, part);
    }
}

// the single vector: K = 1, the unit strides fold away
template <int UNROLL, bool PERM, bool O32 = false>
__global__ __launch_bounds__(256) void ell_slice_kernel(int64_t m, int64_t n_slices,
                                                        const int32_t *__restrict__ perm,
                                                        const int64_t *__restrict__ slice_off,
                                                        const int32_t *__restrict__ col,
                                                        const double *__restrict__ val,
                                                        const double *__restrict__ x,
                                                        double *__restrict__ y) {
    ell_slice_body<1, UNROLL, PERM, O32>(m, n_slices, perm, slice_off, col, val, x, 1, y, 1);
}

// y = alpha * A x + beta * y: the single-vector body with the axpby epilogue
template <int UNROLL, bool PERM, bool O32>
__global__ __launch_bounds__(256) void ell_slice_axpby_kernel(int64_t m, int64_t n_slices,
                                                              const int32_t *__restrict__ perm,
                                                              const int64_t *__restrict__ slice_off,
                                                              const int32_t *__restrict__ col,
                                                              const double *__restrict__ val,
                                                              const double *__restrict__ x, double *__restrict__ y,
                                                              double alpha, double beta) {
    ell_slice_body<1, UNROLL, PERM, O32, true>(m, n_slices, perm, slice_off, col, val, x, 1, y, 1, alpha, beta);
}

// y = A x with the rows' dot terms reduced into the plan's partials
template <int UNROLL, bool PERM, bool O32>
__global__ __launch_bounds__(256) void ell_slice_dot_kernel(int64_t m, int64_t n_slices,
                                                            const int32_t *__restrict__ perm,
                                                            const int64_t *__restrict__ slice_off,
                                                            const int32_t *__restrict__ col,
                                                            const double *__restrict__ val,
                                                            const double *__restrict__ x, double *__restrict__ y,
                                                            const double *__restrict__ w, double *__restrict__ part) {
    ell_slice_body<1, UNROLL, PERM, O32, false, true>(m, n_slices, perm, slice_off, col, val, x, 1, y, 1, 0.0, 0.0, w,
                                                      part);
}

template <int K, int UNROLL, bool PERM, bool O32>
__global__ __launch_bounds__(256) void ell_slice_multi_kernel(int64_t m, int64_t n_slices,
                                                              const int32_t *__restrict__ perm,
                                                              const int64_t *__restrict__ slice_off,
                                                              const int32_t *__restrict__ col,
                                                              const double *__restrict__ val,
                                                              const double *__restrict__ X, int64_t ldx,
                                                              double *__restrict__ Y, int64_t ldy) {
    ell_slice_body<K, UNROLL, PERM, O32>(m, n_slices, perm, slice_off, col, val, X, ldx, Y, ldy);
}

constexpr int kEllLdsKb = 64;  // LDS per workgroup of a large ELL launch: 2 workgroups per CU

// Above 256 MB of slots the launch requests 64 KB of LDS: two workgroups
// (8 waves, ~48 KB of slots in flight) per CU instead of the 8 the
// registers allow -- fewer concurrent streams, as DIA's cap (config 4,
// same plans: 2.421-2.425 -> 2.382-2.387 ms over three plans,
// profiles/round4/probe/c4_ell_window_variants.jsonl).
static size_t ell_lds(const EllDev &e) {
    return (size_t)e.slots * sizeof(double) >= kStreamVmmMinBytes ? (size_t)kEllLdsKb * 1024 : 0;
}

// 32-bit byte offsets: the X block below 4 GB and a slice's values below 2 GB
static bool ell_o32(const spmv_plan_s *p, int64_t ldx) {
    return p->n * ldx < ((int64_t)1 << 29) && ldx < ((int64_t)1 << 28) &&
           (int64_t)p->ell.max_width * 64 * 8 < ((int64_t)1 << 31);
}

// one launch of K vectors, U quads per iteration (K = 1: ldx = ldy = 1; ab:
// with the axpby epilogue)
template <int K, int U>
static void launch_ell_ku(const spmv_plan_s *p, const double *X, int64_t ldx, double *Y, int64_t ldy, size_t lds,
                          bool o32, const Axpby *ab = nullptr, const DotArgs *dot = nullptr) {
    const EllDev &e = p->ell;
    const dim3 blocks((unsigned)((e.n_slices + 3) / 4));
    auto go = [&](auto perm, auto o) {
        constexpr bool P = decltype(perm)::value, O = decltype(o)::value;
        if constexpr (K == 1) {
            if (dot)
                hipLaunchKernelGGL((ell_slice_dot_kernel<U, P, O>), blocks, dim3(256), lds, p->stream, p->m,
                                   e.n_slices, e.perm, e.slice_off, e.col, e.val, X, Y, dot->w, dot->part);
            else if (ab)
                hipLaunchKernelGGL((ell_slice_axpby_kernel<U, P, O>), blocks, dim3(256), lds, p->stream, p->m,
                                   e.n_slices, e.perm, e.slice_off, e.col, e.val, X, Y, ab->alpha, ab->beta);
            else
                hipLaunchKernelGGL((ell_slice_kernel<U, P, O>), blocks, dim3(256), lds, p->stream, p->m, e.n_slices,
                                   e.perm, e.slice_off, e.col, e.val, X, Y);
        } else
            hipLaunchKernelGGL((ell_slice_multi_kernel<K, U, P, O>), blocks, dim3(256), lds, p->stream, p->m,
                               e.n_slices, e.perm, e.slice_off, e.col, e.val, X, ldx, Y, ldy);
    };
    auto go_o = [&](auto perm) {
        if (o32) go(perm, std::true_type{});
        else go(perm, std::false_type{});
    };
    if (e.perm) go_o(std::true_type{});
    else go_o(std::false_type{});
}

// the launch's workgroups (4 slices each): the slots a dot launch writes
int64_t ell_dot_blocks(const spmv_plan_s *p) { return (p->ell.n_slices + 3) / 4; }

int launch_ell(const spmv_plan_s *p, const double *x, double *y, const Axpby *ab, const DotArgs *dot) {
    const EllDev &e = p->ell;
    if (e.n_slices == 0) return SPMV_SUCCESS;
    // 2 quads (4 slots each) per lane per iteration: 2 beat 4 by 28 % at
    // config 4, 5 % at config 2 (round 4 A/B)
    launch_ell_ku<1, 2>(p, x, 1, y, 1, ell_lds(e), ell_o32(p, 1), ab, dot);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

// 2, 2, 1 quads per iteration for K = 2, 4, 8 (65 / 95 / 97 VGPRs as
// compiled with O32, 78 / 106 / 100 without; no scratch: K = 8 at 2 quads would
// hold 128 VGPRs of gathers alone)
int launch_ell_multi(const spmv_plan_s *p, int K, const double *X, int64_t ldx, double *Y, int64_t ldy) {
    if (p->ell.n_slices == 0) return SPMV_SUCCESS;
    const size_t lds = ell_lds(p->ell);
    const bool o32 = ell_o32(p, ldx);
    switch (K) {
        case 2: launch_ell_ku<2, 2>(p, X, ldx, Y, ldy, lds, o32); break;
        case 4: launch_ell_ku<4, 2>(p, X, ldx, Y, ldy, lds, o32); break;
        case 8: launch_ell_ku<8, 1>(p, X, ldx, Y, ldy, lds, o32); break;
        default: set_error("ell multi: no kernel of this width"); return SPMV_ERROR_INVALID_VALUE;
    }
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

}  // namespace spmv
