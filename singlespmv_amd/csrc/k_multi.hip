// k_multi.hip -- Y = A X for K interleaved right-hand sides (spmv_execute_multi):
// the DIA and sliced-ELL kernels of k_dia.hip / k_ell.hip with K accumulators
// per row, so the matrix is streamed once for K vectors, plus the strided
// copies of the generic path.
//
// X and Y are row-major blocks: x_j[i] = X[i*ldx + j], y_j[r] = Y[r*ldy + j].
// The fused kernels need K even, X and Y 16-byte aligned and ldx, ldy even, so
// that a row's K values are K/2 aligned 16-byte accesses (the caller checks,
// capi.cpp multi_block_fused).  They read the existing plan layouts (DiaDev,
// EllDev) and sum every (row, column) exactly as the single-vector kernel
// does: one accumulator, slots / diagonals in the stored order, a rounded
// multiply then a rounded add -- column j of Y is bit for bit what
// spmv_execute gives for column j of X, and depends on no other column.
#include "device.hpp"
#include "internal.hpp"

namespace spmv {

// a row's K contiguous values as K/2 16-byte loads / nontemporal stores
template <int K>
__device__ __forceinline__ void ld_row(const double *p, double (&g)[K]) {
#pragma unroll
    for (int j = 0; j < K; j += 2) {
        const f64x2 t = *reinterpret_cast<const f64x2 *>(p + j);
        g[j] = t.x;
        g[j + 1] = t.y;
    }
}
template <int K>
__device__ __forceinline__ void st_row(double *p, const double (&a)[K]) {
#pragma unroll
    for (int j = 0; j < K; j += 2) {
        f64x2 t;
        t.x = a[j];
        t.y = a[j + 1];
        __builtin_nontemporal_store(t, reinterpret_cast<f64x2 *>(p + j));  // y is not re-read
    }
}

// ---- DIA -------------------------------------------------------------------
// Block and value addressing of dia_kernel: 512-row workgroups, two rows per
// lane, one 16-byte value load per diagonal (8 in flight), `group` interleave,
// offsets ascending.  Each value pair feeds 2 K accumulators.
//
// LDSX: the workgroup's x window (win rows, all K columns) is staged into LDS
// as K PLANES, xs[j*wpad + i] = x_j[c0 + i], not as interleaved rows.  A lane
// reads rows li, li + 1 of every plane; li = 2*lane + const has either
// parity, so in a plane the pair is two ds_read_b64 at a 16-byte lane stride:
// the 32 lanes of a group span 512 B, lanes l and l + 16 share a bank, 2-way,
// whatever K is -- the pattern of dia_kernel.  Interleaved rows would make
// the pair 2 K contiguous doubles (K ds_read_b128, always aligned) at a lane
// stride of 16 K bytes: the 16 lanes of a ds_read_b128 group then land on
// 16 / K of the 16 slots of a bank row, 2-way at K = 2, 4-way at 4, 8-way at
// 8 -- worse exactly where the LDS rate matters (K = 8 reads 64 B of LDS per
// 8 B of values).  wpad = win rounded up to 16, plus 16 / K: consecutive
// planes start 128 / K bytes apart in a 128-byte bank row, so the staging
// stores (16 consecutive lanes = 16 / K rows x K planes, ds_write_b64) hit 16
// different bank pairs.
//
// Without LDSX (window beyond the LDS at this K, or wider than the rows the
// lanes read: dia_multi_use_lds) the x rows are read from global memory,
// clamped to [0, n - 1] like dia_kernel's.
template <int K, bool LDSX>
__global__ __launch_bounds__(256) void dia_multi_kernel(int64_t m, int64_t mp, int64_t n, int n_diags,
                                                        const int32_t *__restrict__ off, int32_t off_min, int32_t win,
                                                        int32_t wpad, const double *__restrict__ val,
                                                        const double *__restrict__ X, int64_t ldx,
                                                        double *__restrict__ Y, int64_t ldy, int32_t group) {
    extern __shared__ double xs[];
    constexpr int UNROLL = 8;
    const int64_t r0 = 2 * (int64_t)blockIdx.x * blockDim.x;
    const int64_t r = r0 + 2 * threadIdx.x;
    int64_t vbase = (int64_t)blockIdx.x * n_diags * kDiaBlockRows, dstride = kDiaBlockRows;
    if (group > 0) {
        const int64_t t = blockIdx.x / group, g = blockIdx.x - t * group;
        const int64_t rest = mp / kDiaBlockRows - t * group;
        vbase = (t * group * n_diags + g) * kDiaBlockRows;
        dstride = (rest < group ? rest : group) * kDiaBlockRows;
    }
    const double *vb = val + vbase + 2 * threadIdx.x;
    auto xrow = [&](int64_t c) { return X + (c < 0 ? 0 : (c >= n ? n - 1 : c)) * ldx; };
    if (LDSX) {
        // out-of-range columns only meet zero-filled slots: any in-bounds row works
        const int64_t c0 = r0 + off_min;
        for (int idx = threadIdx.x; idx < win * K; idx += blockDim.x) {
            const int i = idx / K, j = idx - i * K;
            xs[j * wpad + i] = xrow(c0 + i)[j];
        }
        __syncthreads();
    }
    if (r >= m) return;
    double a0[K], a1[K];
#pragma unroll
    for (int j = 0; j < K; ++j) a0[j] = a1[j] = 0.0;
    const int lbase = 2 * threadIdx.x - off_min;  // LDS row of column r + 0
    auto step = [&](f64x2 v, int32_t o) {
        if (LDSX) {
            const double *q = xs + lbase + o;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const double g0 = q[j * wpad], g1 = q[j * wpad + 1];
                a0[j] = madd(v.x, g0, a0[j]);
                a1[j] = madd(v.y, g1, a1[j]);
            }
        } else {
            double g0[K], g1[K];
            ld_row<K>(xrow(r + o), g0);
            ld_row<K>(xrow(r + o + 1), g1);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                a0[j] = madd(v.x, g0[j], a0[j]);
                a1[j] = madd(v.y, g1[j], a1[j]);
            }
        }
    };
    int d = 0;
    for (; d + UNROLL <= n_diags; d += UNROLL) {
        f64x2 v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) v[u] = ld_stream2(vb + (int64_t)(d + u) * dstride);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) step(v[u], off[d + u]);
    }
    for (; d < n_diags; ++d) step(ld_stream2(vb + (int64_t)d * dstride), off[d]);
    st_row<K>(Y + r * ldy, a0);
    if (r + 1 < m) st_row<K>(Y + (r + 1) * ldy, a1);
}

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

// LDS a workgroup may request on gfx950
constexpr size_t kMultiMaxLds = (size_t)160 << 10;

static int64_t dia_multi_wpad(int64_t win, int K) { return (win + 15) / 16 * 16 + 16 / K; }

// LDSX is taken where the staged window fits the LDS at this K and is no
// larger than what the lanes would otherwise read directly: staging moves
// win rows per workgroup, the global-x variant n_diags * 512 (64 diagonals,
// span 63: 576 against 32768, staged 2.9 x faster at K = 8; three diagonals
// 1500 apart: 3513 against 1536, staged 3.6 x / 4.8 x slower at K = 2 / 4 --
// profiles/multi_rhs/dia_variants.jsonl).
static bool dia_multi_use_lds(const spmv_plan_s *p, int K) {
    const DiaDev &d = p->dia;
    const int64_t win = 512 + (int64_t)d.off_host.back() - d.off_host.front() + 1;
    const bool fits = sizeof(double) * (size_t)dia_multi_wpad(win, K) * K <= kMultiMaxLds;
    bool lds = fits && win <= (int64_t)d.n_diags * kDiaBlockRows;
    // probe build: 0 = global x, 1 = LDS wherever it fits (tools/multi_rhs_times.py --dia-variants)
    if (const char *e = probe_env("SPMV_LAUNCH_DIA_MULTI_LDSX")) lds = fits && std::atoi(e) != 0;
    return lds;
}

template <int K>
static void launch_dia_multi_k(const spmv_plan_s *p, const double *X, int64_t ldx, double *Y, int64_t ldy) {
    const DiaDev &d = p->dia;
    const int64_t blocks = ((p->m + 1) / 2 + 255) / 256;
    const int32_t off_min = d.off_host.front();
    const int64_t win = 512 + (int64_t)d.off_host.back() - off_min + 1;
    if (dia_multi_use_lds(p, K)) {
        const int32_t wpad = (int32_t)dia_multi_wpad(win, K);
        // Only the window is requested.  launch_dia's 96-KB request for plans
        // above kDiaVmmMinBytes (one workgroup per CU: fewer HBM streams) costs
        // this kernel its LDS read rate, which needs more than one wave per
        // SIMD: 64 diagonals, 2 M rows, same plan, K = 2 / 4 / 8: 0.265 / 0.292 /
        // 0.524 ms with the request, 0.181 / 0.246 / 0.383 without
        // (profiles/multi_rhs/dia_variants.jsonl)
        int kb = 0;
        if (const char *e = probe_env("SPMV_LAUNCH_DIA_MULTI_LDS_KB")) kb = std::atoi(e);  // probe: occupancy A/B
        const size_t lds = std::min(kMultiMaxLds, std::max(sizeof(double) * (size_t)wpad * K, (size_t)kb * 1024));
        hipLaunchKernelGGL((dia_multi_kernel<K, true>), dim3((unsigned)blocks), dim3(256), lds, p->stream, p->m, d.mp,
                           p->n, d.n_diags, d.off, off_min, (int32_t)win, wpad, d.val, X, ldx, Y, ldy, d.group);
    } else {
        hipLaunchKernelGGL((dia_multi_kernel<K, false>), dim3((unsigned)blocks), dim3(256), 0, p->stream, p->m, d.mp,
                           p->n, d.n_diags, d.off, off_min, 0, 0, d.val, X, ldx, Y, ldy, d.group);
    }
}

int launch_dia_multi(const spmv_plan_s *p, int K, const double *X, int64_t ldx, double *Y, int64_t ldy) {
    if (p->m == 0) return SPMV_SUCCESS;
    if (p->dia.n_diags == 0) return launch_multi_zero(p, K, Y, ldy);  // no stored diagonal: Y = 0
    switch (K) {
        case 2: launch_dia_multi_k<2>(p, X, ldx, Y, ldy); break;
        case 4: launch_dia_multi_k<4>(p, X, ldx, Y, ldy); break;
        case 8: launch_dia_multi_k<8>(p, X, ldx, Y, ldy); break;
        default: set_error("dia multi: no kernel of this width"); return SPMV_ERROR_INVALID_VALUE;
    }
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

// ---- sliced ELL / JDS ------------------------------------------------------
// ell_slice_kernel with K accumulators: one wave per 64-row slice, one lane
// per row, the same column quad and two value-half loads; each gathered
// column c fetches the K contiguous doubles of X row c (K/2 16-byte loads
// from one or two lines the single-vector gather pulls anyway).  UNROLL
// quads per iteration: 4 UNROLL K doubles of gathers in flight per lane --
// 2, 2, 1 quads for K = 2, 4, 8 (65 / 95 / 97 VGPRs as compiled with O32, 78 /
// 106 / 100 without; no scratch: K = 8 at 2 quads would hold 128 VGPRs of
// gathers alone).
template <int K, int UNROLL, bool PERM, bool O32>
__global__ __launch_bounds__(256) void ell_slice_multi_kernel(int64_t m, int64_t n_slices,
                                                              const int32_t *__restrict__ perm,
                                                              const int64_t *__restrict__ slice_off,
                                                              const int32_t *__restrict__ col,
                                                              const double *__restrict__ val,
                                                              const double *__restrict__ X, int64_t ldx,
                                                              double *__restrict__ Y, int64_t ldy) {
    const int64_t slice = (int64_t)blockIdx.x * (blockDim.x / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (slice >= n_slices) return;
    const int64_t srow = slice * 64 + lane;
    // JDS: the matrix row, loaded before the slots so its latency hides behind them
    const int64_t row = PERM ? (srow < m ? (int64_t)perm[srow] : 0) : srow;
    const int64_t base = slice_off[slice];
    const int64_t quads = (slice_off[slice + 1] - base) >> 8;
    const char *cs = (const char *)(col + base);  // wave-uniform slice bases
    const char *vs = (const char *)(val + base);
    auto at = [&](const char *b, int64_t byte_off) {
        if constexpr (O32) return b + (uint32_t)byte_off;
        else return b + byte_off;
    };
    auto ldc = [&](int64_t q) { return ld_stream4((const int32_t *)at(cs, (q * 256 + lane * 4) * 4)); };
    auto ldv = [&](int64_t q, int h) { return ld_stream2((const double *)at(vs, (q * 256 + h * 128 + lane * 2) * 8)); };
    const uint32_t ldx8 = O32 ? (uint32_t)ldx * 8u : 0u;
    auto ldxr = [&](int c, double (&g)[K]) {
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
    if (srow < m) st_row<K>(Y + row * ldy, acc);
}

template <int K, int U, bool O32>
static void launch_ell_multi_ko(const spmv_plan_s *p, const double *X, int64_t ldx, double *Y, int64_t ldy) {
    const EllDev &e = p->ell;
    const int64_t blocks = (e.n_slices + 3) / 4;
    // the LDS request of launch_ell above 256 MB of slots: two workgroups per CU
    const size_t lds = (size_t)e.slots * sizeof(double) >= kStreamVmmMinBytes ? (size_t)64 * 1024 : 0;
    if (e.perm)
        hipLaunchKernelGGL((ell_slice_multi_kernel<K, U, true, O32>), dim3((unsigned)blocks), dim3(256), lds, p->stream,
                           p->m, e.n_slices, e.perm, e.slice_off, e.col, e.val, X, ldx, Y, ldy);
    else
        hipLaunchKernelGGL((ell_slice_multi_kernel<K, U, false, O32>), dim3((unsigned)blocks), dim3(256), lds, p->stream,
                           p->m, e.n_slices, e.perm, e.slice_off, e.col, e.val, X, ldx, Y, ldy);
}

template <int K, int U>
static void launch_ell_multi_k(const spmv_plan_s *p, const double *X, int64_t ldx, double *Y, int64_t ldy) {
    // 32-bit byte offsets: the X block below 4 GB and a slice's values below 2 GB
    const bool o32 = p->n * ldx < ((int64_t)1 << 29) && ldx < ((int64_t)1 << 28) &&
                     (int64_t)p->ell.max_width * 64 * 8 < ((int64_t)1 << 31);
    if (o32) launch_ell_multi_ko<K, U, true>(p, X, ldx, Y, ldy);
    else launch_ell_multi_ko<K, U, false>(p, X, ldx, Y, ldy);
}

int launch_ell_multi(const spmv_plan_s *p, int K, const double *X, int64_t ldx, double *Y, int64_t ldy) {
    if (p->ell.n_slices == 0) return SPMV_SUCCESS;
    switch (K) {
        case 2: launch_ell_multi_k<2, 2>(p, X, ldx, Y, ldy); break;
        case 4: launch_ell_multi_k<4, 2>(p, X, ldx, Y, ldy); break;
        case 8: launch_ell_multi_k<8, 1>(p, X, ldx, Y, ldy); break;
        default: set_error("ell multi: no kernel of this width"); return SPMV_ERROR_INVALID_VALUE;
    }
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

// ---- generic path: one column through the plan's own kernels ---------------
// dst[i*dst_ld] = src[i*src_ld]: ld = 1 on the contiguous side
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
