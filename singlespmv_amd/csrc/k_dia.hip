// k_dia.hip -- DIA SpMV for gfx950: replaces the serial opt_dia loop
// (src/opt_dia.cpp:65-97, y[col+off-ioff] += diag*x[col], plus a leaked
// tmp[m+n-1] per call at :80).
//
// Row-indexed diagonals, blocked: the 512 rows of workgroup b hold every
// diagonal contiguously, val[(b*n_diags + d)*512 + r%512] = A[r, r + off[d]],
// so a workgroup streams ONE contiguous n_diags*4 KB block (the first layout,
// diagonal-major val[d*mp + r], read 64 streams 160 MB apart at config 4:
// 1.81 ms vs the blocked layout's, profiles/round1/probe/dia_blocked_ab.jsonl).
// One lane = two rows; the diagonal loop is wave-uniform and the offsets are
// loaded as scalars, so HBM sees ~8 B per stored slot + x + y.  Diagonals are summed in ascending offset order, i.e.
// ascending column order with rounded multiply + add: bit-identical to the
// sequential opt_crs row sum.  Out-of-range slots hold 0 and read a clamped,
// in-bounds x entry.
//
// K right-hand sides (spmv_execute_multi, K = 2, 4, 8: x_j[i] = X[i*ldx + j],
// y_j[r] = Y[r*ldy + j], rows 16-byte aligned) run the same body with 2 K
// accumulators per lane, so the values are streamed once for K vectors.
// Every column is summed exactly as the single vector is -- column j of Y is
// bit for bit what spmv_execute gives for column j of X.
#include "device.hpp"
#include "internal.hpp"

namespace spmv {

// Two rows per lane: one 16-byte load of the lane's two rows per diagonal, so
// a wave instruction streams 1 KiB; UNROLL of them in flight.
//
// LDSX: the workgroup's 512 rows need x over ONE contiguous column window
// [r0 + off_min, r0 + 511 + off_max + 1]; it is staged once into LDS with
// coalesced loads and every diagonal reads its pair x[c], x[c+1] from there,
// so the only HBM stream left is val (and x once).  Without LDSX (diagonal
// span too wide for the window, or dia_multi_use_lds) the x rows are read
// from global memory per diagonal, clamped to [0, n - 1].
//
// The window (win rows, all K columns) is staged as K PLANES,
// xs[j*wpad + i] = x_j[c0 + i] (K = 1: xs[i]), not as interleaved rows.  A
// lane reads rows li, li + 1 of every plane; li = 2*lane + const has either
// parity, so in a plane the pair is two ds_read_b64 at a 16-byte lane stride:
// the 32 lanes of a group span 512 B, lanes l and l + 16 share a bank, 2-way,
// whatever K is.  Interleaved rows would make the pair 2 K contiguous doubles
// (K ds_read_b128, always aligned) at a lane stride of 16 K bytes: the 16
// lanes of a ds_read_b128 group then land on 16 / K of the 16 slots of a bank
// row, 2-way at K = 2, 4-way at 4, 8-way at 8 -- worse exactly where the LDS
// rate matters (K = 8 reads 64 B of LDS per 8 B of values).  wpad = win
// rounded up to 16, plus 16 / K: consecutive planes start 128 / K bytes apart
// in a 128-byte bank row, so the staging stores (16 consecutive lanes =
// 16 / K rows x K planes, ds_write_b64) hit 16 different bank pairs.
//
// K = 1 is the single-vector kernel: ldx = ldy = 1, and YMODE is its store.
//
// AB (K = 1, spmv_execute_axpby): the store writes alpha * sum + beta * y0
// (device.hpp axpby).  y0 is read with the very access the store uses -- the
// 16-byte row pair where y is 16-byte aligned, else two scalars -- and its
// load is issued before the diagonal loop, so it never trails the wave.
//
// DOT (K = 1, spmv_execute_dot): the lane's terms of the two sums it stores,
// added in row order, go into the workgroup's slot of `part` (device.hpp
// dot_block_store).  w[r], w[r + 1] are 8-byte loads (w's alignment is its
// own, YMODE describes y's), issued where y0's are.  No lane leaves early: one
// whose rows are >= m walks no diagonal, stores nothing, and still meets the
// reduction and its barrier.
template <int K, int UNROLL, bool LDSX, int YMODE, bool AB = false, bool DOT = false>
__device__ __forceinline__ void dia_body(int64_t m, int64_t mp, int64_t n, int n_diags,
                                         const int32_t *__restrict__ off, int32_t off_min, int32_t win, int32_t wpad,
                                         const double *__restrict__ val, const double *__restrict__ X, int64_t ldx,
                                         double *__restrict__ Y, int64_t ldy, int32_t group, double *xs,
                                         double alpha = 0.0, double beta = 0.0,
                                         const double *__restrict__ w = nullptr,
                                         double *__restrict__ part = nullptr) {
    static_assert(!AB || K == 1, "the axpby epilogue is single-vector");
    static_assert(!DOT || (K == 1 && !AB), "the dot epilogue is single-vector, without alpha and beta");
    const int64_t r0 = 2 * (int64_t)blockIdx.x * blockDim.x;
    const int64_t r = r0 + 2 * threadIdx.x;
    // group > 0 (DiaDev::group): blocks interleaved per group of `group`
    // consecutive blocks, diagonal by diagonal (the block's diagonal d at
    // stride gt*512); else one contiguous n_diags*4 KB block
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
        // out-of-range columns only meet zero-filled slots: any finite x works
        const int64_t c0 = r0 + off_min;
        for (int idx = threadIdx.x; idx < win * K; idx += blockDim.x) {
            const int i = idx / K, j = idx - i * K;
            xs[j * wpad + i] = xrow(c0 + i)[j];
        }
        __syncthreads();
    }
    if constexpr (!DOT) {
        if (r >= m) return;
    }
    const int nd = DOT && r >= m ? 0 : n_diags;  // the diagonals this lane walks
    f64x2 y0 = {0.0, 0.0};
    if constexpr (AB) {  // the store's own branches, below
        if (r + 1 < m && (reinterpret_cast<uintptr_t>(Y) & 15) == 0) {
            y0 = ld_stream2(Y + r);
        } else {
            y0.x = ld_stream(Y + r);
            if (r + 1 < m) y0.y = ld_stream(Y + r + 1);
        }
    }
    f64x2 wr = {0.0, 0.0};
    if constexpr (DOT) {
        if (w != nullptr && r < m) wr.x = w[r];
        if (w != nullptr && r + 1 < m) wr.y = w[r + 1];
    }
    double a0[K], a1[K];
#pragma unroll
    for (int j = 0; j < K; ++j) a0[j] = a1[j] = 0.0;
    const int lbase = 2 * threadIdx.x - off_min;  // LDS row of column r + 0
    // x_j of the lane's two rows on the diagonal at offset o: from the window ...
    auto xpair = [&](int32_t o, int j, double &g0, double &g1) {
        const double *q = xs + lbase + o;
        g0 = q[j * wpad];
        g1 = q[j * wpad + 1];
    };
    // ... or all K columns from global memory
    auto xrows = [&](int32_t o, double (&g0)[K], double (&g1)[K]) {
        const int64_t c = r + o;
        ld_row<K>(xrow(c), g0);
        ld_row<K>(xrow(c + 1), g1);
    };
    auto add = [&](f64x2 v, int j, double g0, double g1) {
        a0[j] = madd(v.x, g0, a0[j]);
        a1[j] = madd(v.y, g1, a1[j]);
    };
    // one diagonal, gathered and added (from the window column by column)
    auto step = [&](f64x2 v, int32_t o) {
        double g0[K], g1[K];
        if constexpr (!LDSX) xrows(o, g0, g1);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if constexpr (LDSX) xpair(o, j, g0[j], g1[j]);
            add(v, j, g0[j], g1[j]);
        }
    };
    int d = 0;
    for (; d + UNROLL <= nd; d += UNROLL) {
        f64x2 v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) v[u] = ld_stream2(vb + (int64_t)(d + u) * dstride);
        if constexpr (K == 1) {
            // the whole batch is gathered, then added: its UNROLL x pairs are
            // in flight together (the schedule config 4 was measured with)
            double g0[UNROLL][1], g1[UNROLL][1];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                if constexpr (LDSX) xpair(off[d + u], 0, g0[u][0], g1[u][0]);
                else xrows(off[d + u], g0[u], g1[u]);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) add(v[u], 0, g0[u][0], g1[u][0]);
        } else {
            // K = 8 cannot hold 2 K UNROLL gathered doubles: diagonal by diagonal
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) step(v[u], off[d + u]);
        }
    }
    for (; d < nd; ++d) step(ld_stream2(vb + (int64_t)d * dstride), off[d]);
    if constexpr (K == 1) {
        if constexpr (AB) {
            a0[0] = axpby(alpha, a0[0], beta, y0.x);
            a1[0] = axpby(alpha, a1[0], beta, y0.y);
        }
        // y is written once and not re-read: the row pair as one 16-byte
        // nontemporal store where y is 16-byte aligned (r is even)
        if (DOT && r >= m) {
            // no row: nothing to store
        } else if (r + 1 < m && (reinterpret_cast<uintptr_t>(Y) & 15) == 0) {
            f64x2 yv;
            yv.x = a0[0];
            yv.y = a1[0];
            // YMODE 1 (probe A/B): ordinary 16-byte stores (y lines stay in L2)
            if constexpr (YMODE == 1) *reinterpret_cast<f64x2 *>(Y + r) = yv;
            else __builtin_nontemporal_store(yv, reinterpret_cast<f64x2 *>(Y + r));
        } else {
            Y[r] = a0[0];
            if (r + 1 < m) Y[r + 1] = a1[0];
        }
        if constexpr (DOT) {
            double t = 0.0, q = 0.0;
            dot_add(t, q, r < m, w != nullptr, wr.x, a0[0]);
            dot_add(t, q, r + 1 < m, w != nullptr, wr.y, a1[0]);
            dot_block_store(t, q, part);
        }
    } else {
        st_row<K>(Y + r * ldy, a0);
        if (r + 1 < m) st_row<K>(Y + (r + 1) * ldy, a1);
    }
}

// the single vector: K = 1, the unit strides and the plane pitch fold away
template <int UNROLL, bool LDSX, int YMODE = 0>
__global__ __launch_bounds__(256) void dia_kernel(int64_t m, int64_t mp, int64_t n, int n_diags,
                                                  const int32_t *__restrict__ off, int32_t off_min, int32_t win,
                                                  const double *__restrict__ val,
                                                  const double *__restrict__ x,
                                                  double *__restrict__ y, int32_t group) {
    extern __shared__ double xs[];
    dia_body<1, UNROLL, LDSX, YMODE>(m, mp, n, n_diags, off, off_min, win, 0, val, x, 1, y, 1, group, xs);
}

// y = alpha * A x + beta * y: the single-vector body with the axpby epilogue
template <bool LDSX>
__global__ __launch_bounds__(256) void dia_axpby_kernel(int64_t m, int64_t mp, int64_t n, int n_diags,
                                                        const int32_t *__restrict__ off, int32_t off_min, int32_t win,
                                                        const double *__restrict__ val,
                                                        const double *__restrict__ x,
                                                        double *__restrict__ y, int32_t group, double alpha,
                                                        double beta) {
    extern __shared__ double xs[];
    dia_body<1, 8, LDSX, 0, true>(m, mp, n, n_diags, off, off_min, win, 0, val, x, 1, y, 1, group, xs, alpha, beta);
}

// y = A x with the rows' dot terms reduced into the plan's partials
template <bool LDSX>
__global__ __launch_bounds__(256) void dia_dot_kernel(int64_t m, int64_t mp, int64_t n, int n_diags,
                                                      const int32_t *__restrict__ off, int32_t off_min, int32_t win,
                                                      const double *__restrict__ val, const double *__restrict__ x,
                                                      double *__restrict__ y, int32_t group,
                                                      const double *__restrict__ w, double *__restrict__ part) {
    extern __shared__ double xs[];
    dia_body<1, 8, LDSX, 0, false, true>(m, mp, n, n_diags, off, off_min, win, 0, val, x, 1, y, 1, group, xs, 0.0, 0.0,
                                         w, part);
}

template <int K, bool LDSX>
__global__ __launch_bounds__(256) void dia_multi_kernel(int64_t m, int64_t mp, int64_t n, int n_diags,
                                                        const int32_t *__restrict__ off, int32_t off_min, int32_t win,
                                                        int32_t wpad, const double *__restrict__ val,
                                                        const double *__restrict__ X, int64_t ldx,
                                                        double *__restrict__ Y, int64_t ldy, int32_t group) {
    extern __shared__ double xs[];
    dia_body<K, 8, LDSX, 0>(m, mp, n, n_diags, off, off_min, win, wpad, val, X, ldx, Y, ldy, group, xs);
}

// LDS x window of a 512-row workgroup: 512 rows + diagonal span + 1
constexpr int kDiaMaxWin = 8192;  // doubles (64 KB)
// LDS requested per workgroup (KB), at least the window: > 80 KB = one per CU
constexpr int kDiaLdsKb = 96;
// LDS a workgroup may request on gfx950
constexpr size_t kDiaMaxLds = (size_t)160 << 10;

// the launch geometry of both kernels: 512-row workgroups and their x window
struct DiaGeom {
    dim3 blocks;
    int32_t off_min;
    int64_t win;
};
static DiaGeom dia_geom(const spmv_plan_s *p) {
    const DiaDev &d = p->dia;
    const int32_t off_min = d.off_host.front(), off_max = d.off_host.back();
    return {dim3((unsigned)(((p->m + 1) / 2 + 255) / 256)), off_min, 512 + (int64_t)off_max - off_min + 1};
}

// the launch's workgroups: the slots a dot launch writes (0: no stored diagonal)
int64_t dia_dot_blocks(const spmv_plan_s *p) {
    return p->m > 0 && p->dia.n_diags > 0 ? (int64_t)dia_geom(p).blocks.x : 0;
}

int launch_dia(const spmv_plan_s *p, const double *x, double *y, const Axpby *ab, const DotArgs *dot) {
    const DiaDev &d = p->dia;
    if (p->m == 0) return SPMV_SUCCESS;
    if (d.n_diags == 0) {  // no stored diagonal: y = 0 (axpby: alpha * (+0.0) + beta * y)
        if (ab) return launch_axpby(p, y, nullptr, *ab);
        SPMV_HIP_TRY(hipMemsetAsync(y, 0, sizeof(double) * (size_t)p->m, p->stream));
        return SPMV_SUCCESS;
    }
    const DiaGeom g = dia_geom(p);
    // The LDS request caps the workgroups per CU (kDiaLdsKb: one, 4 waves,
    // 32 KB of values in flight; the x window alone would allow 8): fewer
    // value streams keep the HBM channels out of the oversubscribed mode some
    // placements fall into.  Config 4, launch variants on the same plans:
    // 1.476-1.527 ms at 1 per CU, 1.500-1.594 at 2, 1.537-1.641 at 8
    // (profiles/round3/probe/dia_occupancy_paired_c4.jsonl,
    // dia_unroll_occupancy_c4.jsonl; profiles/round3/README.md)
    // Below the size at which DIA values take VMM handles (kDiaVmmMinBytes,
    // 256 MB) the launch keeps the x window's own occupancy: 64 diagonals,
    // same plans, 200 K rows (100 MB) 0.0166 ms uncapped vs 0.0188 capped;
    // 2 M rows (1 GB) 0.163 vs 0.159; 6 M rows (3 GB) 0.486 vs 0.466
    // (profiles/round4/probe/dia_cap_{200k,2m,6m}.jsonl)
    const bool big = (size_t)d.n_diags * (size_t)d.mp * sizeof(double) >= kDiaVmmMinBytes;
    int kb = big ? kDiaLdsKb : 0;
    if (const char *e = probe_env("SPMV_LAUNCH_DIA_LDS_KB")) kb = std::atoi(e);  // probe: occupancy A/B
    const int dbg = launch_dbg(0);  // probe: bit 0 = x from global memory, no LDS window
    const bool fits = g.win <= kDiaMaxWin;
    auto go = [&](auto kernel, bool ldsx, auto... ab_args) {
        const size_t lds = ldsx ? std::max(sizeof(double) * (size_t)g.win, (size_t)kb * 1024) : 0;
        hipLaunchKernelGGL(kernel, g.blocks, dim3(256), lds, p->stream, p->m, d.mp, p->n, d.n_diags, d.off, g.off_min,
                           ldsx ? (int32_t)g.win : 0, d.val, x, y, d.group, ab_args...);
    };
    if (dot) {  // the product's shape with the dot epilogue
        if (fits && !(dbg & 1)) go(dia_dot_kernel<true>, true, dot->w, dot->part);
        else go(dia_dot_kernel<false>, false, dot->w, dot->part);
        SPMV_HIP_TRY(hipGetLastError());
        return SPMV_SUCCESS;
    }
    if (ab) {  // the product's shape (8 diagonals in flight, nontemporal y) with the axpby epilogue
        if (fits && !(dbg & 1)) go(dia_axpby_kernel<true>, true, ab->alpha, ab->beta);
        else go(dia_axpby_kernel<false>, false, ab->alpha, ab->beta);
        SPMV_HIP_TRY(hipGetLastError());
        return SPMV_SUCCESS;
    }
    if (fits && !(dbg & 1)) go(dia_kernel<8, true>, true);
    else go(dia_kernel<8, false>, false);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

static int64_t dia_multi_wpad(int64_t win, int K) { return (win + 15) / 16 * 16 + 16 / K; }

// LDSX is taken where the staged window fits the LDS at this K and is no
// larger than what the lanes would otherwise read directly: staging moves
// win rows per workgroup, the global-x variant n_diags * 512 (64 diagonals,
// span 63: 576 against 32768, staged 2.9 x faster at K = 8; three diagonals
// 1500 apart: 3513 against 1536, staged 3.6 x / 4.8 x slower at K = 2 / 4 --
// profiles/multi_rhs/dia_variants.jsonl).
static bool dia_multi_use_lds(const spmv_plan_s *p, int64_t win, int K) {
    const bool fits = sizeof(double) * (size_t)dia_multi_wpad(win, K) * K <= kDiaMaxLds;
    bool lds = fits && win <= (int64_t)p->dia.n_diags * kDiaBlockRows;
    // probe build: 0 = global x, 1 = LDS wherever it fits (tools/multi_rhs_times.py --dia-variants)
    if (const char *e = probe_env("SPMV_LAUNCH_DIA_MULTI_LDSX")) lds = fits && std::atoi(e) != 0;
    return lds;
}

template <int K>
static void launch_dia_multi_k(const spmv_plan_s *p, const double *X, int64_t ldx, double *Y, int64_t ldy) {
    const DiaDev &d = p->dia;
    const DiaGeom g = dia_geom(p);
    if (dia_multi_use_lds(p, g.win, K)) {
        const int32_t wpad = (int32_t)dia_multi_wpad(g.win, K);
        // Only the window is requested.  launch_dia's 96-KB request for plans
        // above kDiaVmmMinBytes (one workgroup per CU: fewer HBM streams) costs
        // this kernel its LDS read rate, which needs more than one wave per
        // SIMD: 64 diagonals, 2 M rows, same plan, K = 2 / 4 / 8: 0.265 / 0.292 /
        // 0.524 ms with the request, 0.181 / 0.246 / 0.383 without
        // (profiles/multi_rhs/dia_variants.jsonl)
        int kb = 0;
        if (const char *e = probe_env("SPMV_LAUNCH_DIA_MULTI_LDS_KB")) kb = std::atoi(e);  // probe: occupancy A/B
        const size_t lds = std::min(kDiaMaxLds, std::max(sizeof(double) * (size_t)wpad * K, (size_t)kb * 1024));
        hipLaunchKernelGGL((dia_multi_kernel<K, true>), g.blocks, dim3(256), lds, p->stream, p->m, d.mp, p->n,
                           d.n_diags, d.off, g.off_min, (int32_t)g.win, wpad, d.val, X, ldx, Y, ldy, d.group);
    } else {
        hipLaunchKernelGGL((dia_multi_kernel<K, false>), g.blocks, dim3(256), 0, p->stream, p->m, d.mp, p->n,
                           d.n_diags, d.off, g.off_min, 0, 0, d.val, X, ldx, Y, ldy, d.group);
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

}  // namespace spmv
