// k_csr.hip -- CSR SpMV for gfx950: the opt_crs hot loop
// (src/opt_crs.cpp:57-69, `y[i] = sum_j val[j] * x[idx[j]]`) re-designed for
// wave64.
//
// One order of arithmetic: a group of L lanes (L | 64, or a workgroup's 256)
// owns a row and walks it from its 16-byte-aligned start a = ptr[i] & ~3 in
// chunks of 4 L entries; each lane takes ONE 16-byte load of 4 column indices
// and TWO 16-byte loads of 4 values (non-temporal: streamed once), so a wave
// instruction covers 1 KiB contiguous when rows are contiguous.  Entries
// outside [ptr[i], ptr[i+1]) never reach the sum.  Each lane sums its entries
// in order, then the group reduces with a fixed butterfly (β = 0, idempotent).
//
// Two shared pieces state that arithmetic:
//   csr_row_sum<STRIDE>             a lane's walk of one row (any length)
//   csr_batch_load / csr_batch_sum  one wave, U steps of 64 / L rows each of a
//                                   64-row slab: the loads of all U steps
//                                   issued together, no divergence on rows of
//                                   one chunk
// and three product kernels use them:
//   csr_slab2<L>   near-uniform rows: one wave per 64-row slab, x gathered
//                  from global memory, batch after batch (config 2)
//   csr_slabx<L>   the same slabs on rows near the diagonal: x from one LDS
//                  window per workgroup, the col / val stream one batch ahead
//                  of the sums (config 4)
//   csr_adaptive   skewed rows binned by length, all bins in one launch, a
//                  row per L-lane group or per workgroup (config 3; its ADD
//                  instance finishes the HYB / JDS overflow rows)
// Each has an *_axpby_kernel twin (spmv_execute_axpby: y = alpha A x + beta y
// in the store epilogue, csr_slab_store<AB> / csr_store_row<ADD, AB>; the
// row's writer loads its y0 before the row is streamed); alpha and beta are
// arguments of the twins only.
// Each also has a *_dot_kernel twin (spmv_execute_dot: the stored rows' terms
// w[r] * y[r] and y[r]^2 reduced into the workgroup's slot of the plan's
// partials, device.hpp dot_block_store; the writer loads its w[r] before the
// row is streamed).  In a dot twin no wave or lane leaves early: one without
// rows contributes +0.0 and still meets the reduction and its barrier.
//
// Algorithmic bytes per row: 12*nnz_i + rp bytes + 8 (y) and the
// x gathers (8*n total, counted once).
#include "device.hpp"
#include "internal.hpp"

namespace spmv {

// Values of a row-group plan (CsrDev::val_halves, CsrDev::lanes > 0): every
// aligned 256-entry chunk is laid as ELL's slots -- entries 4t, 4t+1 of the
// chunk at 2t, entries 4t+2, 4t+3 at 128 + 2t -- so the two 16-byte value
// loads of a lane's aligned 4-entry group j (at csr_vpos(j) and 128 later)
// each read whole lines across the wave instead of every other 16 bytes of
// every line (config 4: SS's values the same way, 3.08-3.26 -> 2.59-2.70 ms).
template <typename I>
__device__ __forceinline__ I csr_vpos(I j) {  // j % 4 == 0
    return (j & ~(I)255) + ((j & 255) >> 1);
}

// The lane's in-order partial sum of row [s, e): its 4-entry groups at
// (s & ~3) + 4 lane + 4 STRIDE i.  Entries outside [s, e) are masked: no x
// gather, no add.  vh: the values are stored in halves (csr_vpos).
template <int STRIDE>
__device__ __forceinline__ double csr_row_sum(int64_t s, int64_t e, int lane, const int32_t *__restrict__ col,
                                              const double *__restrict__ val, const double *__restrict__ x,
                                              bool vh) {
    double acc = 0.0;
    for (int64_t j = (s & ~(int64_t)3) + 4 * lane; j < e; j += 4 * STRIDE) {
        const i32x4 c = ld_stream4(col + j);
        const int64_t vj = vh ? csr_vpos(j) : j;
        const f64x2 v01 = ld_stream2(val + vj);
        const f64x2 v23 = ld_stream2(val + vj + (vh ? 128 : 2));
        const bool in0 = j + 0 >= s && j + 0 < e, in1 = j + 1 >= s && j + 1 < e;
        const bool in2 = j + 2 >= s && j + 2 < e, in3 = j + 3 >= s && j + 3 < e;
        // masked gathers: only entries of this row
        const double x0 = in0 ? ld_x(x, c.x) : 0.0;
        const double x1 = in1 ? ld_x(x, c.y) : 0.0;
        const double x2 = in2 ? ld_x(x, c.z) : 0.0;
        const double x3 = in3 ? ld_x(x, c.w) : 0.0;
        if (in0) acc = madd(v01.x, x0, acc);
        if (in1) acc = madd(v01.y, x1, acc);
        if (in2) acc = madd(v23.x, x2, acc);
        if (in3) acc = madd(v23.y, x3, acc);
    }
    return acc;
}

// ADD: y[yrow[row]] += sum (the HYB/JDS overflow, one writer per row);
// AB (spmv_execute_axpby): y[row] = alpha * sum + beta * y0, y0 = the y[row]
// the row's writer loaded before its walk (device.hpp axpby); otherwise
// y[row] = sum
template <bool ADD, bool AB = false>
__device__ __forceinline__ void csr_store_row(double *__restrict__ y, const int32_t *__restrict__ yrow, int64_t row,
                                              double sum, double alpha = 0.0, double beta = 0.0, double y0 = 0.0) {
    static_assert(!(ADD && AB), "the overflow add has no axpby form");
    if (ADD) {
        const int64_t yi = yrow[row];
        y[yi] = __dadd_rn(y[yi], sum);
    } else if (AB) {
        y[row] = axpby(alpha, sum, beta, y0);
    } else {
        y[row] = sum;
    }
}

// ---- the slab batch (csr_slab2, csr_slabx) ---------------------------------
// A wave owns a slab of 64 consecutive rows and sums it in L steps of R = 64 /
// L rows, row (st R + g) of the slab by lane group g in step st, exactly as
// csr_row_sum<L> and group_sum<L> sum it (same chunks, same order, same
// butterfly: both kernels and round 3's row-per-group csr_vec4<L> gave
// bit-identical y).  A batch is
// U steps whose col / val loads are issued before their x reads.  A
// long-lived wave replaces 64 / (256 / L) short ones and y leaves in one
// coalesced store per slab (config 4, same plans: csr_vec4<16> 2.82 -> 2.48
// ms, profiles/round4/probe/c4_csr_slab2_first.jsonl).

// O32 (CsrDev::off32: every slab's byte span and x's fit 31 / 32 bits): the
// col / val loads and the x gathers address a wave-uniform base plus a 32-bit
// byte offset (the global_load saddr form: no 64-bit address arithmetic per
// lane).
template <bool O32>
__device__ __forceinline__ const void *at_bytes(const void *base, int idx, int size) {
    if constexpr (O32) return (const char *)base + (uint32_t)idx * (uint32_t)size;
    else return (const char *)base + (int64_t)idx * size;
}

// A wave's col / val stream: entry positions are 32-bit, relative to base =
// the wave's first entry rounded down to 4 (a slab of 64 rows holds < 2^31
// entries).
template <bool O32>
struct CsrStream {
    const int32_t *cb;
    const double *vb;
    int vo, vstep;
    bool vh;
    __device__ __forceinline__ CsrStream(const int32_t *col, const double *val, int64_t base, bool halves)
        : cb(col + base), vh(halves) {
        const int64_t vbase = vh ? base & ~(int64_t)255 : base;
        vb = val + vbase;
        vo = (int)(base - vbase);
        vstep = vh ? 128 : 2;
    }
    // the aligned 4-entry group at j: 4 columns, values 0-1 and 2-3
    __device__ __forceinline__ void load(int j, i32x4 &c, f64x2 &v01, f64x2 &v23) const {
        c = ld_stream4((const int32_t *)at_bytes<O32>(cb, j, 4));
        const int vj = vh ? csr_vpos(j + vo) : j;
        v01 = ld_stream2((const double *)at_bytes<O32>(vb, vj, 8));
        v23 = ld_stream2((const double *)at_bytes<O32>(vb, vj + vstep, 8));
    }
};

template <int L, int U>
struct CsrBatch {
    i32x4 c[U];
    f64x2 a[U], b[U];
    int s[U], len[U];  // the row's start (relative to the stream's base) and length
    bool full;         // every row of the lane is one aligned chunk of its group
};

// Issue the loads of steps st .. st + U - 1.  rpl: lane t holds the start of
// the slab's row t, rpe: the slab's end; the row starts are exchanged by
// ds_bpermute.  Lanes past their row's end load the row's first chunk again
// (same lines, no new traffic) and every loaded column is a real column (plan
// creation validated them; the kPad tail is zero), so the loads and the x
// reads that follow are unconditional.
template <int L, int U, bool O32>
__device__ __forceinline__ void csr_batch_load(CsrBatch<L, U> &B, const CsrStream<O32> &A, int rpl, int rpe, int st) {
    constexpr int R = 64 / L;
    const int lane = threadIdx.x & 63, g = lane / L, gl = lane & (L - 1);
    B.full = true;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int li = (st + u) * R + g;
        const int s = __shfl(rpl, li, 64);
        const int nx = __shfl(rpl, (li + 1) & 63, 64);
        const int e = li == 63 ? rpe : nx;
        const int a0 = s & ~3;
        B.s[u] = s;
        B.len[u] = e - s;
        B.full = B.full && (s & 3) == 0 && B.len[u] == 4 * L;
        const int j0 = a0 + 4 * gl;
        A.load(j0 < e ? j0 : a0, B.c[u], B.a[u], B.b[u]);
    }
}

// Read the batch's x through xr(column) and write its U R row sums to ys (the
// wave's 64 sums in LDS).  A lane's four products of a step are formed first
// (madd's rounded multiply) and then added in entry order, so both add paths
// start from the same values.  When every row of the batch is one aligned chunk
// of its group (4 L entries from a 16-byte boundary: configs 2 and 4) the
// adds run unmasked; otherwise an entry outside [s, e) is dropped by a select
// on its add (one 32-bit compare per entry), and a row longer than one chunk
// takes the rest in order.  Group sums by DPP (group_sum_dpp: bit-identical
// to group_sum).
template <int L, int U, bool O32, typename XR>
__device__ __forceinline__ void csr_batch_sum(const CsrBatch<L, U> &B, const CsrStream<O32> &A, const XR &xr,
                                              double *ys, int st) {
    constexpr int R = 64 / L;
    const int lane = threadIdx.x & 63, g = lane / L, gl = lane & (L - 1);
    double pr[U][4];  // the lane's products, in entry order
#pragma unroll
    for (int u = 0; u < U; ++u) {
        pr[u][0] = __dmul_rn(B.a[u].x, xr(B.c[u].x));
        pr[u][1] = __dmul_rn(B.a[u].y, xr(B.c[u].y));
        pr[u][2] = __dmul_rn(B.b[u].x, xr(B.c[u].z));
        pr[u][3] = __dmul_rn(B.b[u].y, xr(B.c[u].w));
    }
    auto row_done = [&](int u, double acc) {
        acc = group_sum_dpp<L>(acc);
        if (gl == 0) ys[(st + u) * R + g] = acc;
    };
    if (__ballot(!B.full) == 0) {  // no lane with a partial row: unmasked adds
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double acc = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = __dadd_rn(acc, pr[u][q]);
            row_done(u, acc);
        }
        return;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        // the lane's first group: at j0, rel entries past the row's start
        const int j0 = (B.s[u] & ~3) + 4 * gl;
        const int rel = j0 - B.s[u];
        const int e = B.s[u] + B.len[u];  // the row's end
        double acc = 0.0, t;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            t = __dadd_rn(acc, pr[u][q]);
            acc = (unsigned)(rel + q) < (unsigned)B.len[u] ? t : acc;
        }
        // rows longer than one chunk of the group: the rest in order
        for (int jj = j0 + 4 * L; jj < e; jj += 4 * L) {
            i32x4 cc;
            f64x2 v01, v23;
            A.load(jj, cc, v01, v23);
            const double x0 = xr(cc.x), x1 = xr(cc.y), x2 = xr(cc.z), x3 = xr(cc.w);
            acc = madd(v01.x, x0, acc);
            t = madd(v01.y, x1, acc);
            acc = jj + 1 < e ? t : acc;
            t = madd(v23.x, x2, acc);
            acc = jj + 2 < e ? t : acc;
            t = madd(v23.y, x3, acc);
            acc = jj + 3 < e ? t : acc;
        }
        row_done(u, acc);
    }
}

// the wave's 64 row sums, written by its group leaders, leave LDS in one
// coalesced store.  AB (spmv_execute_axpby): lane t stores alpha * sum + beta *
// y0, y0 = the y[r0 + t] it loaded before the slab's batches (csr_slab_y0).
template <bool AB = false>
__device__ __forceinline__ void csr_slab_store(const double *ys, double *__restrict__ y, int64_t r0, int64_t m,
                                               double alpha = 0.0, double beta = 0.0, double y0 = 0.0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int lane = threadIdx.x & 63;
    if (r0 + lane < m) {
        if constexpr (AB) __builtin_nontemporal_store(axpby(alpha, ys[lane], beta, y0), y + r0 + lane);
        else __builtin_nontemporal_store(ys[lane], y + r0 + lane);
    }
}
// lane t's y0 of the slab at r0: indexed exactly as csr_slab_store's store
__device__ __forceinline__ double csr_slab_y0(const double *__restrict__ y, int64_t r0, int64_t m) {
    const int lane = threadIdx.x & 63;
    return r0 + lane < m ? ld_stream(y + r0 + lane) : 0.0;
}

// lane t's w of the slab at r0 (spmv_execute_dot), indexed as the store; w
// null: no w term, nothing read
__device__ __forceinline__ double csr_slab_w(const double *__restrict__ w, int64_t r0, int64_t m) {
    const int lane = threadIdx.x & 63;
    return w != nullptr && r0 + lane < m ? w[r0 + lane] : 0.0;
}
// ... and its terms of the y[r0 + t] csr_slab_store just stored from ys
__device__ __forceinline__ void csr_slab_dot(const double *ys, int64_t r0, int64_t m, bool have_w, double wr, double &t,
                                             double &q) {
    const int lane = threadIdx.x & 63;
    dot_add(t, q, r0 + lane < m, have_w, wr, ys[lane]);
}

// csr_slab2<L, U, O32>: one wave per slab; each batch is loaded, gathered
// from x in global memory and summed before the next one.
template <int L, typename RP, int U, bool O32>
__global__ __launch_bounds__(256) void csr_slab2_kernel(int64_t m, const RP *__restrict__ rp,
                                                        const int32_t *__restrict__ col,
                                                        const double *__restrict__ val,
                                                        const double *__restrict__ x, double *__restrict__ y, bool vh) {
    __shared__ double ysl[4][64];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
    const int lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wv) * 64;
    if (r0 >= m) return;  // wave-uniform
    const int64_t rl = r0 + lane;
    const int64_t base = (int64_t)rp[r0] & ~(int64_t)3;
    const int rpl = (int)((int64_t)rp[rl < m ? rl : m] - base);            // lane t: row r0 + t's start
    const int rpe = (int)((int64_t)rp[r0 + 64 < m ? r0 + 64 : m] - base);  // the slab's end
    const CsrStream<O32> A(col, val, base, vh);
    auto xg = [&](int c) -> double { return *(const double *)at_bytes<O32>(x, c, 8); };
    for (int st = 0; st < L; st += U) {
        CsrBatch<L, U> B;
        csr_batch_load(B, A, rpl, rpe, st);
        csr_batch_sum(B, A, xg, ysl[wv], st);
    }
    csr_slab_store(ysl[wv], y, r0, m);
}

// y = alpha * A x + beta * y: csr_slab2's frame around the same batches, with
// lane t's y0 loaded ahead of them and the axpby store.  (A frame of its own,
// not a shared body function: csr_slab2_kernel's code stays what it was --
// hoisting its frame into a function moved its instructions.)
template <int L, typename RP, int U, bool O32>
__global__ __launch_bounds__(256) void csr_slab2_axpby_kernel(int64_t m, const RP *__restrict__ rp,
                                                              const int32_t *__restrict__ col,
                                                              const double *__restrict__ val,
                                                              const double *__restrict__ x, double *__restrict__ y,
                                                              bool vh, double alpha, double beta) {
    __shared__ double ysl[4][64];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
    const int lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wv) * 64;
    if (r0 >= m) return;  // wave-uniform
    const int64_t rl = r0 + lane;
    const int64_t base = (int64_t)rp[r0] & ~(int64_t)3;
    const int rpl = (int)((int64_t)rp[rl < m ? rl : m] - base);
    const int rpe = (int)((int64_t)rp[r0 + 64 < m ? r0 + 64 : m] - base);
    const double y0 = csr_slab_y0(y, r0, m);
    const CsrStream<O32> A(col, val, base, vh);
    auto xg = [&](int c) -> double { return *(const double *)at_bytes<O32>(x, c, 8); };
    for (int st = 0; st < L; st += U) {
        CsrBatch<L, U> B;
        csr_batch_load(B, A, rpl, rpe, st);
        csr_batch_sum(B, A, xg, ysl[wv], st);
    }
    csr_slab_store<true>(ysl[wv], y, r0, m, alpha, beta, y0);
}

// y = A x with the dot terms: csr_slab2's frame around the same batches (a
// frame of its own, for csr_slab2_axpby_kernel's reason).  A wave past the
// last slab runs no batch and stores nothing; its lanes' +0.0 meet the
// workgroup's reduction like everyone's.
template <int L, typename RP, int U, bool O32>
__global__ __launch_bounds__(256) void csr_slab2_dot_kernel(int64_t m, const RP *__restrict__ rp,
                                                            const int32_t *__restrict__ col,
                                                            const double *__restrict__ val,
                                                            const double *__restrict__ x, double *__restrict__ y,
                                                            bool vh, const double *__restrict__ w,
                                                            double *__restrict__ part) {
    __shared__ double ysl[4][64];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform (SGPR)
    const int lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wv) * 64;
    double t = 0.0, q = 0.0;
    if (r0 < m) {  // wave-uniform
        const int64_t rl = r0 + lane;
        const int64_t base = (int64_t)rp[r0] & ~(int64_t)3;
        const int rpl = (int)((int64_t)rp[rl < m ? rl : m] - base);
        const int rpe = (int)((int64_t)rp[r0 + 64 < m ? r0 + 64 : m] - base);
        const double wr = csr_slab_w(w, r0, m);
        const CsrStream<O32> A(col, val, base, vh);
        auto xg = [&](int c) -> double { return *(const double *)at_bytes<O32>(x, c, 8); };
        for (int st = 0; st < L; st += U) {
            CsrBatch<L, U> B;
            csr_batch_load(B, A, rpl, rpe, st);
            csr_batch_sum(B, A, xg, ysl[wv], st);
        }
        csr_slab_store(ysl[wv], y, r0, m);
        csr_slab_dot(ysl[wv], r0, m, w != nullptr, wr, t, q);
    }
    dot_block_store(t, q, part);
}

// csr_slabx<L, U, S, O32>: csr_slab2 for matrices whose rows stay near the
// diagonal (banded, config 4).  A workgroup owns 256 S consecutive rows (each
// wave S consecutive 64-row slabs) and reads x over one column window
// [c0, c0 + win), the union of its S 256-row granules' windows
// (host- or device-computed, CsrDev::win0); it is staged into LDS once, so the x reads are LDS reads
// (lgkmcnt) and no longer share the in-order vmcnt queue with the col / val
// stream -- which lets the stream run one batch ahead: batch i + 1's loads
// (the next slab's first one included) are in flight while batch i's x reads
// and adds run (A / B ping-pong, as BIN's kernels), and the first batch is
// issued before the window is staged.  Lanes whose loaded entry lies
// outside the window (masked entries of a neighbouring row) read a clamped,
// in-window slot.
// DOT (spmv_execute_dot): a lane adds the terms of its S slabs' rows in slab
// order as each slab is stored and the workgroup reduces once, after the last.
template <int L, typename RP, int U, int S, bool O32, bool AB = false, bool DOT = false>
__device__ __forceinline__ void csr_slabx_body(int64_t m, const RP *__restrict__ rp, const int32_t *__restrict__ col,
                                               const double *__restrict__ val, const double *__restrict__ x,
                                               double *__restrict__ y, const int32_t *__restrict__ win0, int32_t win,
                                               int64_t n, bool vh, double *xs, double (*ysl)[64],
                                               double alpha = 0.0, double beta = 0.0,
                                               const double *__restrict__ w = nullptr,
                                               double *__restrict__ part = nullptr) {
    static_assert(!(AB && DOT), "the dot epilogue has no alpha and beta");
    constexpr int NB = L / U;   // batches per slab
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    // the wave's slabs: rows r0 + 64 k, k < S (r0 >= m: no rows, but the wave
    // still helps stage the window and meets the barrier)
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wv) * 64 * S;
    const int64_t rbase = r0 < m ? r0 : m;
    const int64_t base = (int64_t)rp[rbase] & ~(int64_t)3;
    int rpl[S], rpe[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const int64_t rk = r0 + 64 * k + lane, ek = r0 + 64 * (k + 1);
        rpl[k] = (int)((int64_t)rp[rk < m ? rk : m] - base);
        rpe[k] = (int)((int64_t)rp[ek < m ? ek : m] - base);
    }
    double y0[S];  // AB: lane t's y of each slab, loaded ahead of the stream
#pragma unroll
    for (int k = 0; k < S; ++k) {
        y0[k] = 0.0;
        if constexpr (AB) y0[k] = csr_slab_y0(y, r0 + 64 * k, m);
    }
    double wr[S], dt = 0.0, dq = 0.0;  // DOT: lane t's w of each slab, its running terms
#pragma unroll
    for (int k = 0; k < S; ++k) {
        wr[k] = 0.0;
        if constexpr (DOT) wr[k] = csr_slab_w(w, r0 + 64 * k, m);
    }
    const CsrStream<O32> A(col, val, base, vh);
    auto load = [&](CsrBatch<L, U> &B, int i) {  // batch i: slab i / NB, steps (i % NB) U ..
        csr_batch_load(B, A, rpl[i / NB], rpe[i / NB], (i % NB) * U);
    };
    // the workgroup's window: the union of its S granules' (win0: per
    // 256-row granule, INT32_MAX when a granule has no entries)
    const int64_t ng = (m + kCsrWinGroup - 1) / kCsrWinGroup;
    int64_t c0 = INT32_MAX;
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const int64_t gk = (int64_t)blockIdx.x * S + k;
        if (gk < ng) c0 = c0 < win0[gk] ? c0 : (int64_t)win0[gk];
    }
    if (c0 == INT32_MAX) c0 = 0;
    const uint32_t wmax = (uint32_t)win - 1;
    auto xw = [&](int c) -> double {
        const uint32_t i = (uint32_t)((int64_t)c - c0);
        return xs[i < wmax ? i : wmax];
    };
    auto compute = [&](const CsrBatch<L, U> &B, int i) {
        csr_batch_sum(B, A, xw, ysl[wv], (i % NB) * U);
        if (i % NB == NB - 1) {  // the slab is done; ysl[wv] is free again after the store
            double y0k = y0[0];
#pragma unroll
            for (int k = 1; k < S; ++k) y0k = i / NB == k ? y0[k] : y0k;
            csr_slab_store<AB>(ysl[wv], y, r0 + 64 * (i / NB), m, alpha, beta, y0k);
            if constexpr (DOT) {
                double wk = wr[0];
#pragma unroll
                for (int k = 1; k < S; ++k) wk = i / NB == k ? wr[k] : wk;
                csr_slab_dot(ysl[wv], r0 + 64 * (i / NB), m, w != nullptr, wk, dt, dq);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    };
    // the wave's batches: all S slabs while their rows exist
    const int nb = r0 >= m ? 0 : (int)std::min<int64_t>(S, (m - r0 + 63) / 64) * NB;
    CsrBatch<L, U> Ba, Bb;
    // window staging: its loads go out first, then the first batch's, so
    // both are in flight together
    constexpr int XT = 4;  // window values per thread held in flight (win <= 256 XT: one pass)
    double t[XT];
#pragma unroll
    for (int q = 0; q < XT; ++q) {
        const int i = threadIdx.x + q * 256;
        t[q] = i < win ? x[c0 + i < n ? c0 + i : n - 1] : 0.0;
    }
    if (nb > 0) load(Ba, 0);
#pragma unroll
    for (int q = 0; q < XT; ++q) {
        const int i = threadIdx.x + q * 256;
        if (i < win) xs[i] = t[q];
    }
    for (int i = threadIdx.x + XT * 256; i < win; i += 256) xs[i] = x[c0 + i < n ? c0 + i : n - 1];
    __syncthreads();
    for (int i = 0; i < nb; i += 2) {
        if (i + 1 < nb) load(Bb, i + 1);
        compute(Ba, i);
        if (i + 1 >= nb) break;
        if (i + 2 < nb) load(Ba, i + 2);
        compute(Bb, i + 1);
    }
    if constexpr (DOT) dot_block_store(dt, dq, part);
}

template <int L, typename RP, int U, int S, bool O32>
__global__ __launch_bounds__(256) void csr_slabx_kernel(int64_t m, const RP *__restrict__ rp,
                                                        const int32_t *__restrict__ col,
                                                        const double *__restrict__ val,
                                                        const double *__restrict__ x, double *__restrict__ y,
                                                        const int32_t *__restrict__ win0, int32_t win, int64_t n,
                                                        bool vh) {
    extern __shared__ double xs[];  // [win]
    __shared__ double ysl[4][64];
    csr_slabx_body<L, RP, U, S, O32>(m, rp, col, val, x, y, win0, win, n, vh, xs, ysl);
}

// y = alpha * A x + beta * y: the same body with the axpby epilogue
template <int L, typename RP, int U, int S, bool O32>
__global__ __launch_bounds__(256) void csr_slabx_axpby_kernel(int64_t m, const RP *__restrict__ rp,
                                                              const int32_t *__restrict__ col,
                                                              const double *__restrict__ val,
                                                              const double *__restrict__ x, double *__restrict__ y,
                                                              const int32_t *__restrict__ win0, int32_t win,
                                                              int64_t n, bool vh, double alpha, double beta) {
    extern __shared__ double xs[];  // [win]
    __shared__ double ysl[4][64];
    csr_slabx_body<L, RP, U, S, O32, true>(m, rp, col, val, x, y, win0, win, n, vh, xs, ysl, alpha, beta);
}

// y = A x with the dot terms: the same body with the dot epilogue
template <int L, typename RP, int U, int S, bool O32>
__global__ __launch_bounds__(256) void csr_slabx_dot_kernel(int64_t m, const RP *__restrict__ rp,
                                                            const int32_t *__restrict__ col,
                                                            const double *__restrict__ val,
                                                            const double *__restrict__ x, double *__restrict__ y,
                                                            const int32_t *__restrict__ win0, int32_t win, int64_t n,
                                                            bool vh, const double *__restrict__ w,
                                                            double *__restrict__ part) {
    extern __shared__ double xs[];  // [win]
    __shared__ double ysl[4][64];
    csr_slabx_body<L, RP, U, S, O32, false, true>(m, rp, col, val, x, y, win0, win, n, vh, xs, ysl, 0.0, 0.0, w, part);
}

// Adaptive CSR in ONE launch: workgroup ranges map to the length bins
// (blk_off), so all bins run concurrently instead of back to back; the bin
// test is workgroup-uniform (no divergence).  Bin b has L = kCsrBinLanes[b]
// lanes per row; the last bin is one workgroup per row.
struct CsrBinTable {
    int64_t blk_off[kCsrBins + 1];  // first workgroup of each bin, in launch order
    int64_t row_off[kCsrBins + 1];  // first row (in bin_rows) of each bin
};
// launch order: the longest rows first (their workgroups run longest), so
// the short-row bins fill in behind them instead of forming the tail
constexpr int kCsrLaunchOrder[kCsrBins] = {7, 6, 5, 4, 3, 2, 1, 0};

// DOT (spmv_execute_dot): the row's writer adds its terms to (dt, dq); a
// group past the bin's last row walks an empty row and stores nothing instead
// of leaving (the workgroup reduces after the bins' switch).
template <int L, typename RP, bool ADD, bool AB, bool DOT>
__device__ __forceinline__ void csr_rows_body(int64_t wg, int64_t nrows, const int32_t *__restrict__ rows,
                                              const RP *__restrict__ rp, const int32_t *__restrict__ col,
                                              const double *__restrict__ val, const double *__restrict__ x,
                                              double *__restrict__ y, const int32_t *__restrict__ yrow, double alpha,
                                              double beta, const double *__restrict__ w, double &dt, double &dq) {
    const int64_t g = (wg * 256 + threadIdx.x) / L;
    const int lane = threadIdx.x & (L - 1);
    if constexpr (!DOT) {
        if (g >= nrows) return;
    }
    const bool live = !DOT || g < nrows;
    const int64_t row = live ? (int64_t)rows[g] : 0;
    double y0 = 0.0;  // AB: the writer's y[row], loaded before the row's walk
    if constexpr (AB) {
        if (lane == 0) y0 = ld_stream(y + row);
    }
    double wr = 0.0;  // DOT: the writer's w[row], likewise
    if constexpr (DOT) {
        if (w != nullptr && live && lane == 0) wr = w[row];
    }
    const auto s = live ? rp[row] : (RP)0, e = live ? rp[row + 1] : (RP)0;
    const double acc = group_sum<L>(csr_row_sum<L>(s, e, lane, col, val, x, false));
    if (lane == 0 && live) csr_store_row<ADD, AB>(y, yrow, row, acc, alpha, beta, y0);
    if constexpr (DOT) dot_add(dt, dq, lane == 0 && live, w != nullptr, wr, acc);
}

template <typename RP, bool ADD, bool AB, bool DOT = false>
__device__ __forceinline__ void csr_adaptive_body(const CsrBinTable &t, const int32_t *__restrict__ rows,
                                                  const RP *__restrict__ rp, const int32_t *__restrict__ col,
                                                  const double *__restrict__ val, const double *__restrict__ x,
                                                  double *__restrict__ y, const int32_t *__restrict__ yrow,
                                                  double alpha, double beta, const double *__restrict__ w = nullptr,
                                                  double *__restrict__ dpart = nullptr) {
    static_assert(!DOT || (!ADD && !AB), "the dot epilogue has no add and no alpha and beta");
    __shared__ double part[4];
    double dt = 0.0, dq = 0.0;  // DOT: this thread's terms
    const int64_t blk = blockIdx.x;
    int k = 0;
    while (k < kCsrBins - 1 && blk >= t.blk_off[k + 1]) ++k;  // uniform
    const int b = kCsrLaunchOrder[k];
    const int64_t wg = blk - t.blk_off[k];
    const int32_t *br = rows + t.row_off[b];
    const int64_t n = t.row_off[b + 1] - t.row_off[b];
    switch (b) {
        case 0: csr_rows_body<1, RP, ADD, AB, DOT>(wg, n, br, rp, col, val, x, y, yrow, alpha, beta, w, dt, dq); break;
        case 1: csr_rows_body<2, RP, ADD, AB, DOT>(wg, n, br, rp, col, val, x, y, yrow, alpha, beta, w, dt, dq); break;
        case 2: csr_rows_body<4, RP, ADD, AB, DOT>(wg, n, br, rp, col, val, x, y, yrow, alpha, beta, w, dt, dq); break;
        case 3: csr_rows_body<8, RP, ADD, AB, DOT>(wg, n, br, rp, col, val, x, y, yrow, alpha, beta, w, dt, dq); break;
        case 4: csr_rows_body<16, RP, ADD, AB, DOT>(wg, n, br, rp, col, val, x, y, yrow, alpha, beta, w, dt, dq); break;
        case 5: csr_rows_body<32, RP, ADD, AB, DOT>(wg, n, br, rp, col, val, x, y, yrow, alpha, beta, w, dt, dq); break;
        case 6: csr_rows_body<64, RP, ADD, AB, DOT>(wg, n, br, rp, col, val, x, y, yrow, alpha, beta, w, dt, dq); break;
        default: {
            // one workgroup per row: four wave sums added in wave order
            const int64_t row = br[wg];
            double y0 = 0.0;
            if constexpr (AB) {
                if (threadIdx.x == 0) y0 = ld_stream(y + row);
            }
            double wr = 0.0;
            if constexpr (DOT) {
                if (w != nullptr && threadIdx.x == 0) wr = w[row];
            }
            const double acc =
                group_sum<64>(csr_row_sum<256>(rp[row], rp[row + 1], (int)threadIdx.x, col, val, x, false));
            if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
            __syncthreads();
            if constexpr (DOT) {  // thread 0 holds the row's term
                const double sum = __dadd_rn(__dadd_rn(part[0], part[1]), __dadd_rn(part[2], part[3]));
                if (threadIdx.x == 0) csr_store_row<ADD, AB>(y, yrow, row, sum, alpha, beta, y0);
                dot_add(dt, dq, threadIdx.x == 0, w != nullptr, wr, sum);
            } else if (threadIdx.x == 0)
                csr_store_row<ADD, AB>(y, yrow, row,
                                       __dadd_rn(__dadd_rn(part[0], part[1]), __dadd_rn(part[2], part[3])), alpha,
                                       beta, y0);
        }
    }
    if constexpr (DOT) dot_block_store(dt, dq, dpart);
}

template <typename RP, bool ADD>
__global__ __launch_bounds__(256) void csr_adaptive_kernel(CsrBinTable t, const int32_t *__restrict__ rows,
                                                           const RP *__restrict__ rp,
                                                           const int32_t *__restrict__ col,
                                                           const double *__restrict__ val,
                                                           const double *__restrict__ x, double *__restrict__ y,
                                                           const int32_t *__restrict__ yrow) {
    csr_adaptive_body<RP, ADD, false>(t, rows, rp, col, val, x, y, yrow, 0.0, 0.0);
}

// y = alpha * A x + beta * y: the same body with the axpby epilogue
template <typename RP>
__global__ __launch_bounds__(256) void csr_adaptive_axpby_kernel(CsrBinTable t, const int32_t *__restrict__ rows,
                                                                 const RP *__restrict__ rp,
                                                                 const int32_t *__restrict__ col,
                                                                 const double *__restrict__ val,
                                                                 const double *__restrict__ x, double *__restrict__ y,
                                                                 double alpha, double beta) {
    csr_adaptive_body<RP, false, true>(t, rows, rp, col, val, x, y, nullptr, alpha, beta);
}

// y = A x with the dot terms: the same body with the dot epilogue
template <typename RP>
__global__ __launch_bounds__(256) void csr_adaptive_dot_kernel(CsrBinTable t, const int32_t *__restrict__ rows,
                                                               const RP *__restrict__ rp,
                                                               const int32_t *__restrict__ col,
                                                               const double *__restrict__ val,
                                                               const double *__restrict__ x, double *__restrict__ y,
                                                               const double *__restrict__ w,
                                                               double *__restrict__ part) {
    csr_adaptive_body<RP, false, false, true>(t, rows, rp, col, val, x, y, nullptr, 0.0, 0.0, w, part);
}

// the bins' workgroup ranges, in launch order (bin_off: host offsets)
static CsrBinTable csr_bin_table(const int64_t *bin_off) {
    CsrBinTable t;
    t.blk_off[0] = 0;
    for (int b = 0; b <= kCsrBins; ++b) t.row_off[b] = bin_off[b];
    for (int k = 0; k < kCsrBins; ++k) {
        const int b = kCsrLaunchOrder[k];
        const int64_t n = bin_off[b + 1] - bin_off[b];
        const int L = kCsrBinLanes[b];
        t.blk_off[k + 1] = t.blk_off[k] + (L >= 256 ? n : (n * L + 255) / 256);
    }
    return t;
}

// one launch of the adaptive kernel over length bins
template <typename RP, bool ADD>
static int launch_adaptive(const spmv_plan_s *p, const int64_t *bin_off, const int32_t *bin_rows, const RP *rp,
                           const int32_t *col, const double *val, const double *x, double *y,
                           const int32_t *yrow, const Axpby *ab = nullptr, const DotArgs *dot = nullptr) {
    const CsrBinTable t = csr_bin_table(bin_off);
    if (t.blk_off[kCsrBins] == 0) return SPMV_SUCCESS;
    if constexpr (!ADD) {
        if (dot) {
            hipLaunchKernelGGL((csr_adaptive_dot_kernel<RP>), dim3((unsigned)t.blk_off[kCsrBins]), dim3(256), 0,
                               p->stream, t, bin_rows, rp, col, val, x, y, dot->w, dot->part);
            SPMV_HIP_TRY(hipGetLastError());
            return SPMV_SUCCESS;
        }
        if (ab) {
            hipLaunchKernelGGL((csr_adaptive_axpby_kernel<RP>), dim3((unsigned)t.blk_off[kCsrBins]), dim3(256), 0,
                               p->stream, t, bin_rows, rp, col, val, x, y, ab->alpha, ab->beta);
            SPMV_HIP_TRY(hipGetLastError());
            return SPMV_SUCCESS;
        }
    }
    hipLaunchKernelGGL((csr_adaptive_kernel<RP, ADD>), dim3((unsigned)t.blk_off[kCsrBins]), dim3(256), 0, p->stream,
                       t, bin_rows, rp, col, val, x, y, yrow);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

// launch-time shape of the row-parallel CSR kernels: csr_slabx where the plan
// has x windows (banded rows), else csr_slab2, with U = min(4, L) steps per
// batch.  Config 4 (16 lanes), same plans: csr_vec4 (round 3's row per group)
// 2.80-2.87, csr_slab2 U = 1 / 2 / 4 / 8 2.64 / 2.55 / 2.49 / 2.54 ms,
// csr_slabx U = 4 2.41-2.54 ms against csr_slab2's 2.54-2.62 on the same
// plans; config 2 (gather-bound) within 1 % (round 4 A/Bs,
// profiles/round4/probe/c4_csr_slab2_first.jsonl, c4_csr_slabx_s1.jsonl,
// c4_csr_slabx_pairs.jsonl, c2_csr_slab2_slabx.jsonl).
constexpr int kCsrBatchSteps = 4;  // slab: steps whose loads are issued together

template <int L, typename RP>
static void launch_slab(const spmv_plan_s *p, const double *x, double *y, const Axpby *ab, const DotArgs *dot) {
    constexpr int UU = kCsrBatchSteps < L ? kCsrBatchSteps : L;
    constexpr int S = kCsrSlabsPerWave;  // granules (64-row slabs per wave) per workgroup
    const int64_t waves = (p->m + 63) / 64;
    const CsrDev &c = p->csr;
    if (c.win0) {  // x window in LDS, stream one batch ahead
        const unsigned grid = (unsigned)((p->m + 256 * S - 1) / (256 * S));
        auto go = [&](auto kern, auto... ab_args) {
            hipLaunchKernelGGL(kern, dim3(grid), dim3(256), sizeof(double) * (size_t)c.win, p->stream, p->m,
                               (const RP *)c.row_ptr, c.col, c.val, x, y, c.win0, c.win, p->n, c.val_halves,
                               ab_args...);
        };
        // 32-bit offsets span the wave's S slabs (off32 is per single slab)
        const bool o32 = c.off32 && (S == 1 || (int64_t)S * c.slab_max + 512 < ((int64_t)1 << 28));
        if (dot) {
            if (o32) go(csr_slabx_dot_kernel<L, RP, UU, S, true>, dot->w, dot->part);
            else go(csr_slabx_dot_kernel<L, RP, UU, S, false>, dot->w, dot->part);
            return;
        }
        if (ab) {
            if (o32) go(csr_slabx_axpby_kernel<L, RP, UU, S, true>, ab->alpha, ab->beta);
            else go(csr_slabx_axpby_kernel<L, RP, UU, S, false>, ab->alpha, ab->beta);
        } else if (o32) {
            go(csr_slabx_kernel<L, RP, UU, S, true>);
        } else {
            go(csr_slabx_kernel<L, RP, UU, S, false>);
        }
        return;
    }
    auto go = [&](auto kern, auto... ab_args) {
        hipLaunchKernelGGL(kern, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, p->stream, p->m,
                           (const RP *)c.row_ptr, c.col, c.val, x, y, c.val_halves, ab_args...);
    };
    if (dot) {
        if (c.off32) go(csr_slab2_dot_kernel<L, RP, UU, true>, dot->w, dot->part);
        else go(csr_slab2_dot_kernel<L, RP, UU, false>, dot->w, dot->part);
        return;
    }
    if (ab) {
        if (c.off32) go(csr_slab2_axpby_kernel<L, RP, UU, true>, ab->alpha, ab->beta);
        else go(csr_slab2_axpby_kernel<L, RP, UU, false>, ab->alpha, ab->beta);
    } else if (c.off32) {
        go(csr_slab2_kernel<L, RP, UU, true>);
    } else {
        go(csr_slab2_kernel<L, RP, UU, false>);
    }
}

template <int L, typename RP>
static int launch_csr_t(const spmv_plan_s *p, int64_t nrows, const double *x, double *y, const Axpby *ab,
                       const DotArgs *dot) {
    if (nrows == 0) return SPMV_SUCCESS;
    launch_slab<L, RP>(p, x, y, ab, dot);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

template <typename RP>
static int launch_csr_lanes(const spmv_plan_s *p, int lanes, int64_t nrows, const double *x, double *y,
                            const Axpby *ab, const DotArgs *dot) {
    switch (lanes) {
        case 1: return launch_csr_t<1, RP>(p, nrows, x, y, ab, dot);
        case 2: return launch_csr_t<2, RP>(p, nrows, x, y, ab, dot);
        case 4: return launch_csr_t<4, RP>(p, nrows, x, y, ab, dot);
        case 8: return launch_csr_t<8, RP>(p, nrows, x, y, ab, dot);
        case 16: return launch_csr_t<16, RP>(p, nrows, x, y, ab, dot);
        case 32: return launch_csr_t<32, RP>(p, nrows, x, y, ab, dot);
        case 64: return launch_csr_t<64, RP>(p, nrows, x, y, ab, dot);
        default: set_error("csr lanes must be a power of two in [1,64]"); return SPMV_ERROR_INVALID_VALUE;
    }
}

template <typename RP>
static int launch_csr_rp(const spmv_plan_s *p, const double *x, double *y, const Axpby *ab, const DotArgs *dot) {
    const CsrDev &c = p->csr;
    if (!c.bin_rows) return launch_csr_lanes<RP>(p, c.lanes, p->m, x, y, ab, dot);
    // adaptive: every bin in one launch (workgroup ranges per bin)
    return launch_adaptive<RP, false>(p, c.bin_off, c.bin_rows, (const RP *)c.row_ptr, c.col, c.val, x, y, nullptr,
                                      ab, dot);
}

// the workgroups of the plan's dot launch: the slots it writes (0: nothing
// stored, no launch)
int64_t csr_dot_blocks(const spmv_plan_s *p) {
    const CsrDev &c = p->csr;
    if (p->nnz == 0 || p->m == 0) return 0;
    if (c.bin_rows) return csr_bin_table(c.bin_off).blk_off[kCsrBins];
    if (c.win0) return (p->m + 256 * kCsrSlabsPerWave - 1) / (256 * kCsrSlabsPerWave);
    return ((p->m + 63) / 64 + 3) / 4;
}

int launch_csr(const spmv_plan_s *p, const double *x, double *y, const Axpby *ab, const DotArgs *dot) {
    if (p->nnz == 0) {  // no entries: y = 0 without touching x (x may be NULL when n == 0)
        if (p->m && ab) return launch_axpby(p, y, nullptr, *ab);  // alpha * (+0.0) + beta * y
        if (p->m) SPMV_HIP_TRY(hipMemsetAsync(y, 0, sizeof(double) * (size_t)p->m, p->stream));
        return SPMV_SUCCESS;
    }
    return p->csr.rp64 ? launch_csr_rp<int64_t>(p, x, y, ab, dot) : launch_csr_rp<int32_t>(p, x, y, ab, dot);
}

// HYB / JDS overflow: the adaptive kernel over the overflow rows binned by
// their overflow length, y[row] += sum.  Every plan with overflow rows has
// the bins (overflow_upload_index, formats.cpp); none: no workgroups, no launch.
int launch_hyb_overflow(const spmv_plan_s *p, const double *x, double *y) {
    const HybDev &h = p->hyb;
    return launch_adaptive<int64_t, true>(p, h.bin_off, h.bin_rows, h.row_ptr, h.col, h.val, x, y, h.rows);
}

}  // namespace spmv
