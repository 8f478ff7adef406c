// k_transpose.hip -- the CSR of A^T from a CSR of A in HBM
// (spmv_csr_transpose_device; the plans of the transpose are built from its
// output).  Output row c holds A's entries of column c in ascending source
// entry index: a stable sort of the entries by column, byte for byte what
// transpose_csr_host (capi_create.cpp) gives.
//
//   1. keys = columns, ids = 0 .. nnz-1, stably radix-sorted (sort_pairs_u32:
//      the BIN builder's hipCUB instance, the significant bits of n - 1 only;
//      n = 1: no bits, no sort pass, the buffers stay as they were written),
//   2. the source row of every entry, expanded from row_ptr into the sort's
//      spare key buffer,
//   3. t_row_ptr cut out of the sorted keys (empty columns at the start, in
//      the middle and at the end are runs of equal pointers),
//   4. t_col / t_val / perm gathered through the sorted ids.  Values move as
//      64-bit words.
//
// No placement by an atomically advanced cursor anywhere: such a cursor is not
// stable.  The caller has validated the CSR (validate_csr_device), so every
// key is in [0, n).  Entry ids are 32-bit: nnz < 2^31 - 1.
#include "build_util.hpp"
#include "device.hpp"

namespace spmv {

namespace {

// entries a wave expands per step of tr_rowid_kernel: 64 lanes x kRowidSteps
constexpr int kRowidSteps = 8;
// a gap of at most this many columns is written by the lane that found it
constexpr int64_t kCutInline = 4;

__global__ void tr_keys_kernel(const int32_t *__restrict__ col, int64_t nnz, uint32_t *__restrict__ keys,
                               uint32_t *__restrict__ ids) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nnz; j += (int64_t)gridDim.x * blockDim.x) {
        keys[j] = (uint32_t)col[j];
        ids[j] = (uint32_t)j;
    }
}

// first row r in [lo, m) with rp[r + 1] > j (the row of entry j; j < rp[m])
__device__ __forceinline__ int64_t tr_row_of(const int64_t *__restrict__ rp, int64_t lo, int64_t m, int64_t j) {
    int64_t hi = m - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (rp[mid + 1] > j) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// rowid[j] = the row of source entry j.  A wave owns 64 * kRowidSteps
// consecutive entries; a lane searches row_ptr for its first entry, then walks
// forward (its entries ascend by 64), searching again when the walk crosses a
// long run of empty rows.
__global__ __launch_bounds__(256) void tr_rowid_kernel(const int64_t *__restrict__ rp, int64_t m, int64_t nnz,
                                                       uint32_t *__restrict__ rowid) {
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t base = wave * (64 * kRowidSteps);
    if (base >= nnz) return;
    int64_t r = -1;
    for (int s = 0; s < kRowidSteps; ++s) {
        const int64_t j = base + (int64_t)s * 64 + lane;
        if (j >= nnz) break;
        if (r < 0) {
            r = tr_row_of(rp, 0, m, j);
        } else {
            int steps = 0;
            while (rp[r + 1] <= j) {
                ++r;
                if (++steps == 16) {
                    r = tr_row_of(rp, r, m, j);
                    break;
                }
            }
        }
        rowid[j] = (uint32_t)r;
    }
}

// t_rp[c] = the first sorted position whose key is >= c, for c in [0, n].
// Boundary i (0 .. nnz) lies between keys[i - 1] (-1 before the first) and
// keys[i] (n past the last) and owns the columns (keys[i - 1], keys[i]]: none
// inside a column's run, one at its start, more across empty columns.  Short
// gaps are written by their lane; long ones by the whole wave, one at a time.
__global__ __launch_bounds__(256) void tr_cut_kernel(const uint32_t *__restrict__ keys, int64_t nnz, int64_t n,
                                                     int64_t *__restrict__ t_rp) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    for (int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base <= nnz; base += waves * 64) {
        const int64_t i = base + lane;
        int64_t prev = 0, cur = -1;  // (prev, cur] empty for lanes past the end
        if (i <= nnz) {
            prev = i > 0 ? (int64_t)keys[i - 1] : -1;
            cur = i < nnz ? (int64_t)keys[i] : n;
        }
        const int64_t gap = cur - prev;
        if (gap > 0 && gap <= kCutInline)
            for (int64_t c = prev + 1; c <= cur; ++c) t_rp[c] = i;
        uint64_t big = __ballot(gap > kCutInline);
        while (big) {
            const int l = __ffsll((unsigned long long)big) - 1;
            big &= big - 1;
            const int64_t p = __shfl(prev, l, 64), c1 = __shfl(cur, l, 64);
            for (int64_t c = p + 1 + lane; c <= c1; c += 64) t_rp[c] = base + l;
        }
    }
}

__global__ void tr_gather_kernel(const uint32_t *__restrict__ ids, const uint32_t *__restrict__ rowid, int64_t nnz,
                                 const uint64_t *__restrict__ val, int32_t *__restrict__ t_col,
                                 uint64_t *__restrict__ t_val, int64_t *__restrict__ perm) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t id = ids[i];
        t_col[i] = (int32_t)rowid[id];
        if (t_val) t_val[i] = val[id];
        if (perm) perm[i] = (int64_t)id;
    }
}

}  // namespace

int transpose_csr_device(int64_t m, int64_t n, int64_t nnz, const int64_t *d_rp, const int32_t *d_col,
                         const double *d_val, int64_t *d_t_rp, int32_t *d_t_col, double *d_t_val, int64_t *d_perm) {
    if (nnz >= (int64_t)INT32_MAX) {
        set_error("device transposition: nnz >= 2^31 - 1 is not supported (32-bit entry ids)");
        return SPMV_ERROR_NOT_SUPPORTED;
    }
    const hipStream_t st = nullptr;
    if (nnz == 0) {
        SPMV_HIP_TRY(hipMemsetAsync(d_t_rp, 0, 8 * (size_t)(n + 1), st));
        return build_sync(st, "device transposition");
    }
    DevScratch sc(st);
    uint32_t *k0, *k1, *v0, *v1;
    SPMV_RETURN_IF(sc.alloc(&k0, (size_t)nnz, "transposition sort keys"));
    SPMV_RETURN_IF(sc.alloc(&k1, (size_t)nnz, "transposition sort keys"));
    SPMV_RETURN_IF(sc.alloc(&v0, (size_t)nnz, "transposition sort ids"));
    SPMV_RETURN_IF(sc.alloc(&v1, (size_t)nnz, "transposition sort ids"));
    hipLaunchKernelGGL(tr_keys_kernel, dim3(grid_for(nnz)), dim3(256), 0, st, d_col, nnz, k0, v0);
    int bits = 0;  // significant bits of n - 1
    while (bits < 31 && ((int64_t)1 << bits) < n) ++bits;
    uint32_t *const kb[2] = {k0, k1}, *const vb[2] = {v0, v1};
    int cur = 0;
    SPMV_RETURN_IF(sort_pairs_u32(sc, kb, vb, nnz, bits, &cur));
    const uint32_t *keys = kb[cur], *ids = vb[cur];
    uint32_t *rowid = kb[cur ^ 1];  // the spare key buffer
    hipLaunchKernelGGL(tr_rowid_kernel, dim3(waves_grid((nnz + 64 * kRowidSteps - 1) / (64 * kRowidSteps))), dim3(256),
                       0, st, d_rp, m, nnz, rowid);
    hipLaunchKernelGGL(tr_cut_kernel, dim3(grid_for(nnz + 1)), dim3(256), 0, st, keys, nnz, n, d_t_rp);
    hipLaunchKernelGGL(tr_gather_kernel, dim3(grid_for(nnz)), dim3(256), 0, st, ids, (const uint32_t *)rowid, nnz,
                       (const uint64_t *)d_val, d_t_col, (uint64_t *)d_t_val, d_perm);
    return build_sync(st, "device transposition");
}

}  // namespace spmv
