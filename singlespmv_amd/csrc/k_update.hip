// k_update.hip -- value refresh: new values on a plan's fixed sparsity pattern
// (spmv_plan_update_prepare / spmv_plan_update_values, include/spmv_hip.h).
//
// Prepare: a shadow plan built from the same pattern with values 1 .. nnz
// tells, slot by slot, which CSR entry every value slot of the layout holds
// (0.0 = padding).  map_from_shadow_kernel turns each shadow value array into
// an integer map (0 = padding, else entry + 1) and validates it: every entry
// must be hit exactly once over all value arrays (a bit per entry, set with
// atomicOr; the count of filled slots must be nnz), and no slot the pattern
// leaves empty may hold a non-zero value in the plan.
//
// Update: update_gather_kernel, dst[s] = map[s] ? f(src[map[s] - 1]) : pad,
// the gather form -- the map and dst stream (4 + 8 bytes per slot, 16-byte map
// loads, 16-byte nontemporal stores: the next reader is an SpMV that streams
// the array from HBM), the 8-byte reads of src are near-sequential for CSR,
// ELL, SS, DIA, COO and the HYB overflow and random for BIN's strip-major Mul
// order and CSS's column-sorted lists.  The scatter form would make the
// 8-byte writes random instead.
#include <algorithm>
#include <string>
#include <vector>

#include "build_util.hpp"
#include "device.hpp"

namespace spmv {

namespace {

typedef int64_t i64x2 __attribute__((ext_vector_type(2)));

constexpr unsigned kUpdMaxBlocks = 2048;  // 256 CUs x 8 workgroups; the rest is the grid-stride loop

inline unsigned upd_grid(int64_t items) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, kUpdMaxBlocks));
}

// four consecutive map entries (16 bytes of int32, 32 bytes of int64), streamed
__device__ __forceinline__ void ld_map4(const int32_t *m, int64_t (&e)[4]) {
    const i32x4 t = ld_stream4(m);
    e[0] = t.x, e[1] = t.y, e[2] = t.z, e[3] = t.w;
}
__device__ __forceinline__ void ld_map4(const int64_t *m, int64_t (&e)[4]) {
    const i64x2 a = __builtin_nontemporal_load(reinterpret_cast<const i64x2 *>(m));
    const i64x2 b = __builtin_nontemporal_load(reinterpret_cast<const i64x2 *>(m + 2));
    e[0] = a.x, e[1] = a.y, e[2] = b.x, e[3] = b.y;
}

// what the builder stores for a value v: v, or DIA's 0.0 + v (its fill adds
// each entry into a zeroed slot: -0.0 becomes +0.0)
template <bool DIA_ADD>
__device__ __forceinline__ double stored(double v) {
    if constexpr (DIA_ADD) return __dadd_rn(0.0, v);
    else return v;
}

// dst[s] = map[s] ? f(src[map[s] - 1]) : pad for s in [0, slots).  A lane
// takes four consecutive slots: a wave reads 1 KiB (int32) of the map per
// step and writes 2 KiB of dst as two 16-byte stores per lane; the last
// slots % 4 slots are scalar (the arrays start 16-byte aligned, so there is
// no head).  src needs the alignment of a double only.
template <typename MapT, bool DIA_ADD>
__global__ __launch_bounds__(256) void update_gather_kernel(const MapT *__restrict__ map,
                                                            const double *__restrict__ src,
                                                            double *__restrict__ dst, int64_t slots, double pad) {
    const int64_t quads = slots >> 2;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = tid; q < quads; q += stride) {
        int64_t e[4];
        ld_map4(map + 4 * q, e);
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = e[k] ? stored<DIA_ADD>(src[e[k] - 1]) : pad;
        f64x2 lo, hi;
        lo.x = v[0], lo.y = v[1], hi.x = v[2], hi.y = v[3];
        __builtin_nontemporal_store(lo, reinterpret_cast<f64x2 *>(dst + 4 * q));
        __builtin_nontemporal_store(hi, reinterpret_cast<f64x2 *>(dst + 4 * q + 2));
    }
    const int64_t s = 4 * quads + tid;  // the tail: slots % 4 < 4 lanes of the first wave
    if (s < slots) {
        const int64_t e = map[s];
        dst[s] = e ? stored<DIA_ADD>(src[e - 1]) : pad;
    }
}

// The same gather for DIA's blocked layout (slot ((b * nd + d) * 512 + rl) of
// block b, diagonal d, local row rl; DiaDev, group = 0), visited so that the
// reads of src coalesce: a row's entries are consecutive in the CSR, so the
// slots of ONE row over consecutive diagonals read consecutive src, while
// the slots of one diagonal (consecutive rows) read src a whole row apart.
// A workgroup takes 16 diagonals of one block: lane (dl, rq) owns the 4 rows
// of row quad rq of diagonal d0 + dl -- per wave instruction 16 diagonals x
// 4 row quads: map loads in 64-byte pieces, stores in 128-byte pieces, and
// each of a lane's 4 gathers lands in the up to 128 contiguous bytes its 16
// diagonals share.
template <typename MapT>
__global__ __launch_bounds__(256) void update_gather_dia_kernel(const MapT *__restrict__ map,
                                                                const double *__restrict__ src,
                                                                double *__restrict__ dst, int nd, int64_t nblk,
                                                                double pad) {
    const int dl = threadIdx.x & 15, rq0 = threadIdx.x >> 4;
    const int64_t dgroups = (nd + 15) / 16;
    for (int64_t w = blockIdx.x; w < nblk * dgroups; w += gridDim.x) {
        const int64_t b = w / dgroups;
        const int d = (int)(w - b * dgroups) * 16 + dl;
        if (d >= nd) continue;
        const int64_t base = (b * nd + d) * kDiaBlockRows;
#pragma unroll 2
        for (int rq = rq0; rq < kDiaBlockRows / 4; rq += 16) {
            const int64_t s = base + 4 * rq;
            int64_t e[4];
            ld_map4(map + s, e);
            double v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = e[k] ? stored<true>(src[e[k] - 1]) : pad;
            f64x2 lo, hi;
            lo.x = v[0], lo.y = v[1], hi.x = v[2], hi.y = v[3];
            __builtin_nontemporal_store(lo, reinterpret_cast<f64x2 *>(dst + s));
            __builtin_nontemporal_store(hi, reinterpret_cast<f64x2 *>(dst + s + 2));
        }
    }
}

// counters of the validation, summed over every value array of the plan
enum { kCntFilled = 0, kCntBad = 1, kCntStray = 2, kCntN = 3 };

// shadow value array -> map.  A shadow slot holds 0.0 (padding) or entry + 1
// (the shadow was built from values 1 .. nnz, exact below 2^53).  Counted:
// filled slots; bad slots (no integer in [1, nnz] -- several entries added
// into one slot -- or an entry hit before: `seen` holds one bit per entry);
// stray slots (padding under the pattern, yet a non-zero bit pattern in the
// plan's array `cur`: the plan was built from another pattern).
template <typename MapT>
__global__ __launch_bounds__(256) void map_from_shadow_kernel(const double *__restrict__ shadow,
                                                              const double *__restrict__ cur, int64_t slots,
                                                              int64_t nnz, MapT *__restrict__ map,
                                                              uint32_t *__restrict__ seen,
                                                              unsigned long long *__restrict__ cnt) {
    unsigned long long filled = 0, bad = 0, stray = 0;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (int64_t)gridDim.x * blockDim.x) {
        const double v = shadow[s];
        int64_t e = 0;
        if (v == 0.0) {
            stray += __double_as_longlong(cur[s]) != 0;
        } else if (v >= 1.0 && v <= (double)nnz && (double)(int64_t)v == v) {
            e = (int64_t)v;
            const uint32_t bit = 1u << ((e - 1) & 31);
            const uint32_t old = atomicOr(seen + ((e - 1) >> 5), bit);
            ++filled;
            bad += (old & bit) != 0;
        } else {
            ++bad;
        }
        map[s] = (MapT)e;
    }
    for (int o = 32; o > 0; o >>= 1) {
        filled += __shfl_xor(filled, o, 64);
        bad += __shfl_xor(bad, o, 64);
        stray += __shfl_xor(stray, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (filled) atomicAdd(cnt + kCntFilled, filled);
        if (bad) atomicAdd(cnt + kCntBad, bad);
        if (stray) atomicAdd(cnt + kCntStray, stray);
    }
}

__global__ __launch_bounds__(256) void iota_values_kernel(double *__restrict__ val, int64_t nnz) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * blockDim.x)
        val[i] = (double)(i + 1);
}

template <typename MapT>
void launch_gather(const spmv_plan_s *p, const UpdArray &a, const double *d_val) {
    const unsigned grid = upd_grid(a.slots >> 2);
    const DiaDev &d = p->dia;
    const int64_t nblk = d.mp / kDiaBlockRows;
    if (p->format == SPMV_FORMAT_DIA && d.group == 0 && d.n_diags > 0 &&
        a.slots == (int64_t)d.n_diags * nblk * kDiaBlockRows) {
        const int64_t work = nblk * ((d.n_diags + 15) / 16);
        hipLaunchKernelGGL(update_gather_dia_kernel<MapT>, dim3((unsigned)std::min<int64_t>(work, 4 * kUpdMaxBlocks)),
                           dim3(256), 0, p->stream, (const MapT *)a.map, d_val, a.dst, d.n_diags, nblk, 0.0);
        return;
    }
    if (p->upd.dia_add)
        hipLaunchKernelGGL((update_gather_kernel<MapT, true>), dim3(grid), dim3(256), 0, p->stream,
                           (const MapT *)a.map, d_val, a.dst, a.slots, 0.0);
    else
        hipLaunchKernelGGL((update_gather_kernel<MapT, false>), dim3(grid), dim3(256), 0, p->stream,
                           (const MapT *)a.map, d_val, a.dst, a.slots, 0.0);
}

const char kWrongPattern[] =
    "spmv_plan_update_prepare: the pattern does not reproduce the plan's layout (not the CSR the plan was created from)";

}  // namespace

int launch_iota_values(hipStream_t st, double *val, int64_t nnz) {
    if (nnz <= 0) return SPMV_SUCCESS;
    hipLaunchKernelGGL(iota_values_kernel, dim3(upd_grid(nnz)), dim3(256), 0, st, val, nnz);
    SPMV_HIP_TRY(hipGetLastError());
    return SPMV_SUCCESS;
}

int launch_update_values(const spmv_plan_s *p, const double *d_val) {
    for (const UpdArray &a : p->upd.arrays) {
        if (a.slots <= 0) continue;
        if (p->upd.wide) launch_gather<int64_t>(p, a, d_val);
        else launch_gather<int32_t>(p, a, d_val);
        SPMV_HIP_TRY(hipGetLastError());
    }
    return SPMV_SUCCESS;
}

int update_prepare_from_shadow(spmv_plan_s *p, const spmv_plan_s *shadow) {
    // 1. same format, same array list, same digests of every non-value array
    std::vector<ArrayRef> pa, sa;
    SPMV_RETURN_IF(plan_arrays(p, pa));
    SPMV_RETURN_IF(plan_arrays(shadow, sa));
    bool same = p->format == shadow->format && pa.size() == sa.size();
    for (size_t k = 0; same && k < pa.size(); ++k)
        same = std::string(pa[k].name) == sa[k].name && pa[k].bytes == sa[k].bytes;
    if (same) {
        // the value arrays are skipped: hash the others only
        std::vector<ArrayRef> pn, sn;
        for (size_t k = 0; k < pa.size(); ++k)
            if (!is_value_array(pa[k].name)) {
                pn.push_back(pa[k]);
                sn.push_back(sa[k]);
            }
        std::vector<uint64_t> pd, sd;
        SPMV_RETURN_IF(plan_digests(p, pn, pd));
        SPMV_RETURN_IF(plan_digests(shadow, sn, sd));
        same = pd == sd;
    }
    if (!same) {
        set_error(kWrongPattern);
        return SPMV_ERROR_INVALID_VALUE;
    }
    // 2. the maps: plan-owned plain allocations (4 or 8 bytes per value slot)
    UpdState u;
    u.wide = p->nnz >= (int64_t)INT32_MAX;
    u.dia_add = p->format == SPMV_FORMAT_DIA;
    int st = SPMV_SUCCESS;
    for (size_t k = 0; k < pa.size() && st == SPMV_SUCCESS; ++k) {
        if (!is_value_array(pa[k].name)) continue;
        if (reinterpret_cast<uintptr_t>(pa[k].ptr) & 15) {
            set_error("spmv_plan_update_prepare: a value array of the plan is not 16-byte aligned");
            st = SPMV_ERROR_INVALID_VALUE;
            break;
        }
        UpdArray a;
        a.dst = (double *)const_cast<void *>(pa[k].ptr);
        a.slots = pa[k].bytes / 8;
        st = p->arena.alloc_plain(&a.map, (size_t)a.slots * (u.wide ? 8 : 4));
        if (st == SPMV_SUCCESS) u.arrays.push_back(a);
    }
    auto drop = [&]() {
        (void)hipStreamSynchronize(p->stream);
        for (const UpdArray &a : u.arrays) p->arena.free(a.map);
    };
    // 3. fill and validate them on the plan's stream (the shadow's build has
    //    been synchronised by its builder)
    uint32_t *seen = nullptr;
    unsigned long long *cnt = nullptr;
    const size_t seen_bytes = 4 * (size_t)((p->nnz + 31) / 32);
    if (st == SPMV_SUCCESS) {
        DevScratch scratch(p->stream);
        st = scratch.alloc(&seen, seen_bytes / 4, "entry marks");
        if (st == SPMV_SUCCESS) st = scratch.alloc(&cnt, (size_t)kCntN, "counters");
        hipError_t e = hipSuccess;
        if (st == SPMV_SUCCESS) e = hipMemsetAsync(seen, 0, seen_bytes, p->stream);
        if (st == SPMV_SUCCESS && e == hipSuccess) e = hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * kCntN, p->stream);
        size_t vi = 0;
        for (size_t k = 0; k < pa.size() && st == SPMV_SUCCESS && e == hipSuccess; ++k) {
            if (!is_value_array(pa[k].name)) continue;
            const UpdArray &a = u.arrays[vi++];
            const unsigned grid = upd_grid((a.slots + 3) / 4);
            if (u.wide)
                hipLaunchKernelGGL(map_from_shadow_kernel<int64_t>, dim3(grid), dim3(256), 0, p->stream,
                                   (const double *)sa[k].ptr, (const double *)a.dst, a.slots, p->nnz,
                                   (int64_t *)a.map, seen, cnt);
            else
                hipLaunchKernelGGL(map_from_shadow_kernel<int32_t>, dim3(grid), dim3(256), 0, p->stream,
                                   (const double *)sa[k].ptr, (const double *)a.dst, a.slots, p->nnz,
                                   (int32_t *)a.map, seen, cnt);
            e = hipGetLastError();
        }
        unsigned long long h[kCntN] = {};
        if (st == SPMV_SUCCESS && e == hipSuccess)
            e = hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, p->stream);
        if (st == SPMV_SUCCESS && e == hipSuccess) e = hipStreamSynchronize(p->stream);
        if (st == SPMV_SUCCESS && e != hipSuccess) {
            set_error(std::string("spmv_plan_update_prepare: ") + hipGetErrorString(e));
            (void)hipGetLastError();
            st = SPMV_ERROR_HIP;
        }
        if (st == SPMV_SUCCESS && h[kCntStray] != 0) {
            set_error(kWrongPattern);
            st = SPMV_ERROR_INVALID_VALUE;
        } else if (st == SPMV_SUCCESS && (h[kCntBad] != 0 || h[kCntFilled] != (unsigned long long)p->nnz)) {
            set_error("spmv_plan_update_prepare: the layout adds several entries into one value slot (duplicate "
                      "(row, col) entries of a DIA plan): no entry-to-slot map exists");
            st = SPMV_ERROR_NOT_SUPPORTED;
        }
    }
    if (st != SPMV_SUCCESS) {
        const std::string msg = last_error();  // arena.free does not set one, but keep it whatever happens
        drop();
        set_error(msg);
        return st;
    }
    u.prepared = true;
    p->upd = u;
    return SPMV_SUCCESS;
}

}  // namespace spmv
