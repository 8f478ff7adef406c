// build_util.hpp -- plumbing shared by the plan builders (formats.cpp,
// build_bin.cpp, k_convert.hip, k_devbuild.hip, k_css_build.hip,
// k_bin_build.hip, k_transpose.hip): transient device scratch, plan allocations and uploads,
// launch grids and the end-of-phase check.  Host code only.
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include "internal.hpp"

namespace spmv {

// Transient device scratch of a builder, freed on every exit path once the
// stream its kernels run on has drained.  Allocations go through
// scratch_malloc (internal.hpp): OUT_OF_MEMORY only for hipErrorOutOfMemory
// (the host-CSR routing of capi_create.cpp then takes the host builders), HIP's
// sticky error cleared.
struct DevScratch {
    hipStream_t st;
    std::vector<void *> owned;
    explicit DevScratch(hipStream_t s) : st(s) {}
    DevScratch(const DevScratch &) = delete;
    DevScratch &operator=(const DevScratch &) = delete;
    ~DevScratch() {
        (void)hipStreamSynchronize(st);
        for (void *t : owned) (void)hipFree(t);
    }
    template <typename T>
    int alloc(T **q, size_t count, const char *what) {
        SPMV_RETURN_IF(scratch_malloc(q, sizeof(T) * count, what));
        owned.push_back(*q);
        return SPMV_SUCCESS;
    }
    // host table -> scratch, copied on the stream
    template <typename T>
    int upload(T **q, const std::vector<T> &h, const char *what = "table") {
        SPMV_RETURN_IF(alloc(q, h.size(), what));
        if (!h.empty()) SPMV_HIP_TRY(hipMemcpyAsync(*q, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, st));
        return SPMV_SUCCESS;
    }
};

// k_bin_build.hip: stable radix sort of (key, value) pairs by the keys' low
// `bits` bits on sc.st, double-buffered: keys[0] / vals[0] hold the input,
// keys[*current] / vals[*current] the result (bits = 0: the input itself), the
// other pair is clobbered.  The workspace lives in sc.
int sort_pairs_u32(DevScratch &sc, uint32_t *const keys[2], uint32_t *const vals[2], int64_t count, int bits,
                   int *current);

// count elements owned by the plan (zero-count safe)
template <typename T>
int plan_alloc(spmv_plan_s *p, T **dst, int64_t count) {
    void *q = nullptr;
    SPMV_RETURN_IF(p->arena.alloc(&q, sizeof(T) * (size_t)std::max<int64_t>(count, 1)));
    *dst = static_cast<T *>(q);
    return SPMV_SUCCESS;
}

// host array -> a new plan allocation (count elements; pad zeroed elements after)
template <typename T>
int plan_upload(spmv_plan_s *p, T **dst, const T *src, int64_t count, int64_t pad = 0) {
    SPMV_RETURN_IF(plan_alloc(p, dst, count + pad));
    if (count > 0) SPMV_HIP_TRY(hipMemcpy(*dst, src, sizeof(T) * (size_t)count, hipMemcpyHostToDevice));
    if (pad > 0) SPMV_HIP_TRY(hipMemset(*dst + count, 0, sizeof(T) * (size_t)pad));
    return SPMV_SUCCESS;
}
template <typename T>
int plan_upload(spmv_plan_s *p, T **dst, const std::vector<T> &src) {
    return plan_upload(p, dst, src.data(), (int64_t)src.size());
}

// grid of 256-thread workgroups for a grid-stride loop over n items, `per` items each
inline unsigned grid_for(int64_t n, int per = 256) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, 65536));
}
// one wave per item, 4 waves per 256-thread workgroup
inline unsigned waves_grid(int64_t waves) { return (unsigned)std::max<int64_t>(1, (waves + 3) / 4); }

// end of a builder phase: launch errors, then the stream drained
inline int build_sync(hipStream_t st, const char *what) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) return SPMV_SUCCESS;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    (void)hipGetLastError();
    return SPMV_ERROR_HIP;
}

}  // namespace spmv
