// capi_create.cpp -- the plan life cycle of include/spmv_hip.h: argument and
// CSR checks, the routing between the host and the device builders, the
// transpose, destroy.  Every entry point returns an int status.
#include <omp.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "build_util.hpp"

namespace spmv {

spmv_options_t resolve_options(const spmv_options_t *opt) {
    spmv_options_t o;
    if (opt) o = *opt;
    else spmv_options_default(&o);
    return o;
}

// Placement of the streamed arrays of the row-parallel formats (CSR, ELL,
// HYB, JDS, SS, COO, CSS; BIN and DIA place their large buffer themselves):
// AUTO maps every array of >= kStreamVmmMinBytes into 2-MB VMM handles
// (config 4, same launches on both placements, interleaved in one process:
// CSR 2.95 -> 2.81 ms, ELL 2.57 -> 2.40; profiles/round4/probe/
// c4_csr_vec4_slab_caps_vmm_plain.jsonl, c4_ell_caps_unroll_vmm_plain.jsonl), VMM does so from 32 MB, PLAIN never.
static void stream_placement(spmv_plan_s *p, int fmt, const spmv_options_t &o) {
    if (fmt == SPMV_FORMAT_BIN || fmt == SPMV_FORMAT_DIA) return;
    if (o.placement == SPMV_PLACEMENT_AUTO) p->arena.vmm_min = kStreamVmmMinBytes;
    else if (o.placement == SPMV_PLACEMENT_VMM) p->arena.vmm_min = kBinVmmMinBytes;
}

// The prologue of every create path: resolve the plan's device (requested <
// 0: the current one), check that it is a gfx950 and bind it.
static int open_device(int requested, int *dev) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
        (void)hipGetLastError();
        set_error("no HIP device visible (libspmv_hip needs an MI355X / gfx950)");
        return SPMV_ERROR_NO_DEVICE;
    }
    *dev = requested;
    if (*dev < 0) SPMV_HIP_TRY(hipGetDevice(dev));
    if (*dev >= count) {
        set_error("device ordinal out of range");
        return SPMV_ERROR_INVALID_VALUE;
    }
    hipDeviceProp_t prop;
    SPMV_HIP_TRY(hipGetDeviceProperties(&prop, *dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(std::string("device is ") + prop.gcnArchName + "; kernels are built for gfx950 only");
        return SPMV_ERROR_NO_DEVICE;
    }
    SPMV_HIP_TRY(hipSetDevice(*dev));
    return SPMV_SUCCESS;
}

// A fresh plan bound to `dev`; nullptr (error set) when the host is out of memory.
static spmv_plan_s *new_plan(int dev, int64_t m, int64_t n, int64_t nnz) {
    spmv_plan_s *p = new (std::nothrow) spmv_plan_s;
    if (!p) {
        set_error("host allocation of the plan failed");
        return nullptr;
    }
    p->device = dev;
    p->arena.device = dev;
    p->m = m;
    p->n = n;
    p->nnz = nnz;
    return p;
}

// The builders of every format, indexed by SPMV_FORMAT_* (AUTO is resolved
// before the table is read).
struct FormatBuilders {
    int (*host)(spmv_plan_s *, const HostCsr &, const spmv_options_t &);
    int (*device)(spmv_plan_s *, const DevCsr &, const spmv_options_t &);
};
static int build_ell_host(spmv_plan_s *p, const HostCsr &A, const spmv_options_t &o) {
    return build_ell(p, A, o, INT32_MAX);
}
static const FormatBuilders kBuilders[SPMV_FORMAT_BIN + 1] = {
    {nullptr, nullptr},                  // AUTO
    {build_csr, build_csr_device},       // CSR
    {build_ell_host, build_ell_device},  // ELL
    {build_ss, build_ss_device},         // SS
    {build_dia, build_dia_device},       // DIA
    {build_hyb, build_hyb_device},       // HYB
    {build_css, build_css_device},       // CSS
    {build_coo, build_coo_device},       // COO
    {build_jds, build_jds_device},       // JDS
    {build_bin, build_bin_device},       // BIN
};
static const FormatBuilders *builders_for(int fmt) {
    if (fmt > SPMV_FORMAT_AUTO && fmt <= SPMV_FORMAT_BIN) return &kBuilders[fmt];
    set_error("unknown format");
    return nullptr;
}

// The options a finished plan keeps (spmv_plan_s::opts): `o` as the create
// path ended with it (choose_crs_exact's rewrites applied), the format built,
// the plan's device; crs_exact itself is resolved, so it is cleared.
static void keep_options(spmv_plan_s *p, const spmv_options_t &o, int fmt, int dev) {
    p->opts = o;
    p->opts.format = fmt;
    p->opts.device = dev;
    p->opts.crs_exact = 0;
}

// Validate a host CSR before anything touches the GPU: an out-of-range
// column would become an out-of-bounds gather on the device.
// (need_val = false: a pattern, spmv_csr_transpose without values)
static int validate_csr(const HostCsr &A, bool need_val = true) {
    SPMV_CHECK_ARG(A.m >= 0 && A.n >= 0 && A.nnz >= 0, "negative dimension");
    SPMV_CHECK_ARG(A.m < (int64_t)INT32_MAX && A.n < (int64_t)INT32_MAX,
                   "m and n must be < 2^31 (int32 column indices)");
    SPMV_CHECK_ARG(A.row_ptr != nullptr, "row_ptr is NULL");
    SPMV_CHECK_ARG(A.nnz == 0 || (A.col != nullptr && (A.val != nullptr || !need_val)), "col/val is NULL");
    SPMV_CHECK_ARG(A.row_ptr[0] == 0, "row_ptr[0] != 0");
    SPMV_CHECK_ARG(A.row_ptr[A.m] == A.nnz, "row_ptr[m] != nnz");
    int64_t bad_rp = 0, bad_col = 0;
#pragma omp parallel for schedule(static) reduction(+ : bad_rp)
    for (int64_t r = 0; r < A.m; ++r) bad_rp += A.row_ptr[r + 1] < A.row_ptr[r];
    SPMV_CHECK_ARG(bad_rp == 0, "row_ptr is not non-decreasing");
    const int64_t n = A.n;
#pragma omp parallel for schedule(static) reduction(+ : bad_col)
    for (int64_t j = 0; j < A.nnz; ++j) bad_col += (A.col[j] < 0) | (A.col[j] >= n);
    SPMV_CHECK_ARG(bad_col == 0, "column index outside [0, n)");
    return SPMV_SUCCESS;
}

// The CSR of A^T from a validated host CSR of A: a stable counting sort of
// the entries by column (output row c = A's entries of column c in ascending
// entry index), t_col = the source rows.  The reference of
// transpose_csr_device (k_transpose.hip), byte for byte.  t_val and perm are
// optional; values move as 64-bit words.
static void transpose_csr_host(const HostCsr &A, int64_t *t_rp, int32_t *t_col, double *t_val, int64_t *perm) {
    std::fill(t_rp, t_rp + A.n + 1, (int64_t)0);
    for (int64_t j = 0; j < A.nnz; ++j) ++t_rp[A.col[j] + 1];
    for (int64_t c = 0; c < A.n; ++c) t_rp[c + 1] += t_rp[c];
    // t_rp[c] is column c's cursor while the entries are placed, then shifted back
    for (int64_t r = 0; r < A.m; ++r)
        for (int64_t j = A.row_ptr[r]; j < A.row_ptr[r + 1]; ++j) {
            const int64_t d = t_rp[A.col[j]]++;
            t_col[d] = (int32_t)r;
            if (t_val) std::memcpy(&t_val[d], &A.val[j], sizeof(double));
            if (perm) perm[d] = j;
        }
    for (int64_t c = A.n; c > 0; --c) t_rp[c] = t_rp[c - 1];
    t_rp[0] = 0;
}

int check_device_arrays(const void *const *ptrs, int count, int dev, const char *who, const char *what) {
    for (int k = 0; k < count; ++k) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, ptrs[k]) != hipSuccess || a.type != hipMemoryTypeDevice || a.device != dev) {
            (void)hipGetLastError();
            set_error(std::string(who) + what);
            return SPMV_ERROR_INVALID_VALUE;
        }
    }
    return SPMV_SUCCESS;
}

// Every check of a CSR the caller says lives in HBM, in the order of the
// host routes: the arguments, then the device (`requested` as open_device
// takes it, *dev = the one bound), then that the arrays -- and `also`, the
// caller's further device arrays, null ones skipped -- are memory of that
// device, then the CSR itself (k_convert.hip).  need_val = false: a pattern.
static int check_device_csr(const char *who, int requested, int *dev, const DevCsr &A, bool need_val,
                            std::initializer_list<const void *> also = {}) {
    SPMV_CHECK_ARG(A.m >= 0 && A.n >= 0 && A.nnz >= 0, "negative dimension");
    SPMV_CHECK_ARG(A.m < (int64_t)INT32_MAX && A.n < (int64_t)INT32_MAX,
                   "m and n must be < 2^31 (int32 column indices)");
    SPMV_CHECK_ARG(A.d_rp != nullptr, "row_ptr is NULL");
    SPMV_CHECK_ARG(A.nnz == 0 || (A.d_col != nullptr && (A.d_val != nullptr || !need_val)),
                   need_val ? "col/val is NULL" : "col_idx is NULL");
    SPMV_RETURN_IF(open_device(requested, dev));
    const void *ptrs[8] = {A.d_rp};
    int count = 1;
    if (A.nnz) ptrs[count++] = A.d_col;
    if (A.nnz && A.d_val) ptrs[count++] = A.d_val;
    for (const void *q : also)
        if (q && count < 8) ptrs[count++] = q;
    SPMV_RETURN_IF(check_device_arrays(ptrs, count, *dev, who));
    return validate_csr_device(A.d_rp, A.m, A.d_col, A.nnz, A.n);
}

int create_on_device(const DevCsr &D, spmv_options_t *opts, spmv_plan_t *out) {
    SPMV_CHECK_ARG(out != nullptr, "plan out-pointer is NULL");
    *out = nullptr;
    spmv_options_t o = *opts;
    int dev = -1;
    SPMV_RETURN_IF(check_device_csr("spmv_plan_create_csr_device", o.device, &dev, D, true));
    const int64_t m = D.m, n = D.n, nnz = D.nnz;
    spmv_plan_s *p = new_plan(dev, m, n, nnz);
    if (!p) return SPMV_ERROR_OUT_OF_MEMORY;
    // the row pointers are the only part of the matrix the host sees: row
    // lengths drive AUTO and every slice / bin / overflow decision (an explicit
    // SS, DIA or COO request never reads them on the host and does not pay for
    // the copy)
    std::vector<int64_t> hrp;
    if (o.format != SPMV_FORMAT_SS && o.format != SPMV_FORMAT_DIA && o.format != SPMV_FORMAT_COO) {
        hrp.resize((size_t)m + 1);
        const hipError_t e = hipMemcpy(hrp.data(), D.d_rp, 8 * (size_t)(m + 1), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            delete p;
            set_error(std::string("row_ptr to host: ") + hipGetErrorString(e));
            (void)hipGetLastError();
            return SPMV_ERROR_HIP;
        }
    }
    const DevCsr A{m, n, nnz, hrp.data(), D.d_rp, D.d_col, D.d_val};
    int fmt = o.format, st = SPMV_SUCCESS;
    if (fmt == SPMV_FORMAT_AUTO) {
        int census = SPMV_SUCCESS;
        fmt = choose_format_rp(m, n, nnz, hrp.data(), o, [&]() {
            std::vector<int32_t> offs;
            census = dia_offsets_device(p, A, 256, 1.25, offs);
            return census == SPMV_SUCCESS;
        });
        if (census != SPMV_SUCCESS && census != kDiaRefused) st = census;
    }
    if (st == SPMV_SUCCESS && fmt == SPMV_FORMAT_CSR && o.crs_exact) {
        int census = SPMV_SUCCESS;
        fmt = choose_crs_exact(
            m, n, nnz, hrp.data(), o,
            [&]() {
                std::vector<int32_t> offs;
                census = dia_offsets_device(p, A, 256, 1.25, offs);
                return census == SPMV_SUCCESS;
            },
            [&]() {
                int order = kRowsUnsorted;
                const int s2 = rows_order_device(p, A, &order);
                if (s2 != SPMV_SUCCESS) census = s2;
                return order;
            });
        if (census != SPMV_SUCCESS && census != kDiaRefused) st = census;
    }
    bool host_build = false;
    if (st == SPMV_SUCCESS) {
        stream_placement(p, fmt, o);
        const FormatBuilders *b = builders_for(fmt);
        if (!b) st = SPMV_ERROR_INVALID_VALUE;
        else if (fmt == SPMV_FORMAT_BIN && probe_env("SPMV_BIN_HOST_BUILD")) host_build = true;
        else st = b->device(p, A, o);
        // (BIN: rows out of strip order and no room for their sorted copy --
        // the host builders)
        if (st == kBinNeedHostBuild) host_build = true;
    }
    if (st == SPMV_SUCCESS && !host_build) {
        p->format = fmt;
        p->built_on_device = 1;
        keep_options(p, o, fmt, dev);
        *out = p;
        return SPMV_SUCCESS;
    }
    p->arena.release();
    delete p;
    if (!host_build) return st;
    *opts = o;
    opts->device = dev;
    opts->format = fmt;  // AUTO resolved above
    opts->build = SPMV_BUILD_HOST;
    return kNeedHostBuild;
}

// The host builders on a checked host CSR, on the bound device `dev`.
static int create_on_host(const HostCsr &A, spmv_options_t o, int dev, spmv_plan_t *out) {
    spmv_plan_s *p = new_plan(dev, A.m, A.n, A.nnz);
    if (!p) return SPMV_ERROR_OUT_OF_MEMORY;
    int fmt = o.format == SPMV_FORMAT_AUTO ? choose_format(A, o) : o.format;
    if (fmt == SPMV_FORMAT_CSR && o.crs_exact) fmt = choose_crs_exact(A, o);
    stream_placement(p, fmt, o);
    const FormatBuilders *b = builders_for(fmt);
    const int st = b ? b->host(p, A, o) : SPMV_ERROR_INVALID_VALUE;
    if (st != SPMV_SUCCESS) {
        p->arena.release();
        delete p;
        return st;
    }
    p->format = fmt;
    keep_options(p, o, fmt, dev);
    *out = p;
    return SPMV_SUCCESS;
}

int create_staged_on_host(const DevCsr &D, const spmv_options_t &o, spmv_plan_t *out) {
    SPMV_HIP_TRY(hipSetDevice(o.device));
    std::vector<int64_t> rp((size_t)D.m + 1);
    std::vector<int32_t> col((size_t)D.nnz);
    std::vector<double> val((size_t)D.nnz);
    SPMV_HIP_TRY(hipMemcpy(rp.data(), D.d_rp, 8 * (size_t)(D.m + 1), hipMemcpyDeviceToHost));
    if (D.nnz) {
        SPMV_HIP_TRY(hipMemcpy(col.data(), D.d_col, 4 * (size_t)D.nnz, hipMemcpyDeviceToHost));
        SPMV_HIP_TRY(hipMemcpy(val.data(), D.d_val, 8 * (size_t)D.nnz, hipMemcpyDeviceToHost));
    }
    const HostCsr H{D.m, D.n, D.nnz, rp.data(), col.data(), val.data()};
    return create_on_host(H, o, o.device, out);
}

// The CSR of A^T (T: n rows) in `sc`, from a validated CSR of A in HBM on the
// bound device (k_transpose.hip, its sort buffers freed before it returns).
static int transpose_in_scratch(DevScratch &sc, const DevCsr &A, DevCsr *T) {
    int64_t *t_rp = nullptr;
    int32_t *t_col = nullptr;
    double *t_val = nullptr;
    SPMV_RETURN_IF(sc.alloc(&t_rp, (size_t)A.n + 1, "transposed row_ptr"));
    SPMV_RETURN_IF(sc.alloc(&t_col, (size_t)A.nnz, "transposed col_idx"));
    SPMV_RETURN_IF(sc.alloc(&t_val, (size_t)A.nnz, "transposed val"));
    SPMV_RETURN_IF(transpose_csr_device(A.m, A.n, A.nnz, A.d_rp, A.d_col, A.d_val, t_rp, t_col, t_val, nullptr));
    *T = DevCsr{A.n, A.m, A.nnz, nullptr, t_rp, t_col, t_val};
    return SPMV_SUCCESS;
}

// Stage a (validated) host CSR into HBM and build the plan there
// (create_on_device: the same layouts byte for byte, AUTO resolved by the
// same chooser; transpose: the plan of A^T, from its CSR in scratch).
// A format the device builders do not make comes back as kNeedHostBuild with
// the resolved options in *o; SPMV_ERROR_OUT_OF_MEMORY when the staging copy
// (or the transposition's scratch) does not fit.  Either way the caller then
// takes the host builders.
static int create_via_device(const HostCsr &A, bool transpose, spmv_options_t *o, spmv_plan_t *out) {
    void *d[3] = {nullptr, nullptr, nullptr};
    const size_t bytes[3] = {8 * (size_t)(A.m + 1), 4 * (size_t)std::max<int64_t>(A.nnz, 1),
                             8 * (size_t)std::max<int64_t>(A.nnz, 1)};
    auto release = [&]() {
        (void)hipDeviceSynchronize();  // the builders' kernels have read the staging copy
        for (void *q : d)
            if (q) (void)hipFree(q);
    };
    for (int k = 0; k < 3; ++k)
        if (hipMalloc(&d[k], bytes[k]) != hipSuccess) {
            (void)hipGetLastError();
            release();
            set_error("device staging of the CSR: out of device memory");
            return SPMV_ERROR_OUT_OF_MEMORY;
        }
    hipError_t e = hipMemcpy(d[0], A.row_ptr, bytes[0], hipMemcpyHostToDevice);
    if (e == hipSuccess && A.nnz) e = hipMemcpy(d[1], A.col, 4 * (size_t)A.nnz, hipMemcpyHostToDevice);
    if (e == hipSuccess && A.nnz) e = hipMemcpy(d[2], A.val, 8 * (size_t)A.nnz, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        release();
        set_error(std::string("device staging of the CSR: ") + hipGetErrorString(e));
        return SPMV_ERROR_HIP;
    }
    const DevCsr D{A.m, A.n, A.nnz, nullptr, (const int64_t *)d[0], (const int32_t *)d[1], (const double *)d[2]};
    int st;
    if (transpose) {
        DevScratch scratch(nullptr);
        DevCsr T;
        st = transpose_in_scratch(scratch, D, &T);
        if (st == SPMV_SUCCESS) st = create_on_device(T, o, out);
    } else {
        st = create_on_device(D, o, out);
    }
    release();
    return st;
}

// spmv_options_t::build AUTO: host CSRs from this many entries up are built
// by the device builders (config 4's DIA plan: 10.3 s through the host
// builders; below this size a host build takes well under a second)
constexpr int64_t kDeviceBuildMinNnz = (int64_t)1 << 24;

// The body of every create from a host CSR (transpose: the plan of A^T).
// Every check of the arguments and of the CSR comes before the device is
// opened.  The device builders make every format; what they cannot (BIN rows
// out of strip order without room for their sorted copy) and a staging copy
// that does not fit take the host builders -- with the format AUTO resolved
// on the device.
static int create_from_csr(const HostCsr &A, const spmv_options_t *opt_in, spmv_plan_t *out, bool transpose = false) {
    SPMV_CHECK_ARG(out != nullptr, "plan out-pointer is NULL");
    *out = nullptr;
    spmv_options_t o = resolve_options(opt_in);
    SPMV_CHECK_ARG(o.build >= SPMV_BUILD_AUTO && o.build <= SPMV_BUILD_DEVICE, "build must be SPMV_BUILD_*");
    SPMV_RETURN_IF(validate_csr(A));
    int dev = -1;
    SPMV_RETURN_IF(open_device(o.device, &dev));
    o.device = dev;
    int st = kNeedHostBuild;
    // (the device transposition's 32-bit entry ids: larger matrices take the host route)
    if ((o.build == SPMV_BUILD_DEVICE || (o.build == SPMV_BUILD_AUTO && A.nnz >= kDeviceBuildMinNnz)) &&
        (!transpose || A.nnz < (int64_t)INT32_MAX)) {
        st = create_via_device(A, transpose, &o, out);
        if (st == SPMV_ERROR_OUT_OF_MEMORY) st = kNeedHostBuild;
        if (st == kNeedHostBuild) SPMV_HIP_TRY(hipSetDevice(dev));
    }
    if (st == kNeedHostBuild && !transpose) st = create_on_host(A, o, dev, out);
    else if (st == kNeedHostBuild) {
        std::vector<int64_t> t_rp;
        std::vector<int32_t> t_col;
        std::vector<double> t_val;
        try {
            t_rp.resize((size_t)A.n + 1);
            t_col.resize((size_t)A.nnz);
            t_val.resize((size_t)A.nnz);
        } catch (const std::bad_alloc &) {
            set_error("host allocation of the transposed CSR failed");
            return SPMV_ERROR_OUT_OF_MEMORY;
        }
        transpose_csr_host(A, t_rp.data(), t_col.data(), t_val.data(), nullptr);
        const HostCsr T{A.n, A.m, A.nnz, t_rp.data(), t_col.data(), t_val.data()};
        st = create_on_host(T, o, dev, out);
    }
    if (st == SPMV_SUCCESS && transpose) (*out)->transposed = 1;
    return st;
}

}  // namespace spmv

using namespace spmv;

extern "C" {

void spmv_options_default(spmv_options_t *o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->format = SPMV_FORMAT_AUTO;
    o->device = -1;
}

int spmv_plan_create_csr(int64_t m, int64_t n, int64_t nnz, const int64_t *row_ptr,
                         const int32_t *col_idx, const double *val, const spmv_options_t *opt,
                         spmv_plan_t *plan) {
    HostCsr A{m, n, nnz, row_ptr, col_idx, val};
    return create_from_csr(A, opt, plan);
}

int spmv_plan_create_csr32(int32_t m, int32_t n, int32_t nnz, const int32_t *row_ptr,
                           const int32_t *col_idx, const double *val, const spmv_options_t *opt,
                           spmv_plan_t *plan) {
    SPMV_CHECK_ARG(m >= 0 && row_ptr != nullptr, "bad m or NULL row_ptr");
    std::vector<int64_t> rp((size_t)m + 1);
    for (int32_t i = 0; i <= m; ++i) rp[i] = row_ptr[i];
    HostCsr A{m, n, nnz, rp.data(), col_idx, val};
    return create_from_csr(A, opt, plan);
}

int spmv_plan_create_csr_device(int64_t m, int64_t n, int64_t nnz, const int64_t *d_row_ptr,
                                const int32_t *d_col_idx, const double *d_val, const spmv_options_t *opt,
                                spmv_plan_t *out) {
    const DevCsr A{m, n, nnz, nullptr, d_row_ptr, d_col_idx, d_val};
    spmv_options_t o = resolve_options(opt);
    const int st = create_on_device(A, &o, out);
    return st == kNeedHostBuild ? create_staged_on_host(A, o, out) : st;
}

int spmv_plan_create_csr32_device(int32_t m, int32_t n, int32_t nnz, const int32_t *d_row_ptr,
                                  const int32_t *d_col_idx, const double *d_val, const spmv_options_t *opt,
                                  spmv_plan_t *out) {
    SPMV_CHECK_ARG(out != nullptr, "plan out-pointer is NULL");
    *out = nullptr;
    SPMV_CHECK_ARG(m >= 0 && n >= 0 && nnz >= 0 && d_row_ptr != nullptr, "bad dimensions or NULL row_ptr");
    int dev = -1;
    SPMV_RETURN_IF(open_device(opt ? opt->device : -1, &dev));
    const void *rp32 = d_row_ptr;
    SPMV_RETURN_IF(check_device_arrays(&rp32, 1, dev, "spmv_plan_create_csr32_device"));
    int64_t *rp64 = nullptr;
    SPMV_RETURN_IF(widen_row_ptr_device(d_row_ptr, m, &rp64));
    const int st = spmv_plan_create_csr_device(m, n, nnz, rp64, d_col_idx, d_val, opt, out);
    (void)hipFree(rp64);
    return st;
}

int spmv_csr_transpose(int64_t m, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col_idx,
                       const double *val, int64_t *t_row_ptr, int32_t *t_col_idx, double *t_val, int64_t *perm) {
    SPMV_CHECK_ARG((val == nullptr) == (t_val == nullptr) || nnz <= 0, "val and t_val: both or neither");
    SPMV_CHECK_ARG(t_row_ptr != nullptr && (nnz <= 0 || t_col_idx != nullptr), "t_row_ptr / t_col_idx is NULL");
    const HostCsr A{m, n, nnz, row_ptr, col_idx, val};
    SPMV_RETURN_IF(validate_csr(A, false));
    transpose_csr_host(A, t_row_ptr, t_col_idx, t_val, perm);
    return SPMV_SUCCESS;
}

int spmv_csr_transpose_device(int32_t device, int64_t m, int64_t n, int64_t nnz, const int64_t *d_row_ptr,
                              const int32_t *d_col_idx, const double *d_val, int64_t *d_t_row_ptr,
                              int32_t *d_t_col_idx, double *d_t_val, int64_t *d_perm) {
    SPMV_CHECK_ARG((d_val == nullptr) == (d_t_val == nullptr) || nnz <= 0, "val and t_val: both or neither");
    SPMV_CHECK_ARG(d_t_row_ptr != nullptr && (nnz <= 0 || d_t_col_idx != nullptr), "t_row_ptr / t_col_idx is NULL");
    const DevCsr A{m, n, nnz, nullptr, d_row_ptr, d_col_idx, d_val};
    int dev = -1;
    // (nnz = 0: the entry arrays are not read, whatever the caller passed)
    SPMV_RETURN_IF(check_device_csr("spmv_csr_transpose_device", device, &dev, A, false,
                                    {d_t_row_ptr, nnz ? d_t_col_idx : nullptr, nnz && d_val ? d_t_val : nullptr,
                                     nnz ? d_perm : nullptr}));
    return transpose_csr_device(m, n, nnz, d_row_ptr, d_col_idx, d_val, d_t_row_ptr, d_t_col_idx, d_t_val, d_perm);
}

int spmv_plan_create_csr_transposed(int64_t m, int64_t n, int64_t nnz, const int64_t *row_ptr,
                                    const int32_t *col_idx, const double *val, const spmv_options_t *opt,
                                    spmv_plan_t *plan) {
    const HostCsr A{m, n, nnz, row_ptr, col_idx, val};
    return create_from_csr(A, opt, plan, true);
}

// The plan of A^T from a CSR of A in HBM: the CSR of A^T in scratch, the
// device builders on it (they check it as they check any caller's), the
// scratch freed.  The plan keeps neither A nor the permutation.
int spmv_plan_create_csr_device_transposed(int64_t m, int64_t n, int64_t nnz, const int64_t *d_row_ptr,
                                           const int32_t *d_col_idx, const double *d_val, const spmv_options_t *opt,
                                           spmv_plan_t *out) {
    SPMV_CHECK_ARG(out != nullptr, "plan out-pointer is NULL");
    *out = nullptr;
    const DevCsr A{m, n, nnz, nullptr, d_row_ptr, d_col_idx, d_val};
    spmv_options_t o = resolve_options(opt);
    SPMV_RETURN_IF(check_device_csr("spmv_plan_create_csr_device_transposed", o.device, &o.device, A, true));
    DevScratch scratch(nullptr);
    DevCsr T;
    SPMV_RETURN_IF(transpose_in_scratch(scratch, A, &T));
    int st = create_on_device(T, &o, out);
    if (st == kNeedHostBuild) st = create_staged_on_host(T, o, out);
    if (st == SPMV_SUCCESS) (*out)->transposed = 1;
    return st;
}

int spmv_coo_to_csr(int32_t m, int64_t nnz, const int32_t *row_idx, int64_t *row_ptr) {
    SPMV_CHECK_ARG(m >= 0 && nnz >= 0 && row_ptr != nullptr, "bad arguments");
    SPMV_CHECK_ARG(nnz == 0 || row_idx != nullptr, "row_idx is NULL");
    // the linear scan of src/opt_crs.cpp:26-33
    int64_t p = 0;
    for (int64_t i = 0; i < nnz; ++i) {
        const int32_t r = row_idx[i];
        SPMV_CHECK_ARG(r >= 0 && r < m, "row index outside [0, m)");
        SPMV_CHECK_ARG(r + 1 >= p, "COO rows are not sorted");
        while (p <= r) row_ptr[p++] = i;
    }
    while (p <= m) row_ptr[p++] = nnz;
    return SPMV_SUCCESS;
}

int spmv_plan_create_coo(int32_t m, int32_t n, int32_t nnz, const int32_t *row_idx,
                         const int32_t *col_idx, const double *val, const spmv_options_t *opt,
                         spmv_plan_t *plan) {
    SPMV_CHECK_ARG(m >= 0 && nnz >= 0, "negative dimension");
    std::vector<int64_t> rp((size_t)m + 1);
    SPMV_RETURN_IF(spmv_coo_to_csr(m, nnz, row_idx, rp.data()));
    HostCsr A{m, n, nnz, rp.data(), col_idx, val};
    return create_from_csr(A, opt, plan);
}

int spmv_plan_destroy(spmv_plan_t p) {
    if (!p) return SPMV_SUCCESS;
    (void)bind_device(p);
    cg_graph_release(p);
    p->arena.release();
    delete p;
    return SPMV_SUCCESS;
}

}  // extern "C"
