// capi.cpp -- the C-ABI of include/spmv_hip.h: plan life cycle, execute,
// timing, info.  Every entry point returns an int status; nothing exit()s.
#include <omp.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "build_util.hpp"

namespace spmv {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
const char *last_error() { return g_err.c_str(); }

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
    if (const char *e = probe_env("SPMV_ARENA_VMM_MB")) p->arena.vmm_min = (size_t)std::max(0, std::atoi(e)) << 20;
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
    if (const char *e = probe_env("SPMV_ARENA_VMM_MB")) p->arena.vmm_min = (size_t)std::max(0, std::atoi(e)) << 20;
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

// every pointer device memory on `dev`?
static int check_device_arrays(const void *const *ptrs, int count, int dev, const char *who) {
    for (int k = 0; k < count; ++k) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, ptrs[k]) != hipSuccess || a.type != hipMemoryTypeDevice || a.device != dev) {
            (void)hipGetLastError();
            set_error(std::string(who) + ": arrays must be device memory on the plan's device");
            return SPMV_ERROR_INVALID_VALUE;
        }
    }
    return SPMV_SUCCESS;
}

// spmv_options_t::build AUTO: host CSRs from this many entries up are built
// by the device builders (config 4's DIA plan: 10.3 s through the host
// builders; below this size a host build takes well under a second)
constexpr int64_t kDeviceBuildMinNnz = (int64_t)1 << 24;

static int create_from_csr(const HostCsr &A, const spmv_options_t *opt_in, spmv_plan_t *out);

// spmv_plan_create_csr_device's body.  A plan the device builders do not
// make (BIN rows out of strip order when the device has no room for their
// sorted copy) is built by the host builders: from a D2H copy of the CSR, or --
// when need_host_fmt is given (create_via_device, whose caller still holds the
// host CSR) -- by returning kNeedHostBuild with the resolved options there
// (format chosen, crs_exact's rewrites applied, build = HOST).
constexpr int kNeedHostBuild = -2000;
static int create_device_impl(int64_t m, int64_t n, int64_t nnz, const int64_t *d_row_ptr,
                              const int32_t *d_col_idx, const double *d_val, const spmv_options_t *opt_in,
                              spmv_plan_t *out, spmv_options_t *need_host) {
    SPMV_CHECK_ARG(out != nullptr, "plan out-pointer is NULL");
    *out = nullptr;
    spmv_options_t o;
    if (opt_in) o = *opt_in;
    else spmv_options_default(&o);
    SPMV_CHECK_ARG(m >= 0 && n >= 0 && nnz >= 0, "negative dimension");
    SPMV_CHECK_ARG(m < (int64_t)INT32_MAX && n < (int64_t)INT32_MAX, "m and n must be < 2^31 (int32 column indices)");
    SPMV_CHECK_ARG(d_row_ptr != nullptr, "row_ptr is NULL");
    SPMV_CHECK_ARG(nnz == 0 || (d_col_idx != nullptr && d_val != nullptr), "col/val is NULL");
    int dev = -1;
    SPMV_RETURN_IF(open_device(o.device, &dev));
    const void *ptrs[3] = {d_row_ptr, d_col_idx, d_val};
    SPMV_RETURN_IF(check_device_arrays(ptrs, nnz ? 3 : 1, dev, "spmv_plan_create_csr_device"));
    SPMV_RETURN_IF(validate_csr_device(d_row_ptr, m, d_col_idx, nnz, n));
    spmv_plan_s *p = new_plan(dev, m, n, nnz);
    if (!p) return SPMV_ERROR_OUT_OF_MEMORY;
    // the row pointers are the only part of the matrix the host sees: row
    // lengths drive AUTO and every slice / bin / overflow decision (an explicit
    // SS, DIA or COO request never reads them on the host and does not pay for
    // the copy)
    std::vector<int64_t> hrp;
    if (o.format != SPMV_FORMAT_SS && o.format != SPMV_FORMAT_DIA && o.format != SPMV_FORMAT_COO) {
        hrp.resize((size_t)m + 1);
        const hipError_t e = hipMemcpy(hrp.data(), d_row_ptr, 8 * (size_t)(m + 1), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            delete p;
            set_error(std::string("row_ptr to host: ") + hipGetErrorString(e));
            (void)hipGetLastError();
            return SPMV_ERROR_HIP;
        }
    }
    const DevCsr A{m, n, nnz, hrp.data(), d_row_ptr, d_col_idx, d_val};
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
        // the host builder below)
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
    if (need_host) {
        *need_host = o;
        need_host->device = dev;
        need_host->format = fmt;  // AUTO resolved above
        need_host->build = SPMV_BUILD_HOST;
        return kNeedHostBuild;
    }
    {
        // host builders: stage the CSR through host memory
        std::vector<int64_t> rp((size_t)m + 1);
        std::vector<int32_t> col((size_t)nnz);
        std::vector<double> val((size_t)nnz);
        SPMV_HIP_TRY(hipMemcpy(rp.data(), d_row_ptr, 8 * (size_t)(m + 1), hipMemcpyDeviceToHost));
        if (nnz) {
            SPMV_HIP_TRY(hipMemcpy(col.data(), d_col_idx, 4 * (size_t)nnz, hipMemcpyDeviceToHost));
            SPMV_HIP_TRY(hipMemcpy(val.data(), d_val, 8 * (size_t)nnz, hipMemcpyDeviceToHost));
        }
        o.device = dev;
        o.format = fmt;  // AUTO resolved above
        o.build = SPMV_BUILD_HOST;
        HostCsr H{m, n, nnz, rp.data(), col.data(), val.data()};
        return create_from_csr(H, &o, out);
    }
}

// The plan of A^T from a validated CSR of A in HBM on the bound device: the
// CSR of A^T in scratch (k_transpose.hip, its sort buffers freed before the
// builders run), create_device_impl on it, the scratch freed.  The plan keeps
// neither A nor the permutation.
static int create_device_transposed_impl(int64_t m, int64_t n, int64_t nnz, const int64_t *d_row_ptr,
                                         const int32_t *d_col_idx, const double *d_val, const spmv_options_t *opt,
                                         spmv_plan_t *out, spmv_options_t *need_host) {
    DevScratch scratch(nullptr);
    int64_t *t_rp = nullptr;
    int32_t *t_col = nullptr;
    double *t_val = nullptr;
    SPMV_RETURN_IF(scratch.alloc(&t_rp, (size_t)n + 1, "transposed row_ptr"));
    SPMV_RETURN_IF(scratch.alloc(&t_col, (size_t)nnz, "transposed col_idx"));
    SPMV_RETURN_IF(scratch.alloc(&t_val, (size_t)nnz, "transposed val"));
    SPMV_RETURN_IF(transpose_csr_device(m, n, nnz, d_row_ptr, d_col_idx, d_val, t_rp, t_col, t_val, nullptr));
    const int st = create_device_impl(n, m, nnz, t_rp, t_col, t_val, opt, out, need_host);
    if (st == SPMV_SUCCESS) (*out)->transposed = 1;
    return st;
}

// Stage a (validated) host CSR into HBM and build the plan there
// (create_device_impl: the same layouts byte for byte, AUTO resolved by the
// same chooser; transpose: the plan of A^T, create_device_transposed_impl).
// A format the device builders do not make comes back as
// kNeedHostBuild with the resolved options in *host_opts;
// SPMV_ERROR_OUT_OF_MEMORY when the staging copy (or the transposition's
// scratch) does not fit.  Either way the caller then takes the host builders.
static int create_via_device(const HostCsr &A, spmv_options_t o, int dev, spmv_plan_t *out,
                             spmv_options_t *host_opts, bool transpose = false) {
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
    o.device = dev;
    const int st = (transpose ? create_device_transposed_impl : create_device_impl)(
        A.m, A.n, A.nnz, (const int64_t *)d[0], (const int32_t *)d[1], (const double *)d[2], &o, out, host_opts);
    release();
    return st;
}

// spmv_plan_create_csr_transposed's body: create_from_csr's routing with the
// transposition in front of the builders of either route.
static int create_from_csr_transposed(const HostCsr &A, const spmv_options_t *opt_in, spmv_plan_t *out) {
    SPMV_CHECK_ARG(out != nullptr, "plan out-pointer is NULL");
    *out = nullptr;
    spmv_options_t o;
    if (opt_in) o = *opt_in;
    else spmv_options_default(&o);
    SPMV_CHECK_ARG(o.build >= SPMV_BUILD_AUTO && o.build <= SPMV_BUILD_DEVICE, "build must be SPMV_BUILD_*");
    SPMV_RETURN_IF(validate_csr(A));
    int dev = -1;
    SPMV_RETURN_IF(open_device(o.device, &dev));
    // (the device transposition's 32-bit entry ids: larger matrices take the host route)
    if ((o.build == SPMV_BUILD_DEVICE || (o.build == SPMV_BUILD_AUTO && A.nnz >= kDeviceBuildMinNnz)) &&
        A.nnz < (int64_t)INT32_MAX) {
        spmv_options_t ho = o;
        const int st = create_via_device(A, o, dev, out, &ho, true);
        if (st != SPMV_ERROR_OUT_OF_MEMORY && st != kNeedHostBuild) return st;
        if (st == kNeedHostBuild) o = ho;
        SPMV_HIP_TRY(hipSetDevice(dev));
    }
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
    o.device = dev;
    o.build = SPMV_BUILD_HOST;
    const HostCsr T{A.n, A.m, A.nnz, t_rp.data(), t_col.data(), t_val.data()};
    const int st = create_from_csr(T, &o, out);
    if (st == SPMV_SUCCESS) (*out)->transposed = 1;
    return st;
}

static int create_from_csr(const HostCsr &A, const spmv_options_t *opt_in, spmv_plan_t *out) {
    SPMV_CHECK_ARG(out != nullptr, "plan out-pointer is NULL");
    *out = nullptr;
    spmv_options_t o;
    if (opt_in) o = *opt_in;
    else spmv_options_default(&o);
    SPMV_CHECK_ARG(o.build >= SPMV_BUILD_AUTO && o.build <= SPMV_BUILD_DEVICE, "build must be SPMV_BUILD_*");
    SPMV_RETURN_IF(validate_csr(A));
    int dev = -1;
    SPMV_RETURN_IF(open_device(o.device, &dev));
    // the device builders make every format; what they cannot (BIN rows out
    // of strip order without room for their sorted copy) and a staging copy
    // that does not fit take the host builders below -- with the format AUTO
    // resolved on the device
    if (o.build == SPMV_BUILD_DEVICE || (o.build == SPMV_BUILD_AUTO && A.nnz >= kDeviceBuildMinNnz)) {
        spmv_options_t ho = o;
        const int st = create_via_device(A, o, dev, out, &ho);
        if (st != SPMV_ERROR_OUT_OF_MEMORY && st != kNeedHostBuild) return st;
        if (st == kNeedHostBuild) o = ho;
        SPMV_HIP_TRY(hipSetDevice(dev));
    }
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

static int dispatch(const spmv_plan_s *p, const double *x, double *y) {
    switch (p->format) {
        case SPMV_FORMAT_CSR: return launch_csr(p, x, y);
        case SPMV_FORMAT_ELL: return launch_ell(p, x, y);
        case SPMV_FORMAT_HYB:
        case SPMV_FORMAT_JDS:
            SPMV_RETURN_IF(launch_ell(p, x, y));
            phase_mark(p);  // ell | overflow
            return launch_hyb_overflow(p, x, y);
        case SPMV_FORMAT_SS: return launch_ss(p, x, y);
        case SPMV_FORMAT_DIA: return launch_dia(p, x, y);
        case SPMV_FORMAT_CSS: return launch_css(p, x, y);
        case SPMV_FORMAT_COO: return launch_coo(p, x, y);
        case SPMV_FORMAT_BIN: return launch_bin(p, x, y);
    }
    set_error("plan has an unknown format");
    return SPMV_ERROR_INVALID_VALUE;
}

static int bind_device(const spmv_plan_s *p) {
    int cur = -1;
    SPMV_HIP_TRY(hipGetDevice(&cur));
    if (cur != p->device) SPMV_HIP_TRY(hipSetDevice(p->device));
    return SPMV_SUCCESS;
}

// Times `iters` repetitions of `run` (a status; the first failure ends the
// loop) between two events on `s`.  Both events are destroyed on every path.
template <class Run>
static int time_on_stream(hipStream_t s, int32_t iters, double *ms, Run run) {
    hipEvent_t a = nullptr, b = nullptr;
    hipError_t e = hipEventCreate(&a);
    if (e == hipSuccess) e = hipEventCreate(&b);
    if (e == hipSuccess) e = hipEventRecord(a, s);
    int st = SPMV_SUCCESS;
    for (int32_t i = 0; i < iters && st == SPMV_SUCCESS && e == hipSuccess; ++i) st = run();
    if (e == hipSuccess) e = hipEventRecord(b, s);
    if (e == hipSuccess) e = hipEventSynchronize(b);
    float f = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&f, a, b);
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    SPMV_HIP_TRY(e);
    *ms = f;
    return st;
}

}  // namespace spmv

using namespace spmv;

extern "C" {

int spmv_api_version(void) { return SPMV_HIP_API_VERSION; }

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
                                const int32_t *d_col_idx, const double *d_val, const spmv_options_t *opt_in,
                                spmv_plan_t *out) {
    return create_device_impl(m, n, nnz, d_row_ptr, d_col_idx, d_val, opt_in, out, nullptr);
}

int spmv_plan_create_csr32_device(int32_t m, int32_t n, int32_t nnz, const int32_t *d_row_ptr,
                                  const int32_t *d_col_idx, const double *d_val, const spmv_options_t *opt,
                                  spmv_plan_t *out) {
    SPMV_CHECK_ARG(out != nullptr, "plan out-pointer is NULL");
    *out = nullptr;
    SPMV_CHECK_ARG(m >= 0 && n >= 0 && nnz >= 0 && d_row_ptr != nullptr, "bad dimensions or NULL row_ptr");
    int dev = -1;
    SPMV_RETURN_IF(open_device(opt ? opt->device : -1, &dev));
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, d_row_ptr) != hipSuccess || a.type != hipMemoryTypeDevice || a.device != dev) {
        (void)hipGetLastError();
        set_error("spmv_plan_create_csr32_device: arrays must be device memory on the plan's device");
        return SPMV_ERROR_INVALID_VALUE;
    }
    int64_t *rp64 = nullptr;
    SPMV_RETURN_IF(widen_row_ptr_device(d_row_ptr, m, &rp64));
    const int st = spmv_plan_create_csr_device(m, n, nnz, rp64, d_col_idx, d_val, opt, out);
    (void)hipFree(rp64);
    return st;
}

// ---- the transpose: the CSR of A^T, and plans built from it -----------------
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
    SPMV_CHECK_ARG(m >= 0 && n >= 0 && nnz >= 0, "negative dimension");
    SPMV_CHECK_ARG(m < (int64_t)INT32_MAX && n < (int64_t)INT32_MAX, "m and n must be < 2^31 (int32 column indices)");
    SPMV_CHECK_ARG(d_row_ptr != nullptr, "row_ptr is NULL");
    SPMV_CHECK_ARG(nnz == 0 || d_col_idx != nullptr, "col_idx is NULL");
    int dev = -1;
    SPMV_RETURN_IF(open_device(device, &dev));
    std::vector<const void *> ptrs = {d_row_ptr, d_t_row_ptr};
    if (nnz) {
        ptrs.insert(ptrs.end(), {d_col_idx, d_t_col_idx});
        if (d_val) ptrs.insert(ptrs.end(), {d_val, d_t_val});
        if (d_perm) ptrs.push_back(d_perm);
    }
    SPMV_RETURN_IF(check_device_arrays(ptrs.data(), (int)ptrs.size(), dev, "spmv_csr_transpose_device"));
    SPMV_RETURN_IF(validate_csr_device(d_row_ptr, m, d_col_idx, nnz, n));
    return transpose_csr_device(m, n, nnz, d_row_ptr, d_col_idx, d_val, d_t_row_ptr, d_t_col_idx, d_t_val, d_perm);
}

int spmv_plan_create_csr_transposed(int64_t m, int64_t n, int64_t nnz, const int64_t *row_ptr,
                                    const int32_t *col_idx, const double *val, const spmv_options_t *opt,
                                    spmv_plan_t *plan) {
    const HostCsr A{m, n, nnz, row_ptr, col_idx, val};
    return create_from_csr_transposed(A, opt, plan);
}

int spmv_plan_create_csr_device_transposed(int64_t m, int64_t n, int64_t nnz, const int64_t *d_row_ptr,
                                           const int32_t *d_col_idx, const double *d_val, const spmv_options_t *opt,
                                           spmv_plan_t *out) {
    SPMV_CHECK_ARG(out != nullptr, "plan out-pointer is NULL");
    *out = nullptr;
    SPMV_CHECK_ARG(m >= 0 && n >= 0 && nnz >= 0, "negative dimension");
    SPMV_CHECK_ARG(m < (int64_t)INT32_MAX && n < (int64_t)INT32_MAX, "m and n must be < 2^31 (int32 column indices)");
    SPMV_CHECK_ARG(d_row_ptr != nullptr, "row_ptr is NULL");
    SPMV_CHECK_ARG(nnz == 0 || (d_col_idx != nullptr && d_val != nullptr), "col/val is NULL");
    int dev = -1;
    SPMV_RETURN_IF(open_device(opt ? opt->device : -1, &dev));
    const void *ptrs[3] = {d_row_ptr, d_col_idx, d_val};
    SPMV_RETURN_IF(check_device_arrays(ptrs, nnz ? 3 : 1, dev, "spmv_plan_create_csr_device_transposed"));
    SPMV_RETURN_IF(validate_csr_device(d_row_ptr, m, d_col_idx, nnz, n));
    spmv_options_t o;
    if (opt) o = *opt;
    else spmv_options_default(&o);
    o.device = dev;
    return create_device_transposed_impl(m, n, nnz, d_row_ptr, d_col_idx, d_val, &o, out, nullptr);
}

int spmv_plan_is_transposed(spmv_plan_t p, int32_t *transposed) {
    SPMV_CHECK_ARG(p != nullptr && transposed != nullptr, "NULL plan or out-pointer");
    *transposed = p->transposed;
    return SPMV_SUCCESS;
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
    p->arena.release();
    delete p;
    return SPMV_SUCCESS;
}

int spmv_set_stream(spmv_plan_t p, void *stream) {
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    p->stream = (hipStream_t)stream;
    return SPMV_SUCCESS;
}

static int execute_impl(spmv_plan_t p, double alpha, const double *x, double *y, uint32_t flags);

int spmv_execute(spmv_plan_t p, const double *x, double *y, uint32_t flags) {
    return execute_impl(p, 1.0, x, y, flags);
}

int spmv_execute_alpha(spmv_plan_t p, double alpha, const double *x, double *y, uint32_t flags) {
    return execute_impl(p, alpha, x, y, flags);
}

static int execute_impl(spmv_plan_t p, double alpha, const double *x, double *y, uint32_t flags) {
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    const bool staged = (flags & SPMV_X_STAGED) != 0;
    const bool y_staged = (flags & SPMV_Y_STAGED) != 0;
    SPMV_CHECK_ARG((x != nullptr || p->n == 0 || staged) && (y != nullptr || p->m == 0 || y_staged),
                   "x or y is NULL");
    SPMV_CHECK_ARG(!(y_staged && (flags & SPMV_Y_DEVICE)), "SPMV_Y_STAGED with SPMV_Y_DEVICE");
    SPMV_CHECK_ARG(!staged || p->x_stage != nullptr, "SPMV_X_STAGED without a previously staged x");
    SPMV_RETURN_IF(bind_device(p));
    // spmv_fetch_y serves the y of the latest execute only when that execute
    // was SPMV_Y_STAGED: any other execute (device y, host y) clears the mark
    p->y_staged = false;
    const double *dx = x;
    double *dy = y;
    if (staged) {
        dx = p->x_stage;
        flags |= SPMV_X_DEVICE;
    } else if (!(flags & SPMV_X_DEVICE)) {
        // opt_cusparse.cpp:72 -- H2D copy of x on every call
        if (!p->x_stage) {
            void *q;
            SPMV_RETURN_IF(p->arena.alloc(&q, sizeof(double) * (size_t)std::max<int64_t>(p->n, 1)));
            p->x_stage = (double *)q;
        }
        if (p->n) SPMV_HIP_TRY(hipMemcpyAsync(p->x_stage, x, sizeof(double) * p->n, hipMemcpyHostToDevice, p->stream));
        dx = p->x_stage;
    }
    if (!(flags & SPMV_Y_DEVICE)) {
        if (!p->y_stage) {
            void *q;
            SPMV_RETURN_IF(p->arena.alloc(&q, sizeof(double) * (size_t)std::max<int64_t>(p->m, 1)));
            p->y_stage = (double *)q;
        }
        dy = p->y_stage;
    }
    SPMV_RETURN_IF(dispatch(p, dx, dy));
    SPMV_RETURN_IF(launch_scale(p, dy, alpha));
    if (y_staged) {
        p->y_staged = true;
        if (!(flags & SPMV_ASYNC) || !(flags & SPMV_X_DEVICE)) SPMV_HIP_TRY(hipStreamSynchronize(p->stream));
    } else if (!(flags & SPMV_Y_DEVICE)) {
        // opt_cusparse.cpp:82 -- D2H copy of y on every call
        if (p->m) SPMV_HIP_TRY(hipMemcpyAsync(y, dy, sizeof(double) * p->m, hipMemcpyDeviceToHost, p->stream));
        SPMV_HIP_TRY(hipStreamSynchronize(p->stream));
    } else if (!(flags & SPMV_ASYNC) || !(flags & SPMV_X_DEVICE)) {
        SPMV_HIP_TRY(hipStreamSynchronize(p->stream));
    }
    return SPMV_SUCCESS;
}

int spmv_fetch_y(spmv_plan_t p, double *y) {
    SPMV_CHECK_ARG(p != nullptr && (y != nullptr || p->m == 0), "plan or y is NULL");
    SPMV_CHECK_ARG(p->y_staged && p->y_stage, "spmv_fetch_y without a previous SPMV_Y_STAGED execute");
    SPMV_RETURN_IF(bind_device(p));
    if (p->m) SPMV_HIP_TRY(hipMemcpyAsync(y, p->y_stage, sizeof(double) * p->m, hipMemcpyDeviceToHost, p->stream));
    SPMV_HIP_TRY(hipStreamSynchronize(p->stream));
    return SPMV_SUCCESS;
}

int spmv_time(spmv_plan_t p, const double *x_dev, double *y_dev, int32_t iters, double *ms) {
    SPMV_CHECK_ARG(p != nullptr && ms != nullptr && iters > 0, "bad arguments");
    SPMV_RETURN_IF(bind_device(p));
    return time_on_stream(p->stream, iters, ms, [&] { return dispatch(p, x_dev, y_dev); });
}

}  // extern "C"

// ---- multi-vector execute (Y = A X, k interleaved right-hand sides) ---------
namespace spmv {

// Widths with a fused kernel (k_dia.hip, k_ell.hip), per format, widest first.
// Every width that beat K single-vector executes on the same plan is listed
// (DESIGN §3.7); a width that is not listed is cut narrower.
static const int kMultiWidthsDia[] = {8, 4, 2};
static const int kMultiWidthsEll[] = {8, 4, 2};

static bool multi_format_fused(const spmv_plan_s *p) {
    if (p->format == SPMV_FORMAT_DIA || p->format == SPMV_FORMAT_ELL) return true;
    // JDS: the sliced-ELL part alone; overflow rows (a second kernel adding
    // into y) take the generic path, as HYB does
    return p->format == SPMV_FORMAT_JDS && p->hyb.nnz == 0 && p->hyb.n_rows == 0;
}

static bool multi_width_listed(const spmv_plan_s *p, int w) {
    const int *tab = p->format == SPMV_FORMAT_DIA ? kMultiWidthsDia : kMultiWidthsEll;
    for (int i = 0; i < 3; ++i)
        if (tab[i] == w) return true;
    return false;
}

// The cut of k columns: greedily 8, 4, 2 (the listed widths), then single
// columns -- block starts are even.  A block is fused when the format has a
// kernel, its X and Y block addresses are 16-byte aligned and ldx, ldy are
// even; else each of its columns is a width-1 block of the generic path.
static void multi_cut(const spmv_plan_s *p, int32_t k, uintptr_t x_addr, int64_t ldx, uintptr_t y_addr, int64_t ldy,
                      std::vector<int32_t> &widths) {
    widths.clear();
    const bool fmt = multi_format_fused(p);
    const bool even = ldx % 2 == 0 && ldy % 2 == 0;
    int32_t j = 0;
    while (j < k) {
        int w = 1;
        for (int c : {8, 4, 2})
            if (k - j >= c && (!fmt || multi_width_listed(p, c))) {
                w = c;
                break;
            }
        const bool fused = w >= 2 && fmt && even && ((x_addr + sizeof(double) * (size_t)j) & 15) == 0 &&
                           ((y_addr + sizeof(double) * (size_t)j) & 15) == 0;
        if (fused) widths.push_back(w);
        else widths.insert(widths.end(), (size_t)w, 1);
        j += w;
    }
}

static int multi_check_args(int32_t k, const double *X, int64_t ldx, const double *Y, int64_t ldy, uint32_t flags) {
    (void)X;
    (void)Y;
    SPMV_CHECK_ARG(!(flags & (SPMV_X_STAGED | SPMV_Y_STAGED)),
                   "multi execute: SPMV_X_STAGED / SPMV_Y_STAGED are not supported");
    SPMV_CHECK_ARG(k >= 1 && k <= SPMV_MULTI_MAX, "multi execute: k outside [1, SPMV_MULTI_MAX]");
    SPMV_CHECK_ARG(ldx >= k, "multi execute: ldx < k");
    SPMV_CHECK_ARG(ldy >= k, "multi execute: ldy < k");
    return SPMV_SUCCESS;
}

// the column scratch of the generic path: n + m doubles of plain hipMalloc
// memory (COO adds into it with f64 atomics), allocated at the first use
static int multi_scratch(spmv_plan_s *p) {
    if (p->m_scratch) return SPMV_SUCCESS;
    const size_t keep = p->arena.vmm_min;
    p->arena.vmm_min = 0;
    void *q = nullptr;
    const int st = p->arena.alloc(&q, sizeof(double) * (size_t)std::max<int64_t>(p->n + p->m, 1));
    p->arena.vmm_min = keep;
    SPMV_RETURN_IF(st);
    p->m_scratch = (double *)q;
    return SPMV_SUCCESS;
}

// the launches of one multi execute on device blocks, on p->stream
static int multi_dispatch(spmv_plan_s *p, int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy) {
    if (p->m == 0) return SPMV_SUCCESS;
    std::vector<int32_t> widths;
    multi_cut(p, k, reinterpret_cast<uintptr_t>(X), ldx, reinterpret_cast<uintptr_t>(Y), ldy, widths);
    int32_t j = 0;
    for (const int32_t w : widths) {
        if (w >= 2) {
            if (p->format == SPMV_FORMAT_DIA) SPMV_RETURN_IF(launch_dia_multi(p, w, X + j, ldx, Y + j, ldy));
            else SPMV_RETURN_IF(launch_ell_multi(p, w, X + j, ldx, Y + j, ldy));
        } else {
            // a contiguous column (ld = 1, hence k = 1) is read / written in place
            const double *xs = X;
            double *ys = Y;
            if (ldx != 1 || ldy != 1) SPMV_RETURN_IF(multi_scratch(p));
            if (ldx != 1) {
                SPMV_RETURN_IF(launch_multi_copy(p, p->n, X + j, ldx, p->m_scratch, 1));
                xs = p->m_scratch;
            }
            if (ldy != 1) ys = p->m_scratch + p->n;
            SPMV_RETURN_IF(dispatch(p, xs, ys));
            if (ldy != 1) SPMV_RETURN_IF(launch_multi_copy(p, p->m, ys, 1, Y + j, ldy));
        }
        j += w;
    }
    return SPMV_SUCCESS;
}

// a host staging block of at least `need` doubles
static int multi_stage(spmv_plan_s *p, double **buf, int64_t *cap, int64_t need) {
    if (*buf && *cap >= need) return SPMV_SUCCESS;
    if (*buf) p->arena.free(*buf);
    *buf = nullptr;
    *cap = 0;
    void *q = nullptr;
    SPMV_RETURN_IF(p->arena.alloc(&q, sizeof(double) * (size_t)std::max<int64_t>(need, 1)));
    *buf = (double *)q;
    *cap = need;
    return SPMV_SUCCESS;
}

}  // namespace spmv

extern "C" {

int spmv_execute_multi(spmv_plan_t p, int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy,
                       uint32_t flags) {
    SPMV_RETURN_IF(multi_check_args(k, X, ldx, Y, ldy, flags));
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    SPMV_CHECK_ARG((X != nullptr || p->n == 0) && (Y != nullptr || p->m == 0), "multi execute: X or Y is NULL");
    SPMV_RETURN_IF(bind_device(p));
    p->y_staged = false;  // like any other non-staged execute (spmv_fetch_y)
    const int64_t kp = (k + 1) & ~1;  // staging pitch: host callers always qualify for the fused path
    const double *dX = X;
    double *dY = Y;
    int64_t dldx = ldx, dldy = ldy;
    if (!(flags & SPMV_X_DEVICE)) {
        SPMV_RETURN_IF(multi_stage(p, &p->mx_stage, &p->mx_cap, p->n * kp));
        if (p->n)
            SPMV_HIP_TRY(hipMemcpy2DAsync(p->mx_stage, sizeof(double) * kp, X, sizeof(double) * ldx,
                                          sizeof(double) * k, (size_t)p->n, hipMemcpyHostToDevice, p->stream));
        dX = p->mx_stage;
        dldx = kp;
    }
    if (!(flags & SPMV_Y_DEVICE)) {
        SPMV_RETURN_IF(multi_stage(p, &p->my_stage, &p->my_cap, p->m * kp));
        dY = p->my_stage;
        dldy = kp;
    }
    SPMV_RETURN_IF(multi_dispatch(p, k, dX, dldx, dY, dldy));
    if (!(flags & SPMV_Y_DEVICE)) {
        if (p->m)
            SPMV_HIP_TRY(hipMemcpy2DAsync(Y, sizeof(double) * ldy, dY, sizeof(double) * kp, sizeof(double) * k,
                                          (size_t)p->m, hipMemcpyDeviceToHost, p->stream));
        SPMV_HIP_TRY(hipStreamSynchronize(p->stream));
    } else if (!(flags & SPMV_ASYNC) || !(flags & SPMV_X_DEVICE)) {
        SPMV_HIP_TRY(hipStreamSynchronize(p->stream));
    }
    return SPMV_SUCCESS;
}

int spmv_multi_path(spmv_plan_t p, int32_t k, const double *X, int64_t ldx, const double *Y, int64_t ldy,
                    uint32_t flags, int32_t *widths, int32_t cap, int32_t *n_blocks) {
    SPMV_RETURN_IF(multi_check_args(k, X, ldx, Y, ldy, flags));
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    SPMV_CHECK_ARG(n_blocks != nullptr && (widths != nullptr || cap <= 0), "n_blocks or widths is NULL");
    // host blocks are staged at an aligned base with pitch k rounded up to even
    const int64_t kp = (k + 1) & ~1;
    const bool xd = (flags & SPMV_X_DEVICE) != 0, yd = (flags & SPMV_Y_DEVICE) != 0;
    std::vector<int32_t> w;
    multi_cut(p, k, xd ? reinterpret_cast<uintptr_t>(X) : 0, xd ? ldx : kp, yd ? reinterpret_cast<uintptr_t>(Y) : 0,
              yd ? ldy : kp, w);
    *n_blocks = (int32_t)w.size();
    for (int32_t b = 0; b < *n_blocks && b < cap; ++b) widths[b] = w[b];
    return SPMV_SUCCESS;
}

int spmv_time_multi(spmv_plan_t p, int32_t k, const double *X_dev, int64_t ldx, double *Y_dev, int64_t ldy,
                    int32_t iters, double *ms) {
    SPMV_RETURN_IF(multi_check_args(k, X_dev, ldx, Y_dev, ldy, 0));
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    SPMV_CHECK_ARG(ms != nullptr && iters > 0, "ms is NULL or iters < 1");
    SPMV_CHECK_ARG((X_dev != nullptr || p->n == 0) && (Y_dev != nullptr || p->m == 0), "multi execute: X or Y is NULL");
    SPMV_RETURN_IF(bind_device(p));
    p->y_staged = false;
    return time_on_stream(p->stream, iters, ms, [&] { return multi_dispatch(p, k, X_dev, ldx, Y_dev, ldy); });
}

}  // extern "C"

// ---- y = alpha * A x + beta * y (epilogues: k_csr / k_ell / k_dia.hip; second pass: k_axpby.hip) --
namespace spmv {

// One writer per row: CSR (every kernel), ELL, DIA, and JDS without overflow
// rows (its overflow kernel adds into a y the ELL part wrote) take alpha and
// beta in the store epilogue.  Every other plan runs its own kernels into a
// scratch vector and one axpby pass.
static bool axpby_fused(const spmv_plan_s *p) {
    // probe build: the generic route forced on any plan (tools/axpby_times.py)
    if (const char *e = probe_env("SPMV_LAUNCH_AXPBY_GENERIC"))
        if (std::atoi(e) != 0) return false;
    if (p->format == SPMV_FORMAT_CSR || p->format == SPMV_FORMAT_ELL || p->format == SPMV_FORMAT_DIA) return true;
    return p->format == SPMV_FORMAT_JDS && p->hyb.nnz == 0 && p->hyb.n_rows == 0;
}

// the generic path's row sums: m + 2 doubles of plain hipMalloc memory (COO
// adds into them with f64 atomics), allocated at the first use.  The spare
// doubles let t start at y's alignment modulo 16 (k_axpby.hip).
static int axpby_scratch(spmv_plan_s *p) {
    if (p->ab_scratch) return SPMV_SUCCESS;
    const size_t keep = p->arena.vmm_min;
    p->arena.vmm_min = 0;
    void *q = nullptr;
    const int st = p->arena.alloc(&q, sizeof(double) * (size_t)(p->m + 2));
    p->arena.vmm_min = keep;
    SPMV_RETURN_IF(st);
    p->ab_scratch = (double *)q;
    return SPMV_SUCCESS;
}

// the launches of one axpby execute on device x and y (beta != 0), on p->stream
static int axpby_dispatch(spmv_plan_s *p, const Axpby &ab, const double *x, double *y) {
    if (p->m == 0) return SPMV_SUCCESS;
    if (axpby_fused(p)) {
        switch (p->format) {
            case SPMV_FORMAT_CSR: return launch_csr(p, x, y, &ab);
            case SPMV_FORMAT_DIA: return launch_dia(p, x, y, &ab);
            default: return launch_ell(p, x, y, &ab);  // ELL, JDS without overflow rows
        }
    }
    SPMV_RETURN_IF(axpby_scratch(p));
    double *t = p->ab_scratch + ((reinterpret_cast<uintptr_t>(y) >> 3) & 1);
    SPMV_RETURN_IF(dispatch(p, x, t));
    return launch_axpby(p, y, t, ab);
}

}  // namespace spmv

extern "C" {

int spmv_execute_axpby(spmv_plan_t p, double alpha, const double *x, double beta, double *y, uint32_t flags) {
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    const bool staged = (flags & SPMV_X_STAGED) != 0;
    SPMV_CHECK_ARG((x != nullptr || p->n == 0 || staged) && (y != nullptr || p->m == 0), "x or y is NULL");
    SPMV_CHECK_ARG(!(flags & ~(SPMV_X_DEVICE | SPMV_Y_DEVICE | SPMV_ASYNC | SPMV_X_STAGED | SPMV_Y_STAGED)),
                   "spmv_execute_axpby: unknown flag bits");
    SPMV_CHECK_ARG(!(flags & SPMV_Y_STAGED), "spmv_execute_axpby: SPMV_Y_STAGED is not supported (y is an input)");
    SPMV_CHECK_ARG(!staged || p->x_stage != nullptr, "SPMV_X_STAGED without a previously staged x");
    // beta = 0 (either sign): y is never read; alpha * A x as spmv_execute_alpha
    if (beta == 0.0) return execute_impl(p, alpha, x, y, flags);
    SPMV_RETURN_IF(bind_device(p));
    p->y_staged = false;  // like any other non-staged execute (spmv_fetch_y)
    // every allocation comes first: out of memory leaves y untouched
    if (!staged && !(flags & SPMV_X_DEVICE) && !p->x_stage) {
        void *q;
        SPMV_RETURN_IF(p->arena.alloc(&q, sizeof(double) * (size_t)std::max<int64_t>(p->n, 1)));
        p->x_stage = (double *)q;
    }
    if (!(flags & SPMV_Y_DEVICE) && !p->y_stage) {
        void *q;
        SPMV_RETURN_IF(p->arena.alloc(&q, sizeof(double) * (size_t)std::max<int64_t>(p->m, 1)));
        p->y_stage = (double *)q;
    }
    if (p->m && !axpby_fused(p)) SPMV_RETURN_IF(axpby_scratch(p));
    const double *dx = x;
    double *dy = y;
    if (staged) {
        dx = p->x_stage;
        flags |= SPMV_X_DEVICE;
    } else if (!(flags & SPMV_X_DEVICE)) {
        if (p->n) SPMV_HIP_TRY(hipMemcpyAsync(p->x_stage, x, sizeof(double) * p->n, hipMemcpyHostToDevice, p->stream));
        dx = p->x_stage;
    }
    if (!(flags & SPMV_Y_DEVICE)) {
        // y is an input: a host y travels up, then down
        if (p->m) SPMV_HIP_TRY(hipMemcpyAsync(p->y_stage, y, sizeof(double) * p->m, hipMemcpyHostToDevice, p->stream));
        dy = p->y_stage;
    }
    const Axpby ab{alpha, beta};
    SPMV_RETURN_IF(axpby_dispatch(p, ab, dx, dy));
    if (!(flags & SPMV_Y_DEVICE)) {
        if (p->m) SPMV_HIP_TRY(hipMemcpyAsync(y, dy, sizeof(double) * p->m, hipMemcpyDeviceToHost, p->stream));
        SPMV_HIP_TRY(hipStreamSynchronize(p->stream));
    } else if (!(flags & SPMV_ASYNC) || !(flags & SPMV_X_DEVICE)) {
        SPMV_HIP_TRY(hipStreamSynchronize(p->stream));
    }
    return SPMV_SUCCESS;
}

int spmv_time_axpby(spmv_plan_t p, double alpha, const double *x_dev, double beta, double *y_dev, int32_t iters,
                    double *ms) {
    SPMV_CHECK_ARG(p != nullptr && ms != nullptr && iters > 0, "bad arguments");
    SPMV_CHECK_ARG((x_dev != nullptr || p->n == 0) && (y_dev != nullptr || p->m == 0), "x or y is NULL");
    SPMV_RETURN_IF(bind_device(p));
    p->y_staged = false;
    if (beta == 0.0)
        return time_on_stream(p->stream, iters, ms, [&]() -> int {
            SPMV_RETURN_IF(dispatch(p, x_dev, y_dev));
            return launch_scale(p, y_dev, alpha);
        });
    if (p->m && !axpby_fused(p)) SPMV_RETURN_IF(axpby_scratch(p));
    const Axpby ab{alpha, beta};
    return time_on_stream(p->stream, iters, ms, [&] { return axpby_dispatch(p, ab, x_dev, y_dev); });
}

int spmv_axpby_path(spmv_plan_t p, int32_t *fused) {
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    SPMV_CHECK_ARG(fused != nullptr, "fused out-pointer is NULL");
    *fused = axpby_fused(p) ? 1 : 0;
    return SPMV_SUCCESS;
}

}  // extern "C"

// ---- value refresh (new values on the plan's pattern; kernels: k_update.hip) --
extern "C" {

int spmv_plan_update_prepare(spmv_plan_t p, const int64_t *row_ptr, const int32_t *col_idx, uint32_t flags) {
    SPMV_CHECK_ARG(!(flags & ~SPMV_CSR_DEVICE), "spmv_plan_update_prepare: flag bits other than SPMV_CSR_DEVICE");
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    SPMV_CHECK_ARG(row_ptr != nullptr, "row_ptr is NULL");
    SPMV_CHECK_ARG(p->nnz == 0 || col_idx != nullptr, "col_idx is NULL");
    if (p->upd.prepared) return SPMV_SUCCESS;
    if (p->nnz == 0 || p->m == 0) {
        p->upd.prepared = true;  // nothing to map
        return SPMV_SUCCESS;
    }
    SPMV_RETURN_IF(bind_device(p));
    // the pattern in HBM (a host pattern is staged, as create_via_device does)
    // with values 1 .. nnz; the builders run on the null stream
    // (a plan of the transpose was created from A: the source has p->n rows)
    const int64_t src_m = p->transposed ? p->n : p->m;
    DevScratch scratch(nullptr);
    const int64_t *d_rp = row_ptr;
    const int32_t *d_col = col_idx;
    if (!(flags & SPMV_CSR_DEVICE)) {
        int64_t *rp = nullptr;
        int32_t *col = nullptr;
        SPMV_RETURN_IF(scratch.alloc(&rp, (size_t)src_m + 1, "row_ptr staging"));
        SPMV_RETURN_IF(scratch.alloc(&col, (size_t)p->nnz, "col_idx staging"));
        SPMV_HIP_TRY(hipMemcpy(rp, row_ptr, 8 * (size_t)(src_m + 1), hipMemcpyHostToDevice));
        SPMV_HIP_TRY(hipMemcpy(col, col_idx, 4 * (size_t)p->nnz, hipMemcpyHostToDevice));
        d_rp = rp;
        d_col = col;
    }
    double *d_val = nullptr;
    SPMV_RETURN_IF(scratch.alloc(&d_val, (size_t)p->nnz, "shadow values"));
    SPMV_RETURN_IF(launch_iota_values(nullptr, d_val, p->nnz));
    if (p->transposed) {
        // A's pattern with the values 1 .. nnz, transposed: the shadow's
        // values then name A's entries, and the maps point into A's order
        const void *ptrs[2] = {d_rp, d_col};
        SPMV_RETURN_IF(check_device_arrays(ptrs, 2, p->device, "spmv_plan_update_prepare"));
        SPMV_RETURN_IF(validate_csr_device(d_rp, src_m, d_col, p->nnz, p->m));
        int64_t *t_rp = nullptr;
        int32_t *t_col = nullptr;
        double *t_val = nullptr;
        SPMV_RETURN_IF(scratch.alloc(&t_rp, (size_t)p->m + 1, "transposed row_ptr"));
        SPMV_RETURN_IF(scratch.alloc(&t_col, (size_t)p->nnz, "transposed col_idx"));
        SPMV_RETURN_IF(scratch.alloc(&t_val, (size_t)p->nnz, "transposed shadow values"));
        SPMV_RETURN_IF(transpose_csr_device(src_m, p->m, p->nnz, d_rp, d_col, d_val, t_rp, t_col, t_val, nullptr));
        d_rp = t_rp;
        d_col = t_col;
        d_val = t_val;
    }
    // the shadow: the plan's resolved options, no placement search, no VMM
    spmv_options_t o = p->opts;
    o.placement = SPMV_PLACEMENT_PLAIN;
    o.build = SPMV_BUILD_DEVICE;
    spmv_plan_t shadow = nullptr;
    int st = create_device_impl(p->m, p->n, p->nnz, d_rp, d_col, d_val, &o, &shadow, nullptr);
    if (st == SPMV_ERROR_INVALID_VALUE || st == SPMV_ERROR_NOT_SUPPORTED) {
        // the plan's own build took these options: it is the pattern that differs
        set_error(std::string("spmv_plan_update_prepare: the pattern does not reproduce the plan's layout (") +
                  last_error() + ")");
        st = SPMV_ERROR_INVALID_VALUE;
    }
    if (st != SPMV_SUCCESS) return st;
    st = bind_device(p);
    if (st == SPMV_SUCCESS) st = update_prepare_from_shadow(p, shadow);
    const std::string msg = last_error();
    (void)spmv_plan_destroy(shadow);
    set_error(msg);
    return st;
}

int spmv_plan_update_values(spmv_plan_t p, const double *val, uint32_t flags) {
    SPMV_CHECK_ARG(!(flags & ~(SPMV_VAL_DEVICE | SPMV_ASYNC)),
                   "spmv_plan_update_values: flag bits other than SPMV_VAL_DEVICE and SPMV_ASYNC");
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    SPMV_CHECK_ARG(p->nnz == 0 || val != nullptr, "val is NULL");
    SPMV_CHECK_ARG(!(flags & SPMV_ASYNC) || (flags & SPMV_VAL_DEVICE), "SPMV_ASYNC without SPMV_VAL_DEVICE");
    SPMV_CHECK_ARG(p->upd.prepared,
                   "spmv_plan_update_values: plan not prepared (spmv_plan_update_prepare comes first)");
    if (p->nnz == 0 || p->m == 0) return SPMV_SUCCESS;
    SPMV_RETURN_IF(bind_device(p));
    const double *d_val = val;
    if (flags & SPMV_VAL_DEVICE) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, val) != hipSuccess || a.type != hipMemoryTypeDevice || a.device != p->device) {
            (void)hipGetLastError();
            set_error("spmv_plan_update_values: SPMV_VAL_DEVICE needs device memory on the plan's device");
            return SPMV_ERROR_INVALID_VALUE;
        }
    } else {
        if (!p->upd.stage) {
            // plain hipMalloc memory, like the maps (no 2-MB rounding)
            const size_t keep = p->arena.vmm_min;
            p->arena.vmm_min = 0;
            void *q = nullptr;
            const int st = p->arena.alloc(&q, sizeof(double) * (size_t)p->nnz);
            p->arena.vmm_min = keep;
            SPMV_RETURN_IF(st);
            p->upd.stage = (double *)q;
        }
        SPMV_HIP_TRY(hipMemcpyAsync(p->upd.stage, val, sizeof(double) * (size_t)p->nnz, hipMemcpyHostToDevice,
                                    p->stream));
        d_val = p->upd.stage;
    }
    SPMV_RETURN_IF(launch_update_values(p, d_val));
    if (!(flags & SPMV_ASYNC)) SPMV_HIP_TRY(hipStreamSynchronize(p->stream));
    return SPMV_SUCCESS;
}

}  // extern "C"

struct spmv_graph_s {
    spmv_plan_t plan = nullptr;  // launches use the plan's stream; destroy does not touch it
    int device = 0;              // the plan's device, for destroy
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    int32_t reps = 0;
};

namespace spmv {

// Capture `reps` dispatches on a private stream (the plan's stream may be the
// null stream, which cannot be captured); the plan's stream is restored
// whatever happens.
static int graph_capture(spmv_plan_s *p, const double *x, double *y, int32_t reps, hipGraph_t *out) {
    hipStream_t cs = nullptr;
    SPMV_HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    const hipStream_t saved = p->stream;
    const int saved_prof = p->prof_k;
    p->stream = cs;
    p->prof_k = -1;  // no profile events inside the graph
    int st = SPMV_SUCCESS;
    hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        for (int32_t r = 0; r < reps && st == SPMV_SUCCESS; ++r) st = dispatch(p, x, y);
        hipGraph_t g = nullptr;
        const hipError_t e2 = hipStreamEndCapture(cs, &g);
        if (st == SPMV_SUCCESS && e2 != hipSuccess) e = e2;
        if (st == SPMV_SUCCESS && e == hipSuccess) *out = g;
        else if (g) (void)hipGraphDestroy(g);
    }
    p->stream = saved;
    p->prof_k = saved_prof;
    (void)hipStreamDestroy(cs);
    if (st != SPMV_SUCCESS) return st;
    if (e != hipSuccess) {
        set_error(std::string("graph capture: ") + hipGetErrorString(e));
        (void)hipGetLastError();
        return SPMV_ERROR_HIP;
    }
    return SPMV_SUCCESS;
}

}  // namespace spmv

extern "C" {

int spmv_graph_create(spmv_plan_t p, const double *x_dev, double *y_dev, int32_t reps, spmv_graph_t *out) {
    SPMV_CHECK_ARG(out != nullptr, "graph out-pointer is NULL");
    *out = nullptr;
    SPMV_CHECK_ARG(p != nullptr && reps > 0, "bad arguments");
    SPMV_CHECK_ARG((x_dev != nullptr || p->n == 0) && (y_dev != nullptr || p->m == 0), "x or y is NULL");
    if (p->format == SPMV_FORMAT_CSS) {
        // the sweep's progress flags are tagged with a per-launch sequence
        // number passed as a kernel argument: a replayed graph would repeat it
        set_error("spmv_graph_create: CSS plans cannot be replayed from a graph");
        return SPMV_ERROR_NOT_SUPPORTED;
    }
    SPMV_RETURN_IF(bind_device(p));
    hipGraph_t g = nullptr;
    SPMV_RETURN_IF(graph_capture(p, x_dev, y_dev, reps, &g));
    hipGraphExec_t ex = nullptr;
    const hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(g);
        set_error(std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
        (void)hipGetLastError();
        return SPMV_ERROR_HIP;
    }
    spmv_graph_s *G = new (std::nothrow) spmv_graph_s;
    if (!G) {
        (void)hipGraphExecDestroy(ex);
        (void)hipGraphDestroy(g);
        set_error("host allocation of the graph failed");
        return SPMV_ERROR_OUT_OF_MEMORY;
    }
    G->plan = p;
    G->device = p->device;
    G->graph = g;
    G->exec = ex;
    G->reps = reps;
    *out = G;
    return SPMV_SUCCESS;
}

int spmv_graph_launch(spmv_graph_t G, uint32_t flags) {
    SPMV_CHECK_ARG(G != nullptr && G->exec != nullptr, "graph is NULL");
    SPMV_RETURN_IF(bind_device(G->plan));
    SPMV_HIP_TRY(hipGraphLaunch(G->exec, G->plan->stream));
    if (!(flags & SPMV_ASYNC)) SPMV_HIP_TRY(hipStreamSynchronize(G->plan->stream));
    return SPMV_SUCCESS;
}

int spmv_graph_time(spmv_graph_t G, int32_t launches, double *ms) {
    SPMV_CHECK_ARG(G != nullptr && G->exec != nullptr && ms != nullptr && launches > 0, "bad arguments");
    SPMV_RETURN_IF(bind_device(G->plan));
    const hipStream_t s = G->plan->stream;
    return time_on_stream(s, launches, ms, [&]() -> int {
        SPMV_HIP_TRY(hipGraphLaunch(G->exec, s));
        return SPMV_SUCCESS;
    });
}

int spmv_graph_destroy(spmv_graph_t G) {
    if (!G) return SPMV_SUCCESS;
    // the plan may already be gone (the header asks for graphs first, but a
    // destroy must not read it): bind the recorded device only
    (void)hipSetDevice(G->device);
    if (G->exec) (void)hipGraphExecDestroy(G->exec);
    if (G->graph) (void)hipGraphDestroy(G->graph);
    delete G;
    return SPMV_SUCCESS;
}

static const char *const kPhases[][3] = {
    {"", "", ""},           {"csr", "", ""},   {"ell", "", ""},     {"tile", "fixup", ""},
    {"dia", "", ""},        {"ell", "overflow", ""}, {"sweep", "", ""}, {"zero_y", "segment", ""},
    {"ell", "overflow", ""}};

const char *spmv_phase_name(spmv_plan_t p, int32_t k) {
    static const char *const kBinPhases[8] = {"mul", "sum", "mul.1", "sum.1", "mul.2", "sum.2", "mul.3", "sum.3"};
    if (p && p->format == SPMV_FORMAT_BIN) {
        if (!p->bin.reuse) return k == 0 ? "mul" : k == 1 ? "sum" : "";  // groups' Mul launches: one phase
        return k >= 0 && k < 8 && k < 2 * p->bin.G ? kBinPhases[k] : "";
    }
    if (!p || k < 0 || k > 2 || p->format < 0 || p->format > SPMV_FORMAT_JDS) return "";
    return kPhases[p->format][k];
}

int spmv_profile(spmv_plan_t p, const double *x_dev, double *y_dev, int32_t iters, double *phase_ms,
                 int32_t max_phases, int32_t *n_phases) {
    SPMV_CHECK_ARG(p != nullptr && iters > 0 && phase_ms != nullptr && n_phases != nullptr && max_phases > 0,
                   "bad arguments");
    SPMV_RETURN_IF(bind_device(p));
    for (auto &e : p->prof_ev) SPMV_HIP_TRY(hipEventCreate(&e));
    std::vector<double> acc(8, 0.0);
    int nph = 1, st = SPMV_SUCCESS;
    for (int i = 0; i < iters && st == SPMV_SUCCESS; ++i) {
        p->prof_k = 0;
        (void)hipEventRecord(p->prof_ev[0], p->stream);
        st = dispatch(p, x_dev, y_dev);
        const int k = p->prof_k;
        p->prof_k = -1;
        (void)hipEventRecord(p->prof_ev[k + 1], p->stream);
        if (hipEventSynchronize(p->prof_ev[k + 1]) != hipSuccess) {
            st = SPMV_ERROR_HIP;
            set_error("spmv_profile: event synchronisation failed");
            break;
        }
        nph = k + 1;
        for (int j = 0; j <= k; ++j) {
            float f = 0;
            (void)hipEventElapsedTime(&f, p->prof_ev[j], p->prof_ev[j + 1]);
            acc[j] += f;
        }
    }
    p->prof_k = -1;
    for (auto &e : p->prof_ev) (void)hipEventDestroy(e);
    *n_phases = nph;
    for (int j = 0; j < std::min(nph, max_phases); ++j) phase_ms[j] = acc[j] / iters;
    return st;
}

// internal (not in the public header): the CSS per-wave timestamps of the
// last launch when the plan was built with SPMV_CSS_DEBUG & 32
int64_t spmv_css_timestamps(spmv_plan_t p, uint64_t *out, int64_t cap) {
    if (!p || p->format != SPMV_FORMAT_CSS || !p->css.tstamp) return -1;
    const int64_t n = (int64_t)p->css.P * p->css.nwg * (kCssWorkers + 2);
    if (out && cap >= n && hipMemcpy(out, p->css.tstamp, 8 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return n;
}

// internal: the CSS block/list layout (bstart [P*nwg+1], woff [P*nwg*15+1])
int spmv_css_layout(spmv_plan_t p, int64_t *bstart, int64_t *woff) {
    if (!p || p->format != SPMV_FORMAT_CSS) return -1;
    const int64_t nb = (int64_t)p->css.P * p->css.nwg;
    if (hipMemcpy(bstart, p->css.bstart, 8 * (size_t)(nb + 1), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(woff, p->css.woff, 8 * (size_t)(nb * kCssWorkers + 1), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return 0;
}

// internal (experiment): give the BIN product buffer a fresh allocation (the
// old one is kept until the plan is destroyed, so the new one lands elsewhere)
int spmv_bin_realloc_prod(spmv_plan_t p) {
    if (!p || p->format != SPMV_FORMAT_BIN || !p->bin.prod) return -1;
    void *q = nullptr;
    if (p->arena.alloc(&q, sizeof(double) * (size_t)(std::max<int64_t>(p->bin.prod_cap, 1) + kBinProdSlack)) !=
        SPMV_SUCCESS)
        return -1;
    p->bin.prod = (double *)q;
    return 0;
}

// internal (placement experiments): the BIN product buffer
int spmv_bin_prod(spmv_plan_t p, void **buf, int64_t *bytes) {
    if (!p || p->format != SPMV_FORMAT_BIN || !p->bin.prod || !buf || !bytes) return -1;
    *buf = p->bin.prod;
    *bytes = 8 * std::max<int64_t>(p->bin.prod_cap, 1);
    return 0;
}

int spmv_plan_built_on_device(spmv_plan_t p, int32_t *on_device) {
    SPMV_CHECK_ARG(p != nullptr && on_device != nullptr, "NULL plan or out-pointer");
    *on_device = p->built_on_device;
    return SPMV_SUCCESS;
}

int spmv_plan_info(spmv_plan_t p, spmv_plan_info_t *info) {
    SPMV_CHECK_ARG(p != nullptr && info != nullptr, "NULL argument");
    std::memset(info, 0, sizeof(*info));
    info->format = p->format;
    info->device = p->device;
    info->m = p->m;
    info->n = p->n;
    info->nnz = p->nnz;
    info->stored_slots = p->stored_slots;
    info->device_bytes = p->arena.bytes;
    info->algo_bytes = p->algo_bytes;
    info->row_ptr_bytes = p->csr.rp64 ? 8 : 4;
    info->csr_lanes = p->format == SPMV_FORMAT_HYB ? p->hyb.lanes : p->csr.lanes;
    info->ell_width = p->ell.max_width;
    info->ss_sigma = p->ss.sigma;
    info->n_diags = p->dia.n_diags;
    info->css_passes = p->css.P;
    info->css_slabs = p->css.S;
    info->n_kernels = p->n_kernels;
    info->overflow_nnz = p->hyb.nnz;
    info->empty_rows = p->empty_rows;
    info->css_split_rows = p->css.split_rows;
    std::strncpy(info->kernel, p->kernel_name.c_str(), sizeof(info->kernel) - 1);
    if (p->format == SPMV_FORMAT_BIN) {
        info->bin_bins = p->bin.n_bins;
        info->bin_strips = p->bin.n_strips;
        info->bin_strip_cols = p->bin.strip;
        info->bin_pad = 1 << p->bin.pad_log;
        info->bin_sum_waves = p->bin.sum_waves;
        info->bin_groups = p->bin.G;
        info->bin_long_len = (int32_t)p->bin.long_len;
        info->bin_product_order = p->bin.mo ? SPMV_BIN_ORDER_MUL : SPMV_BIN_ORDER_SUM;
        info->bin_long_rows = p->bin.long_rows;
        info->bin_long_pieces = p->bin.long_pieces;
        info->bin_products = p->bin.prod_cap;
        info->bin_long_entries = p->bin.long_entries;
        info->bin_sum_entries = p->bin.n_entries;
    }
    const std::vector<float> *pm = nullptr;
    if (p->format == SPMV_FORMAT_BIN) {
        info->placement = p->bin.placement;
        pm = &p->bin.placement_ms;
    } else if (p->format == SPMV_FORMAT_DIA) {
        info->placement = p->dia.placement;
        pm = &p->dia.placement_ms;
    } else {
        info->placement = p->arena.maps.empty() ? SPMV_PLACEMENT_PLAIN : SPMV_PLACEMENT_VMM;
    }
    if (pm && !pm->empty()) {
        info->placement_candidates = (int32_t)pm->size();
        info->placement_best_ms = *std::min_element(pm->begin(), pm->end());
        info->placement_worst_ms = *std::max_element(pm->begin(), pm->end());
    }
    return SPMV_SUCCESS;
}

const char *spmv_status_string(int s) {
    switch (s) {
        case SPMV_SUCCESS: return "success";
        case SPMV_ERROR_INVALID_VALUE: return "invalid value";
        case SPMV_ERROR_NOT_SUPPORTED: return "not supported by this format";
        case SPMV_ERROR_OUT_OF_MEMORY: return "out of memory";
        case SPMV_ERROR_HIP: return "HIP runtime error";
        case SPMV_ERROR_IO: return "I/O error";
        case SPMV_ERROR_NO_DEVICE: return "no usable gfx950 device";
    }
    return "unknown status";
}

const char *spmv_last_error(void) { return spmv::last_error(); }

int spmv_partition_rows(const int64_t *row_ptr, int64_t m, int32_t parts, int64_t *cuts) {
    SPMV_CHECK_ARG(row_ptr && cuts && parts > 0 && m >= 0, "bad arguments");
    const int64_t nnz = row_ptr[m];
    cuts[0] = 0;
    for (int k = 1; k < parts; ++k) {
        const int64_t target = (int64_t)((__int128)nnz * k / parts);
        cuts[k] = std::lower_bound(row_ptr, row_ptr + m, target) - row_ptr;
        if (cuts[k] < cuts[k - 1]) cuts[k] = cuts[k - 1];
    }
    cuts[parts] = m;
    return SPMV_SUCCESS;
}

}  // extern "C"
