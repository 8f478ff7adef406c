// capi.cpp -- the C-ABI of include/spmv_hip.h apart from the plan life cycle
// (capi_create.cpp) and the per-call side (capi_execute.cpp): the error
// string, value refresh, plan info and the internal accessors.  Every entry
// point returns an int status; nothing exit()s.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "build_util.hpp"

namespace spmv {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
const char *last_error() { return g_err.c_str(); }

}  // namespace spmv

using namespace spmv;

extern "C" {

int spmv_api_version(void) { return SPMV_HIP_API_VERSION; }

// ---- value refresh (new values on the plan's pattern; kernels: k_update.hip) --
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
    // the pattern in HBM (a host pattern is staged, as a host CSR is for the
    // device builders) with values 1 .. nnz; the builders run on the null stream
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
    const DevCsr S{p->m, p->n, p->nnz, nullptr, d_rp, d_col, d_val};
    spmv_plan_t shadow = nullptr;
    int st = create_on_device(S, &o, &shadow);
    if (st == kNeedHostBuild) st = create_staged_on_host(S, o, &shadow);
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
        const void *q = val;
        SPMV_RETURN_IF(check_device_arrays(&q, 1, p->device, "spmv_plan_update_values",
                                           ": SPMV_VAL_DEVICE needs device memory on the plan's device"));
    } else {
        if (!p->upd.stage) {
            // plain hipMalloc memory, like the maps (no 2-MB rounding)
            void *q = nullptr;
            SPMV_RETURN_IF(p->arena.alloc_plain(&q, sizeof(double) * (size_t)p->nnz));
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

// internal (not in the public header; probe build): the CSS per-wave
// timestamps of the last launch when the plan was built with SPMV_CSS_DEBUG & 32
int64_t spmv_css_timestamps(spmv_plan_t p, uint64_t *out, int64_t cap) {
    if (!p || p->format != SPMV_FORMAT_CSS || !p->css.tstamp) return -1;
    const int64_t n = (int64_t)p->css.P * p->css.nwg * (kCssWorkers + 2);
    if (out && cap >= n && hipMemcpy(out, p->css.tstamp, 8 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return n;
}

// internal (not in the public header; tools/placement_probe.py): the BIN product buffer
int spmv_bin_prod(spmv_plan_t p, void **buf, int64_t *bytes) {
    if (!p || p->format != SPMV_FORMAT_BIN || !p->bin.prod || !buf || !bytes) return -1;
    *buf = p->bin.prod;
    *bytes = 8 * std::max<int64_t>(p->bin.prod_cap, 1);
    return 0;
}

int spmv_plan_is_transposed(spmv_plan_t p, int32_t *transposed) {
    SPMV_CHECK_ARG(p != nullptr && transposed != nullptr, "NULL plan or out-pointer");
    *transposed = p->transposed;
    return SPMV_SUCCESS;
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
