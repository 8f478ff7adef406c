// capi_execute.cpp -- the per-call side of include/spmv_hip.h: execute (one
// vector, k vectors, alpha and beta, with dot products), the conjugate-gradient
// solver, timing, graphs, the phase profile.
// Every entry point returns an int status.
#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "build_util.hpp"

namespace spmv {

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

int bind_device(const spmv_plan_s *p) {
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

// the staging vector *buf of the plan (x_stage, y_stage: `count` doubles),
// allocated at the first use
static int ensure_stage(spmv_plan_s *p, double **buf, int64_t count) {
    return *buf ? SPMV_SUCCESS : plan_alloc(p, buf, count);
}

// How every execute ends, once the copy of a host y is queued: a host y is
// waited for; a device y too, unless the call is SPMV_ASYNC and x was on the
// device as well (a host x must be free to change on return).
static int finish_execute(const spmv_plan_s *p, uint32_t flags, bool host_y) {
    if (host_y || !(flags & SPMV_ASYNC) || !(flags & SPMV_X_DEVICE)) SPMV_HIP_TRY(hipStreamSynchronize(p->stream));
    return SPMV_SUCCESS;
}

// JDS without overflow rows: the sliced-ELL part alone, one writer per row.
// (With overflow rows a second kernel adds into the y the ELL part wrote.)
static bool jds_without_overflow(const spmv_plan_s *p) {
    return p->format == SPMV_FORMAT_JDS && p->hyb.nnz == 0 && p->hyb.n_rows == 0;
}

// ---- y = alpha * A x + beta * y (epilogues: k_csr / k_ell / k_dia.hip; second pass: k_axpby.hip) --

// One writer per row: CSR (every kernel), ELL, DIA, and JDS without overflow
// rows take alpha and beta in the store epilogue.  Every other plan runs its
// own kernels into a scratch vector and one axpby pass.
static bool axpby_fused(const spmv_plan_s *p) {
    // probe build: the generic route forced on any plan (tools/axpby_times.py)
    if (const char *e = probe_env("SPMV_LAUNCH_AXPBY_GENERIC"))
        if (std::atoi(e) != 0) return false;
    if (p->format == SPMV_FORMAT_CSR || p->format == SPMV_FORMAT_ELL || p->format == SPMV_FORMAT_DIA) return true;
    return jds_without_overflow(p);
}

// the generic path's row sums (beta != 0 on a plan that is not fused): m + 2
// doubles of plain hipMalloc memory (COO adds into them with f64 atomics),
// allocated at the first use.  The spare doubles let t start at y's alignment
// modulo 16 (k_axpby.hip).
static int axpby_scratch(spmv_plan_s *p, double beta) {
    if (beta == 0.0 || p->m == 0 || axpby_fused(p) || p->ab_scratch) return SPMV_SUCCESS;
    void *q = nullptr;
    SPMV_RETURN_IF(p->arena.alloc_plain(&q, sizeof(double) * (size_t)(p->m + 2)));
    p->ab_scratch = (double *)q;
    return SPMV_SUCCESS;
}

// the launches of y = alpha * A x + beta * y on device x and y, on p->stream.
// beta = 0 (either sign): y is never read; A x, then the scale by alpha.
static int axpby_dispatch(spmv_plan_s *p, const Axpby &ab, const double *x, double *y) {
    if (ab.beta == 0.0) {
        SPMV_RETURN_IF(dispatch(p, x, y));
        return launch_scale(p, y, ab.alpha);
    }
    if (p->m == 0) return SPMV_SUCCESS;
    if (axpby_fused(p)) {
        switch (p->format) {
            case SPMV_FORMAT_CSR: return launch_csr(p, x, y, &ab);
            case SPMV_FORMAT_DIA: return launch_dia(p, x, y, &ab);
            default: return launch_ell(p, x, y, &ab);  // ELL, JDS without overflow rows
        }
    }
    SPMV_RETURN_IF(axpby_scratch(p, ab.beta));
    double *t = p->ab_scratch + ((reinterpret_cast<uintptr_t>(y) >> 3) & 1);
    SPMV_RETURN_IF(dispatch(p, x, t));
    return launch_axpby(p, y, t, ab);
}

// The body of spmv_execute, spmv_execute_alpha (beta = 0) and
// spmv_execute_axpby: the flag rules of each, x and y staged where they are
// host memory, the launches, the copy back.
static int execute_impl(spmv_plan_t p, const Axpby &ab, const double *x, double *y, uint32_t flags, bool axpby) {
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    const bool staged = (flags & SPMV_X_STAGED) != 0;
    const bool y_staged = !axpby && (flags & SPMV_Y_STAGED) != 0;
    SPMV_CHECK_ARG((x != nullptr || p->n == 0 || staged) && (y != nullptr || p->m == 0 || y_staged),
                   "x or y is NULL");
    if (axpby) {
        SPMV_CHECK_ARG(!(flags & ~(SPMV_X_DEVICE | SPMV_Y_DEVICE | SPMV_ASYNC | SPMV_X_STAGED | SPMV_Y_STAGED)),
                       "spmv_execute_axpby: unknown flag bits");
        SPMV_CHECK_ARG(!(flags & SPMV_Y_STAGED), "spmv_execute_axpby: SPMV_Y_STAGED is not supported (y is an input)");
    } else {
        SPMV_CHECK_ARG(!(y_staged && (flags & SPMV_Y_DEVICE)), "SPMV_Y_STAGED with SPMV_Y_DEVICE");
    }
    SPMV_CHECK_ARG(!staged || p->x_stage != nullptr, "SPMV_X_STAGED without a previously staged x");
    SPMV_RETURN_IF(bind_device(p));
    // spmv_fetch_y serves the y of the latest execute only when that execute
    // was SPMV_Y_STAGED: any other execute (device y, host y) clears the mark
    p->y_staged = false;
    const bool x_host = !staged && !(flags & SPMV_X_DEVICE);
    const bool y_dev = (flags & SPMV_Y_DEVICE) != 0;
    if (staged) flags |= SPMV_X_DEVICE;
    // every allocation comes first: out of memory leaves y untouched
    if (x_host) SPMV_RETURN_IF(ensure_stage(p, &p->x_stage, p->n));
    if (!y_dev) SPMV_RETURN_IF(ensure_stage(p, &p->y_stage, p->m));
    SPMV_RETURN_IF(axpby_scratch(p, ab.beta));
    const double *dx = x_host || staged ? p->x_stage : x;
    double *dy = y_dev ? y : p->y_stage;
    // opt_cusparse.cpp:72 -- H2D copy of x on every call
    if (x_host && p->n) SPMV_HIP_TRY(hipMemcpyAsync(p->x_stage, x, sizeof(double) * p->n, hipMemcpyHostToDevice, p->stream));
    // beta != 0: y is an input: a host y travels up, then down
    if (ab.beta != 0.0 && !y_dev && p->m)
        SPMV_HIP_TRY(hipMemcpyAsync(p->y_stage, y, sizeof(double) * p->m, hipMemcpyHostToDevice, p->stream));
    SPMV_RETURN_IF(axpby_dispatch(p, ab, dx, dy));
    const bool y_host = !y_dev && !y_staged;
    p->y_staged = y_staged;
    // opt_cusparse.cpp:82 -- D2H copy of y on every call
    if (y_host && p->m) SPMV_HIP_TRY(hipMemcpyAsync(y, dy, sizeof(double) * p->m, hipMemcpyDeviceToHost, p->stream));
    return finish_execute(p, flags, y_host);
}

// ---- y = A x with w . y and y . y (epilogues: k_csr / k_ell / k_dia.hip; second pass, finish: k_dot.hip) --

// The workgroups of the plan's fused dot launch (0: it has none).  One writer
// per row: CSR (every kernel), DIA, ELL and JDS without overflow rows; a plan
// with nothing stored (nnz = 0) takes the generic path after its zero fill
// (DESIGN §3.11).
static int64_t dot_fused_blocks(const spmv_plan_s *p) {
    if (p->nnz == 0) return 0;
    switch (p->format) {
        case SPMV_FORMAT_CSR: return csr_dot_blocks(p);
        case SPMV_FORMAT_DIA: return dia_dot_blocks(p);
        case SPMV_FORMAT_ELL: return ell_dot_blocks(p);
        case SPMV_FORMAT_JDS: return jds_without_overflow(p) ? ell_dot_blocks(p) : 0;
        default: return 0;
    }
}
static bool dot_fused(const spmv_plan_s *p) { return dot_fused_blocks(p) > 0; }

// the slots one dot execute writes: a function of the plan alone
static int64_t dot_slots(const spmv_plan_s *p) {
    const int64_t f = dot_fused_blocks(p);
    return f > 0 ? f : dot_rows_blocks(p->m);
}

// the plan's partials, 2 doubles per slot, and behind them the 2 doubles a
// host `dots` is copied from: plain hipMalloc memory, allocated at the first use
static int dot_partials(spmv_plan_s *p) {
    if (p->dot_part) return SPMV_SUCCESS;
    void *q = nullptr;
    SPMV_RETURN_IF(p->arena.alloc_plain(&q, sizeof(double) * (size_t)(2 * dot_slots(p) + 2)));
    p->dot_part = (double *)q;
    return SPMV_SUCCESS;
}

// the launches of one dot execute on device x, y, w (or null) and dots, on
// p->stream: every slot is written by its workgroup, then one workgroup adds them
static int dot_dispatch(spmv_plan_s *p, const double *x, double *y, const double *w, double *dots) {
    const DotArgs d{w, p->dot_part};
    if (dot_fused(p)) {
        switch (p->format) {
            case SPMV_FORMAT_CSR: SPMV_RETURN_IF(launch_csr(p, x, y, nullptr, &d)); break;
            case SPMV_FORMAT_DIA: SPMV_RETURN_IF(launch_dia(p, x, y, nullptr, &d)); break;
            default: SPMV_RETURN_IF(launch_ell(p, x, y, nullptr, &d));  // ELL, JDS without overflow rows
        }
    } else {
        SPMV_RETURN_IF(dispatch(p, x, y));
        SPMV_RETURN_IF(launch_dot_rows(p, y, w, p->dot_part));
    }
    return launch_dot_finish(p, p->dot_part, dot_slots(p), dots);
}

// The body of spmv_execute_dot (ms null) and spmv_time_dot (ms: device
// buffers, `iters` dispatches between two events).
static int dot_impl(spmv_plan_t p, const double *x, double *y, const double *w, double *dots, uint32_t flags,
                    int32_t iters, double *ms) {
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    const bool timed = ms != nullptr;
    const bool staged = (flags & SPMV_X_STAGED) != 0;
    SPMV_CHECK_ARG((x != nullptr || p->n == 0 || staged) && (y != nullptr || p->m == 0), "x or y is NULL");
    SPMV_CHECK_ARG(dots != nullptr, "spmv_execute_dot: dots is NULL");
    SPMV_CHECK_ARG(!(flags & ~(SPMV_X_DEVICE | SPMV_Y_DEVICE | SPMV_ASYNC | SPMV_X_STAGED | SPMV_Y_STAGED |
                               SPMV_W_DEVICE | SPMV_DOTS_DEVICE)),
                   "spmv_execute_dot: unknown flag bits");
    SPMV_CHECK_ARG(!(flags & SPMV_Y_STAGED), "spmv_execute_dot: SPMV_Y_STAGED is not supported");
    const uint32_t all_dev = SPMV_X_DEVICE | SPMV_Y_DEVICE | SPMV_DOTS_DEVICE | (w ? SPMV_W_DEVICE : 0u);
    SPMV_CHECK_ARG(!(flags & SPMV_ASYNC) || (flags & all_dev) == all_dev,
                   "spmv_execute_dot: SPMV_ASYNC needs device x, y, w and dots");
    SPMV_CHECK_ARG(!staged || p->x_stage != nullptr, "SPMV_X_STAGED without a previously staged x");
    SPMV_CHECK_ARG(!timed || iters > 0, "spmv_time_dot: iters < 1");
    SPMV_RETURN_IF(bind_device(p));
    p->y_staged = false;  // like any other non-staged execute (spmv_fetch_y)
    const bool x_host = !staged && !(flags & SPMV_X_DEVICE);
    const bool y_dev = (flags & SPMV_Y_DEVICE) != 0;
    const bool w_host = w != nullptr && !(flags & SPMV_W_DEVICE);
    const bool dots_host = !(flags & SPMV_DOTS_DEVICE);
    // every allocation comes first: out of memory leaves y untouched
    if (x_host) SPMV_RETURN_IF(ensure_stage(p, &p->x_stage, p->n));
    if (!y_dev) SPMV_RETURN_IF(ensure_stage(p, &p->y_stage, p->m));
    if (w_host) SPMV_RETURN_IF(ensure_stage(p, &p->w_stage, p->m));
    SPMV_RETURN_IF(dot_partials(p));
    const double *dx = x_host || staged ? p->x_stage : x;
    double *dy = y_dev ? y : p->y_stage;
    const double *dw = w_host ? p->w_stage : w;
    double *dd = dots_host ? p->dot_part + 2 * dot_slots(p) : dots;
    if (timed) return time_on_stream(p->stream, iters, ms, [&] { return dot_dispatch(p, dx, dy, dw, dd); });
    if (x_host && p->n) SPMV_HIP_TRY(hipMemcpyAsync(p->x_stage, x, sizeof(double) * p->n, hipMemcpyHostToDevice, p->stream));
    if (w_host && p->m) SPMV_HIP_TRY(hipMemcpyAsync(p->w_stage, w, sizeof(double) * p->m, hipMemcpyHostToDevice, p->stream));
    SPMV_RETURN_IF(dot_dispatch(p, dx, dy, dw, dd));
    if (!y_dev && p->m) SPMV_HIP_TRY(hipMemcpyAsync(y, dy, sizeof(double) * p->m, hipMemcpyDeviceToHost, p->stream));
    if (dots_host) {  // 16 bytes, once the stream has drained
        SPMV_HIP_TRY(hipMemcpyAsync(dots, dd, 2 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
        SPMV_HIP_TRY(hipStreamSynchronize(p->stream));
        return SPMV_SUCCESS;
    }
    return finish_execute(p, flags | (staged ? SPMV_X_DEVICE : 0u), !y_dev);
}

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

// ---- conjugate gradients on a plan (vector kernels: k_cg.hip) --

// one plain allocation of the solver's, at the first use
template <typename T>
static int cg_alloc(spmv_plan_s *p, T **buf, size_t bytes) {
    if (*buf) return SPMV_SUCCESS;
    void *q = nullptr;
    SPMV_RETURN_IF(p->arena.alloc_plain(&q, bytes));
    *buf = (T *)q;
    return SPMV_SUCCESS;
}

// Everything a solve allocates, before any device work: r, p, q, the partials
// (two arrays of 2 doubles per workgroup: the init pass fills both), the
// scalar block, the staging of host vectors, and what the plan's own axpby and
// dot executes need.
static int cg_workspace(spmv_plan_s *p, bool host, bool have_dinv) {
    CgWork &w = p->cg;
    const size_t vec = sizeof(double) * (size_t)p->m;
    SPMV_RETURN_IF(cg_alloc(p, &w.r, vec));
    SPMV_RETURN_IF(cg_alloc(p, &w.p, vec));
    SPMV_RETURN_IF(cg_alloc(p, &w.q, vec));
    SPMV_RETURN_IF(cg_alloc(p, &w.part, sizeof(double) * (size_t)(4 * cg_blocks(p->m))));
    SPMV_RETURN_IF(cg_alloc(p, &w.state, sizeof(CgState)));
    if (host) {
        SPMV_RETURN_IF(cg_alloc(p, &w.b_stage, vec));
        SPMV_RETURN_IF(cg_alloc(p, &w.x_stage, vec));
        if (have_dinv) SPMV_RETURN_IF(cg_alloc(p, &w.dinv_stage, vec));
    }
    SPMV_RETURN_IF(axpby_scratch(p, 1.0));
    return dot_partials(p);
}

// the launches of one iteration on p->stream: q = A p and p . q by the plan's
// own dot execute (w = x = p, the dots into the scalar block), then the update,
// the one-workgroup finish and the new direction
static int cg_iteration(spmv_plan_s *p, double *x, const double *dinv) {
    const CgWork &w = p->cg;
    SPMV_RETURN_IF(dot_dispatch(p, w.p, w.q, w.p, w.state->dots));
    SPMV_RETURN_IF(launch_cg_update(p, x, dinv));
    SPMV_RETURN_IF(launch_cg_finish(p));
    return launch_cg_direction(p, dinv);
}

void cg_graph_release(spmv_plan_s *p) {
    CgWork &w = p->cg;
    if (w.exec) (void)hipGraphExecDestroy(w.exec);
    if (w.graph) (void)hipGraphDestroy(w.graph);
    w.exec = nullptr;
    w.graph = nullptr;
}

// The graph of one check interval: `every` iterations, a linear chain,
// captured on a private stream as graph_capture does and instantiated once.
// rtol and max_iters travel through the scalar block, b is read by the init
// pass only: the key is what the captured launches hold, (x, dinv, every).
static int cg_graph(spmv_plan_s *p, double *x, const double *dinv, int32_t every) {
    CgWork &w = p->cg;
    if (w.exec && w.key_x == x && w.key_dinv == dinv && w.key_every == every) return SPMV_SUCCESS;
    cg_graph_release(p);
    hipStream_t cs = nullptr;
    SPMV_HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    const hipStream_t saved = p->stream;
    const int saved_prof = p->prof_k;
    p->stream = cs;
    p->prof_k = -1;
    int st = SPMV_SUCCESS;
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        for (int32_t k = 0; k < every && st == SPMV_SUCCESS; ++k) st = cg_iteration(p, x, dinv);
        e = hipStreamEndCapture(cs, &g);
    }
    p->stream = saved;
    p->prof_k = saved_prof;
    (void)hipStreamDestroy(cs);
    hipGraphExec_t ex = nullptr;
    if (st == SPMV_SUCCESS && e == hipSuccess) e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    if (st != SPMV_SUCCESS || e != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        if (st != SPMV_SUCCESS) return st;
        set_error(std::string("spmv_cg_solve: graph of a check interval: ") + hipGetErrorString(e));
        (void)hipGetLastError();
        return SPMV_ERROR_HIP;
    }
    w.graph = g;
    w.exec = ex;
    w.key_x = x;
    w.key_dinv = dinv;
    w.key_every = every;
    return SPMV_SUCCESS;
}

static int cg_solve(spmv_plan_t p, const double *b, double *x, const double *dinv, double rtol, int32_t max_iters,
                    int32_t check_every, uint32_t flags, spmv_cg_info_t *info) {
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    SPMV_CHECK_ARG(info != nullptr, "spmv_cg_solve: info is NULL");
    SPMV_CHECK_ARG((b != nullptr && x != nullptr) || p->m == 0, "spmv_cg_solve: b or x is NULL");
    SPMV_CHECK_ARG(p->m == p->n, "spmv_cg_solve: the plan is not square");
    SPMV_CHECK_ARG(!(flags & ~(SPMV_CG_DEVICE | SPMV_CG_GRAPH)), "spmv_cg_solve: unknown flag bits");
    SPMV_CHECK_ARG(max_iters >= 0, "spmv_cg_solve: max_iters < 0");
    SPMV_CHECK_ARG(check_every >= 1, "spmv_cg_solve: check_every < 1");
    SPMV_CHECK_ARG(rtol >= 0.0, "spmv_cg_solve: rtol is negative or NaN");
    if ((flags & SPMV_CG_GRAPH) && p->format == SPMV_FORMAT_CSS) {
        // as spmv_graph_create: the sweep's per-launch sequence number is a kernel argument
        set_error("spmv_cg_solve: CSS plans cannot be replayed from a graph (SPMV_CG_GRAPH)");
        return SPMV_ERROR_NOT_SUPPORTED;
    }
    p->y_staged = false;  // like any other non-staged execute (spmv_fetch_y)
    CgState h = {};
    if (p->m > 0) {
        SPMV_RETURN_IF(bind_device(p));
        const bool host = !(flags & SPMV_CG_DEVICE);
        if (!host) {
            const void *ptrs[3] = {b, x, dinv};
            SPMV_RETURN_IF(check_device_arrays(ptrs, dinv ? 3 : 2, p->device, "spmv_cg_solve",
                                               ": SPMV_CG_DEVICE needs device memory on the plan's device"));
        }
        // every allocation comes first: out of memory leaves x untouched
        SPMV_RETURN_IF(cg_workspace(p, host, dinv != nullptr));
        CgWork &w = p->cg;
        const size_t vec = sizeof(double) * (size_t)p->m;
        double *dx = x;
        const double *db = b, *dd = dinv;
        if (host) {
            SPMV_HIP_TRY(hipMemcpyAsync(w.b_stage, b, vec, hipMemcpyHostToDevice, p->stream));
            SPMV_HIP_TRY(hipMemcpyAsync(w.x_stage, x, vec, hipMemcpyHostToDevice, p->stream));
            if (dinv) SPMV_HIP_TRY(hipMemcpyAsync(w.dinv_stage, dinv, vec, hipMemcpyHostToDevice, p->stream));
            db = w.b_stage;
            dx = w.x_stage;
            dd = dinv ? w.dinv_stage : nullptr;
        }
        if (flags & SPMV_CG_GRAPH) SPMV_RETURN_IF(cg_graph(p, dx, dd, check_every));
        // r = b - A x through the plan's own axpby, then z, p and the first scalars
        SPMV_HIP_TRY(hipMemcpyAsync(w.r, db, vec, hipMemcpyDeviceToDevice, p->stream));
        SPMV_RETURN_IF(axpby_dispatch(p, Axpby{-1.0, 1.0}, dx, w.r));
        SPMV_RETURN_IF(launch_cg_init(p, db, dd, rtol * rtol, max_iters));
        for (;;) {  // max_iters is enforced on the device: the loop ends on done
            SPMV_HIP_TRY(hipMemcpyAsync(&h, w.state, sizeof(h), hipMemcpyDeviceToHost, p->stream));
            SPMV_HIP_TRY(hipStreamSynchronize(p->stream));
            if (h.done) break;
            // the last interval is cut at max_iters (launches past it would only
            // run the SpMV for nothing): plain launches, the graph holds check_every
            const int32_t left = std::max<int32_t>(1, max_iters - h.iterations);
            if ((flags & SPMV_CG_GRAPH) && left >= check_every) {
                SPMV_HIP_TRY(hipGraphLaunch(w.exec, p->stream));
            } else {
                for (int32_t k = 0; k < std::min(check_every, left); ++k) SPMV_RETURN_IF(cg_iteration(p, dx, dd));
            }
        }
        if (host) {
            SPMV_HIP_TRY(hipMemcpyAsync(x, w.x_stage, vec, hipMemcpyDeviceToHost, p->stream));
            SPMV_HIP_TRY(hipStreamSynchronize(p->stream));
        }
    }
    info->status = h.status;  // m = 0: CONVERGED, nothing ran
    info->iterations = h.iterations;
    info->rr = h.rr;
    info->bb = h.bb;
    info->rz = h.rz;
    info->pq = h.pq;
    return SPMV_SUCCESS;
}

// ---- multi-vector execute (Y = A X, k interleaved right-hand sides) ---------

// Widths with a fused kernel (k_dia.hip, k_ell.hip), per format, widest first.
// Every width that beat K single-vector executes on the same plan is listed
// (DESIGN §3.7); a width that is not listed is cut narrower.
static const int kMultiWidthsDia[] = {8, 4, 2};
static const int kMultiWidthsEll[] = {8, 4, 2};

static bool multi_format_fused(const spmv_plan_s *p) {
    // JDS: overflow rows take the generic path, as HYB does
    return p->format == SPMV_FORMAT_DIA || p->format == SPMV_FORMAT_ELL || jds_without_overflow(p);
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
    void *q = nullptr;
    SPMV_RETURN_IF(p->arena.alloc_plain(&q, sizeof(double) * (size_t)std::max<int64_t>(p->n + p->m, 1)));
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
    SPMV_RETURN_IF(plan_alloc(p, buf, need));
    *cap = need;
    return SPMV_SUCCESS;
}

}  // namespace spmv

using namespace spmv;

extern "C" {

struct spmv_graph_s {
    spmv_plan_t plan = nullptr;  // launches use the plan's stream; destroy does not touch it
    int device = 0;              // the plan's device, for destroy
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    int32_t reps = 0;
};

int spmv_set_stream(spmv_plan_t p, void *stream) {
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    p->stream = (hipStream_t)stream;
    return SPMV_SUCCESS;
}

int spmv_execute(spmv_plan_t p, const double *x, double *y, uint32_t flags) {
    return execute_impl(p, Axpby{1.0, 0.0}, x, y, flags, false);
}

int spmv_execute_alpha(spmv_plan_t p, double alpha, const double *x, double *y, uint32_t flags) {
    return execute_impl(p, Axpby{alpha, 0.0}, x, y, flags, false);
}

int spmv_execute_axpby(spmv_plan_t p, double alpha, const double *x, double beta, double *y, uint32_t flags) {
    return execute_impl(p, Axpby{alpha, beta}, x, y, flags, true);
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

int spmv_time_axpby(spmv_plan_t p, double alpha, const double *x_dev, double beta, double *y_dev, int32_t iters,
                    double *ms) {
    SPMV_CHECK_ARG(p != nullptr && ms != nullptr && iters > 0, "bad arguments");
    SPMV_CHECK_ARG((x_dev != nullptr || p->n == 0) && (y_dev != nullptr || p->m == 0), "x or y is NULL");
    SPMV_RETURN_IF(bind_device(p));
    p->y_staged = false;
    SPMV_RETURN_IF(axpby_scratch(p, beta));
    const Axpby ab{alpha, beta};
    return time_on_stream(p->stream, iters, ms, [&] { return axpby_dispatch(p, ab, x_dev, y_dev); });
}

int spmv_axpby_path(spmv_plan_t p, int32_t *fused) {
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    SPMV_CHECK_ARG(fused != nullptr, "fused out-pointer is NULL");
    *fused = axpby_fused(p) ? 1 : 0;
    return SPMV_SUCCESS;
}

int spmv_execute_dot(spmv_plan_t p, const double *x, double *y, const double *w, double *dots, uint32_t flags) {
    return dot_impl(p, x, y, w, dots, flags, 0, nullptr);
}

int spmv_time_dot(spmv_plan_t p, const double *x_dev, double *y_dev, const double *w_dev, double *dots_dev,
                  int32_t iters, double *ms) {
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    SPMV_CHECK_ARG(ms != nullptr, "spmv_time_dot: ms is NULL");
    return dot_impl(p, x_dev, y_dev, w_dev, dots_dev,
                    SPMV_X_DEVICE | SPMV_Y_DEVICE | SPMV_W_DEVICE | SPMV_DOTS_DEVICE, iters, ms);
}

int spmv_dot_path(spmv_plan_t p, int32_t *fused) {
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    SPMV_CHECK_ARG(fused != nullptr, "fused out-pointer is NULL");
    *fused = dot_fused(p) ? 1 : 0;
    return SPMV_SUCCESS;
}

int spmv_cg_solve(spmv_plan_t p, const double *b, double *x, const double *dinv, double rtol, int32_t max_iters,
                  int32_t check_every, uint32_t flags, spmv_cg_info_t *info) {
    return cg_solve(p, b, x, dinv, rtol, max_iters, check_every, flags, info);
}

int spmv_cg_path(spmv_plan_t p, int32_t *launches_per_iteration) {
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    SPMV_CHECK_ARG(launches_per_iteration != nullptr, "launches out-pointer is NULL");
    // the plan's dot execute (fused: its kernel and the dot finish; generic: its
    // kernels, the pass over q and the dot finish), then update, finish, direction
    *launches_per_iteration = (dot_fused(p) ? 2 : p->n_kernels + 2) + 3;
    return SPMV_SUCCESS;
}

int spmv_execute_multi(spmv_plan_t p, int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy,
                       uint32_t flags) {
    SPMV_RETURN_IF(multi_check_args(k, X, ldx, Y, ldy, flags));
    SPMV_CHECK_ARG(p != nullptr, "plan is NULL");
    SPMV_CHECK_ARG((X != nullptr || p->n == 0) && (Y != nullptr || p->m == 0), "multi execute: X or Y is NULL");
    SPMV_RETURN_IF(bind_device(p));
    p->y_staged = false;  // like any other non-staged execute (spmv_fetch_y)
    const int64_t kp = (k + 1) & ~1;  // staging pitch: host callers always qualify for the fused path
    const bool y_host = !(flags & SPMV_Y_DEVICE);
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
    if (y_host) {
        SPMV_RETURN_IF(multi_stage(p, &p->my_stage, &p->my_cap, p->m * kp));
        dY = p->my_stage;
        dldy = kp;
    }
    SPMV_RETURN_IF(multi_dispatch(p, k, dX, dldx, dY, dldy));
    if (y_host && p->m)
        SPMV_HIP_TRY(hipMemcpy2DAsync(Y, sizeof(double) * ldy, dY, sizeof(double) * kp, sizeof(double) * k,
                                      (size_t)p->m, hipMemcpyDeviceToHost, p->stream));
    return finish_execute(p, flags, y_host);
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

}  // extern "C"
