/*
 * spmv_hip.h -- C-ABI of the MI355X-native fp64 SpMV engine (libspmv_hip.so).
 *
 * This is the drop-in boundary for the reference's `opt_*` format-dispatch
 * surface (hir0shim/singleSpMV).  Plain C types only: pointers, sizes, int
 * status codes.  No exit(), no torch types, no C++ in the signatures.
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * reference repository):
 *
 *   spmv_plan_create_coo   OptimizeProblem(const SpMat&, const Vec&, SpMatOpt&,
 *                          VecOpt&) of every plugin, e.g. src/opt_crs.h:15,
 *                          src/opt_ell.h:16, src/opt_ss.h:35, src/opt_dia.h:16,
 *                          src/opt_cusparse.h:33; SpMat is src/util.h:7-19.
 *   spmv_plan_create_csr*  opt_crs SpMatOpt {ptr, idx, val} (src/opt_crs.h:3-9)
 *                          and the device CSR of src/opt_cusparse.cpp:36-42.
 *   spmv_execute           extern "C" SpMV(const SpMatOpt&, const VecOpt&,
 *                          Vec&) (e.g. src/opt_crs.h:16-18); with host x / host
 *                          y it reproduces src/opt_cusparse.cpp:72-82 (H2D x,
 *                          y = 1*A*x + 0*y, D2H y).
 *   spmv_plan_destroy      (the reference never frees; no counterpart)
 *   spmv_load_mtx          LoadSparseMatrix (src/util.cpp:30-66), parallel
 *   spmv_load_mtx_csr      the CSR5 benchmark's banner-aware loader
 *                          (CSR5_cuda/main.cu:157-306): pattern/integer,
 *                          symmetric expansion, straight to CSR
 *   spmv_{save,load}_csr_bin (new) binary CSR cache
 *   spmv_rand_vector       srand + CreateRandomVector (src/main.cpp:18,
 *                          src/util.cpp:92-102)
 *   spmv_verify_coo        VerifyResult (src/util.cpp:67-83)
 *   spmv_gen_*             (new) seeded synthetic matrices for the BASELINE
 *                          configs, generated in memory instead of .mtx text
 *   spmv_partition_rows    (new) nnz-balanced row ranges for multi-GPU
 *
 * Semantics shared by every format (β = 0): spmv_execute overwrites every
 * entry of y (src/opt_crs.cpp:68; src/opt_ell.cpp:78; src/opt_dia.cpp:82) and
 * is idempotent -- repeated calls give identical y (the two-call verification
 * of src/main.cpp:41-55).  Host input arrays are borrowed read-only during
 * plan creation and never mutated (unlike the CSR5 handle, which transposes
 * the caller's arrays in place, CSR5_cuda/anonymouslib_cuda.h:203-204).  A
 * plan's sparsity pattern is frozen at creation; its values are not:
 * spmv_plan_update_values rewrites them in place (below, "value refresh").
 *
 * Non-finite and subnormal values: every product and every sum is an IEEE
 * binary64 operation, round to nearest, with gradual underflow -- nothing is
 * flushed to zero, the LDS (ds_add_f64) and global (global_atomic_add_f64)
 * atomic adds of BIN, CSS and COO included -- and stored zeros are multiplied
 * like any other entry (0 * Inf = NaN).  A non-finite x[c] therefore makes
 * non-finite exactly the rows that reference column c in CSR (every kernel),
 * SS, COO, CSS and BIN, with the class (NaN, +Inf, -Inf) the sequential sum
 * gives; every other row is bit for bit what it is for a finite x[c]: masked
 * lanes, tile and unit padding and dummy slots are dropped by selects, never
 * by a zero weight.  The padded layouts multiply 0 by a few more x entries:
 * ELL, JDS and HYB pad a row with its last real column (their 0 * x[c] turns
 * the row's +-Inf into NaN) and an empty row with column 0 (NaN instead of 0
 * where x[0] is not finite and the row's slice has any width); DIA reads x[clamp(r + off, 0, n - 1)] for every
 * stored diagonal off of row r.  This is the caveat noted at
 * spmv_options_t.crs_exact, stated here once for every layout.  Finite terms
 * whose partial sum overflows give a result that depends on the add order,
 * hence on the format.  (tests/test_gpu_special.py.)
 *
 * Threading: thread-compatible.  One plan per thread; a plan may be used from
 * any thread but not concurrently.
 */
#ifndef SPMV_HIP_H
#define SPMV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version 2 changed the layout of spmv_options_t (the bin_* / placement
 * fields, round 2) and spmv_plan_info_t: a caller built against a version-1
 * header passes structs of the wrong size and must be rebuilt.  Version 3
 * (round 3) took bin_product_order from spmv_options_t's reserved words (same
 * size) and appended bin_sum_entries to spmv_plan_info_t.  crs_exact and build
 * (round 5) took the last reserved words: same size, and 0
 * (spmv_options_default) keeps the version-3 results (build = AUTO moves only
 * where the layout is made, not what it is).  The multi-vector entry points
 * (spmv_execute_multi, spmv_time_multi, spmv_multi_path) are new functions
 * and change no struct: the version stays 3.  So do the value-refresh entry
 * points (spmv_plan_update_prepare, spmv_plan_update_values) and the BLAS form
 * (spmv_execute_axpby, spmv_time_axpby, spmv_axpby_path) and the execute
 * with dot products (spmv_execute_dot, spmv_time_dot, spmv_dot_path, with the
 * flags SPMV_W_DEVICE and SPMV_DOTS_DEVICE) and the solver (spmv_cg_solve,
 * spmv_cg_path, the flags SPMV_CG_DEVICE and SPMV_CG_GRAPH).  Callers may
 * check spmv_api_version() == SPMV_HIP_API_VERSION once at startup; the
 * structs are only ever filled by spmv_options_default / spmv_plan_info of a
 * library with the same version. */
#define SPMV_HIP_API_VERSION 3
int spmv_api_version(void);

/* ---- status codes -------------------------------------------------------- */
typedef enum spmv_status {
    SPMV_SUCCESS = 0,
    SPMV_ERROR_INVALID_VALUE = 1,  /* bad argument / inconsistent arrays    */
    SPMV_ERROR_NOT_SUPPORTED = 2,  /* format cannot hold this matrix        */
    SPMV_ERROR_OUT_OF_MEMORY = 3,  /* host or device allocation failed      */
    SPMV_ERROR_HIP = 4,            /* a HIP runtime call failed             */
    SPMV_ERROR_IO = 5,             /* file missing / unparsable             */
    SPMV_ERROR_NO_DEVICE = 6       /* no usable gfx950 device               */
} spmv_status_t;

/* ---- storage formats (the reference's -DOPT_<FMT> plugins) --------------- */
typedef enum spmv_format {
    SPMV_FORMAT_AUTO = 0, /* chosen from the row-length histogram             */
    SPMV_FORMAT_CSR = 1,  /* opt_crs   (src/opt_crs.cpp)                        */
    SPMV_FORMAT_ELL = 2,  /* opt_ell   (src/opt_ell.cpp), device: sliced ELL    */
    SPMV_FORMAT_SS = 3,   /* opt_ss / CSR5: segmented sum over 64 x sigma tiles */
    SPMV_FORMAT_DIA = 4,  /* opt_dia   (src/opt_dia.cpp), device: row-indexed   */
    SPMV_FORMAT_HYB = 5,  /* ELL(K) + CSR overflow (BASELINE config 3)          */
    SPMV_FORMAT_CSS = 6,  /* opt_css lineage: column-slab sweep, y in LDS, x    */
                          /* slab L2-resident per XCD (large random matrices)  */
    SPMV_FORMAT_COO = 7,  /* opt_coo   (src/opt_coo.cpp): f64 atomics per row segment */
    SPMV_FORMAT_JDS = 8,  /* opt_jds   (src/opt_jds.cpp): rows sorted by length,  */
                          /* jagged 64-row slices, y permuted back             */
    SPMV_FORMAT_BIN = 9   /* opt_ss Mul/Sum x opt_css column blocks: Mul with   */
                          /* the x strip in LDS, products binned by row block,  */
                          /* Sum per bin with y in LDS (large random matrices)  */
} spmv_format_t;

typedef struct spmv_plan_s *spmv_plan_t;

typedef struct spmv_options {
    int32_t format;     /* spmv_format_t                                      */
    int32_t device;     /* HIP device ordinal; -1 = the calling thread's current */
    int32_t csr_lanes;  /* CSR: lanes per row 1..64 (power of two), 0 = auto   */
    int32_t ell_width;  /* HYB: ELL width K, 0 = auto (row-length histogram)   */
    int32_t ss_sigma;   /* SS: nnz per lane per tile, 0 = auto                 */
    int32_t dia_max_diags; /* DIA: refuse beyond this many diagonals (0 = 1024) */
    double dia_max_fill;   /* DIA: refuse when stored/nnz exceeds this (0 = 3) */
    int32_t css_slab_shift; /* CSS: slab = 2^shift columns (0 = 18, 2 MiB of x) */
    int32_t css_lag;        /* CSS: pacing slack in slabs (0 = 4, -1 = no pacing) */
    int32_t css_pace;       /* CSS: 0/1 pace against every XCD, 2 own XCD only */
    int32_t bin_strip_cols;  /* BIN: x strip width, 64..20480 columns (0 = 20480) */
    int32_t bin_groups;      /* BIN: row groups sharing one product buffer (0 = 1) */
    int32_t bin_sum_waves;   /* BIN: Sum waves per workgroup 2 | 4 | 8 (0 = auto) */
    int32_t bin_pad;         /* BIN: segment padding 8 | 16 | 32 entries (0 = auto) */
    int32_t csr_row_ptr64;   /* CSR: 1 = 64-bit row pointers below 2^31 nnz too */
    int32_t placement;       /* BIN product buffer / DIA values, see SPMV_PLACEMENT_* */
    int32_t bin_long_len;    /* BIN: rows with >= this many entries are reduced per
                                strip run in the Mul (partial sums, <= 1e-12 from
                                the sequential sum); 0 = auto (max(128, strips)
                                when such rows hold >= 5 % of nnz), -1 = never
                                (every row bit-exact)                         */
    int32_t bin_product_order; /* BIN: where the Mul writes its products
                                (SPMV_BIN_ORDER_*; 0 = auto)                   */
    int32_t crs_exact;       /* CSR requests: 1 = opt_crs semantics -- every row
                                the sequential column-order sum bit for bit
                                (src/opt_crs.cpp:57-69) on the fastest layout
                                that sums so for this matrix: DIA (AUTO's banded
                                rule, rows strictly ascending: no duplicates),
                                BIN with no run path (AUTO's wide-x rule, rows
                                strictly ascending: strip order = CSR order),
                                ELL (near-uniform rows, none > 64), else CSR with
                                one lane per row; spmv_plan_info reports the
                                layout.  Bit for bit for finite x: DIA and ELL
                                padding adds 0 * x[c], which is NaN where x[c]
                                is Inf or NaN (opt_crs skips no entry but has
                                no padding).  0 = the CSR kernels as configured
                                (row groups of L lanes: butterfly sums)       */
    int32_t build;           /* plan builders (SPMV_BUILD_*): AUTO = a host CSR of
                                >= 2^24 entries is staged into HBM and built by
                                the device builders (every format;
                                byte-identical layouts, spmv_plan_digest), when
                                the staging copy fits in device memory
                                (else the host builders, with the format
                                resolved there); smaller ones take the host
                                builders */
} spmv_options_t;

/* Where spmv_plan_create_csr / _csr32 / _coo build the layout. */
typedef enum spmv_build {
    SPMV_BUILD_AUTO = 0,
    SPMV_BUILD_HOST = 1,    /* host builders (formats.cpp, build_bin.cpp)       */
    SPMV_BUILD_DEVICE = 2   /* stage the CSR into HBM and build there whatever
                               the size (same exceptions as AUTO)              */
} spmv_build_t;

/* Placement of the large buffers of a plan (the BIN product buffer, the DIA
 * values, the streamed col / val arrays of CSR, ELL, HYB, JDS, SS, COO, CSS).  The BIN Mul ran ~15 % slower with one
 * plain hipMalloc on most plans than with the same buffer built from 2-MB
 * physical handles (profiles/round1/README.md §4a "Placement, round 3").
 *
 * Known limitation: placement is not fully under the library's control.
 * Measured residual spread of AUTO over 8 same-size plans kept alive in one
 * process (profiles/round5/placement/): config-4 DIA 1.472-1.562 ms (6.1 %,
 * every later plan within 1 % of the first or faster), config-2 BIN
 * 0.797-0.897 ms (12.6 %, worst 7.6 % above the first).  SEARCH narrowed
 * that to 1.2 % (DIA 1.478-1.495) and 4.2 % (BIN 0.801-0.835) at 0.6-7.3 s
 * of build per plan and transient candidate buffers over the free HBM, so it
 * stays an explicit opt-in; a caller who needs the best time builds its hot
 * plan first or with SEARCH (spmv_plan_info reports the mode, the candidates
 * and their best / worst launch). */
#define SPMV_PLACEMENT_AUTO 0   /* BIN products >= 32 MB, DIA values >= 256 MB and
                                   the streamed arrays (col / val / slots) of the
                                   other formats >= 256 MB: VMM; the rest PLAIN  */
#define SPMV_PLACEMENT_PLAIN 1  /* one hipMalloc                                     */
#define SPMV_PLACEMENT_SEARCH 2 /* BIN product buffer (>= 32 MB) / DIA values
                                   (>= 256 MB): up to 8 plain candidates spread
                                   over all free HBM, each timed with one launch
                                   over a zero x, the fastest kept (build-time
                                   cost and transient memory: see above); other
                                   formats: as AUTO                               */
#define SPMV_PLACEMENT_VMM 3    /* hipMemCreate handles of 2 MB mapped back to back
                                   into one VA range aligned to 1 GB (no transient
                                   device memory)                                 */

/* Product order of a BIN plan (spmv_options_t.bin_product_order).  Either
 * way each row is summed in column order (bit-identical y). */
#define SPMV_BIN_ORDER_AUTO 0  /* MUL for short segments (< 112 entries per
                                  row bin x column strip: the wide multi-GPU
                                  rank shapes) where the layout allows it (no
                                  long rows, one row group, < 2^31 entries),
                                  else SUM                                    */
#define SPMV_BIN_ORDER_SUM 1   /* the Mul scatters each product into its (bin,
                                  strip) segment of the Sum's order; the Sum
                                  streams each bin as one contiguous run       */
#define SPMV_BIN_ORDER_MUL 2   /* the Mul writes its products contiguously in
                                  its own order (no segment padding, no
                                  destination array); the Sum gathers each
                                  bin's segments in 8-entry chunks through a
                                  chunk table                                  */

/* Fill `opt` with defaults (AUTO format, current device, auto tuning). */
void spmv_options_default(spmv_options_t *opt);

/* Plan builds are untimed setup (OptimizeProblem, src/main.cpp:36).  They
 * allocate the plan's device arrays and nothing else.
 *
 * Plan from a host sorted COO (the reference SpMat, src/util.h:7-19).
 * Rows must be sorted ascending (LoadSparseMatrix guarantees it); columns
 * within a row may be in any order, duplicates are summed. */
int spmv_plan_create_coo(int32_t m, int32_t n, int32_t nnz, const int32_t *row_idx,
                         const int32_t *col_idx, const double *val,
                         const spmv_options_t *opt, spmv_plan_t *plan);

/* Plan from a host CSR with 64-bit row pointers (nnz may exceed 2^31). */
int spmv_plan_create_csr(int64_t m, int64_t n, int64_t nnz, const int64_t *row_ptr,
                         const int32_t *col_idx, const double *val,
                         const spmv_options_t *opt, spmv_plan_t *plan);

/* Plan from a host CSR with 32-bit row pointers (opt_crs SpMatOpt layout). */
int spmv_plan_create_csr32(int32_t m, int32_t n, int32_t nnz, const int32_t *row_ptr,
                           const int32_t *col_idx, const double *val,
                           const spmv_options_t *opt, spmv_plan_t *plan);

/* Plan from a CSR that already lives in device memory (64-bit row pointers;
 * all three arrays on the plan's device, only read).  Every format is built
 * on the device (the CSR5 conversion pipeline's role,
 * CSR5_cuda/detail/cuda/format_cuda.h:21-718): only the row pointers (and,
 * for BIN, the (bin, strip) counts and the long rows' run descriptors) visit
 * the host, for the layout decisions that depend on row lengths alone; AUTO
 * is resolved there too, its diagonal census run on the device; CSS's
 * per-wave column sorts are one stable radix sort.  The layouts are
 * byte-identical to the host builders' (spmv_plan_digest); BIN sorts rows
 * whose columns are not ascending by 20480-column strip on the device first
 * (when the device has no room for that copy, the CSR is copied to the host
 * and the host builder runs).  The input is validated on the device like
 * spmv_plan_create_csr's host check. */
int spmv_plan_create_csr_device(int64_t m, int64_t n, int64_t nnz, const int64_t *d_row_ptr,
                                const int32_t *d_col_idx, const double *d_val,
                                const spmv_options_t *opt, spmv_plan_t *plan);

/* The same from 32-bit device row pointers (the CSR5 handle's inputCSR,
 * CSR5_cuda/anonymouslib_cuda.h:60-73, takes int arrays on the device). */
int spmv_plan_create_csr32_device(int32_t m, int32_t n, int32_t nnz, const int32_t *d_row_ptr,
                                  const int32_t *d_col_idx, const double *d_val,
                                  const spmv_options_t *opt, spmv_plan_t *plan);

/* ---- the transpose: y = A^T x ----------------------------------------------
 * Every format here is a row layout with one writer per row, so A^T is not
 * scattered out of a plan of A (f64 atomics, COO speed, no sequential sums):
 * it gets a plan of its own, built from a CSR of A^T.  The two functions
 * below make that CSR; the three after them build the plan from A directly.
 *
 * The transposition.  Input: a CSR of A, (m, n, nnz, row_ptr int64 [m + 1],
 * col_idx int32 [nnz], val f64 [nnz]); columns inside a row may be unsorted
 * and may repeat (whatever spmv_plan_create_csr accepts).  Output: the CSR of
 * A^T -- t_row_ptr int64 [n + 1], t_col_idx int32 [nnz] (the source row of
 * each entry), t_val f64 [nnz] -- and perm int64 [nnz], the source entry
 * index of each output entry.  Output row c holds A's entries of column c in
 * ascending source entry index (a stable sort of the entries by column), so
 * every output row is in ascending column order whatever order A's rows were
 * in, duplicates stay adjacent in source order, and transposing twice returns
 * a column-sorted CSR unchanged.  Values move as bits (NaN payloads, -0.0,
 * subnormals, Inf); nothing is added or merged.  val and t_val may both be
 * NULL (the pattern alone); perm may be NULL.  Outputs must not overlap the
 * inputs.  The host and the device function give the same bytes.
 *
 * Refusals, in this order, all SPMV_ERROR_INVALID_VALUE with the outputs
 * untouched: val without t_val or the reverse; a NULL t_row_ptr, or a NULL
 * t_col_idx with nnz > 0; then spmv_plan_create_csr's input check (negative
 * or >= 2^31 - 1 dimensions, NULL row_ptr / col_idx, row_ptr[0] != 0,
 * row_ptr[m] != nnz, decreasing row_ptr, a column outside [0, n)); the device
 * function checks that every array is device memory on `device`, then runs
 * the same input check there -- before any kernel indexes by a column.
 *
 * The device function serves nnz < 2^31 - 1 (32-bit entry ids) and returns
 * SPMV_ERROR_NOT_SUPPORTED beyond; the host function has no such limit.  It
 * runs on the null stream and has synchronised on return.  Transient device
 * memory: 16 bytes per entry (sort keys and ids, double-buffered) and the
 * radix sort's workspace, freed before it returns; SPMV_ERROR_OUT_OF_MEMORY
 * leaves the outputs unspecified and leaks nothing. */
int spmv_csr_transpose(int64_t m, int64_t n, int64_t nnz, const int64_t *row_ptr,
                       const int32_t *col_idx, const double *val, int64_t *t_row_ptr,
                       int32_t *t_col_idx, double *t_val, int64_t *perm);
/* the same on `device` (-1: the current one), all arrays device memory there */
int spmv_csr_transpose_device(int32_t device, int64_t m, int64_t n, int64_t nnz,
                              const int64_t *d_row_ptr, const int32_t *d_col_idx,
                              const double *d_val, int64_t *d_t_row_ptr,
                              int32_t *d_t_col_idx, double *d_t_val, int64_t *d_perm);

/* Plans of the transpose.  (m, n) is A's shape; the result is an ordinary plan
 * of A^T: spmv_plan_info reports m = n_A and n = m_A, x holds m_A doubles and
 * y holds n_A, and every array has the digest (spmv_plan_digest) of the plan
 * spmv_plan_create_csr / _csr_device builds from spmv_csr_transpose's output
 * with the same options.  execute, execute_alpha, execute_axpby,
 * execute_multi, graphs, profile and digest treat it as any other plan.  It
 * keeps neither A nor the permutation: device_bytes is its companion's.
 *
 * Host arrays follow opt->build as spmv_plan_create_csr does: the host
 * transposition and the host builders (SPMV_BUILD_HOST, AUTO below 2^24
 * entries), or the staging copy, the device transposition and the device
 * builders; the device route falls back to the host route when the staging
 * copy or the transposition's scratch does not fit, for what the device
 * builders do not make, and from 2^31 - 1 entries on.  All routes give the
 * same digests.  Device arrays: validated, transposed into scratch, built by
 * the device builders, the scratch freed; transient memory is the CSR of A^T
 * (12 bytes per entry + 8 (n + 1)) on top of the transposition's own, then of
 * the builders'.  SPMV_ERROR_OUT_OF_MEMORY there is final (no host
 * transposition from this entry point), as is SPMV_ERROR_NOT_SUPPORTED from
 * 2^31 - 1 entries on.
 *
 * Value refresh: "the CSR the plan was created from" is A's.
 * spmv_plan_update_prepare takes A's row_ptr (m_A + 1) and col_idx,
 * spmv_plan_update_values takes values in A's entry order.
 *
 * Not covered: an op argument on spmv_execute* (A^T out of a plan of A), a
 * plan that holds A and A^T together, a transposed spmv_plan_create_coo,
 * spmv_dist_*, the drop-in (opt_hip.h) and the CSR5 handle. */
int spmv_plan_create_csr_transposed(int64_t m, int64_t n, int64_t nnz, const int64_t *row_ptr,
                                    const int32_t *col_idx, const double *val,
                                    const spmv_options_t *opt, spmv_plan_t *plan);
int spmv_plan_create_csr_device_transposed(int64_t m, int64_t n, int64_t nnz,
                                           const int64_t *d_row_ptr, const int32_t *d_col_idx,
                                           const double *d_val, const spmv_options_t *opt,
                                           spmv_plan_t *plan);
/* *transposed = 1 for a plan made by one of the two functions above, else 0 */
int spmv_plan_is_transposed(spmv_plan_t plan, int32_t *transposed);

int spmv_plan_destroy(spmv_plan_t plan);

/* ---- per-phase profile (replaces the g_profile / PROF_BEGIN instrumentation
 * of src/util.cpp:16-18, src/util.h:59-65 and the Mul/Sum split printed by
 * src/main.cpp:172-175).  Runs `iters` synchronised calls on device x/y and
 * returns the mean ms of each phase of the plan's launch sequence:
 *   CSR "csr" | ELL "ell" | JDS, HYB "ell","overflow" | SS "tile","fixup" |
 *   DIA "dia" | CSS "sweep" | COO "zero_y","segment" | BIN "mul","sum"
 * JDS and HYB report the "overflow" phase even when no row overflows (then
 * it times no launch).  BIN has two phases whatever bin_groups is: the row
 * groups' Mul launches are one phase, their one Sum launch the other (only
 * the probe build's per-group product buffer, an experiment switch the
 * product library ignores, numbers a "mul.g","sum.g" pair per group).
 * spmv_phase_name(plan, k) names phase k, "" for k outside [0, n_phases). */
int spmv_profile(spmv_plan_t plan, const double *x_dev, double *y_dev, int32_t iters,
                 double *phase_ms, int32_t max_phases, int32_t *n_phases);
const char *spmv_phase_name(spmv_plan_t plan, int32_t k);

/* Measured STREAM-read ceiling of `device` (GB/s): nontemporal 16-byte reads
 * of a `bytes` buffer (use >> 256 MB), `iters` launches timed with events. */
int spmv_stream_probe(int32_t device, int64_t bytes, int32_t iters, double *read_gbs);

/* Measured STREAM-write ceiling of `device` (GB/s): nontemporal 16-byte
 * stores over a `bytes` buffer, `iters` launches timed with events. */
int spmv_stream_write_probe(int32_t device, int64_t bytes, int32_t iters, double *write_gbs);

/* Measured mixed read + write ceiling of `device` (GB/s of reads + writes): a
 * grid-stride stream reading `bytes` (16-byte loads) and writing
 * write_quarters/4 of them back (nontemporal 16-byte stores), the fastest of
 * `iters` launches; BIN's Mul moves about 3 quarters. */
int spmv_mixed_probe(int32_t device, int64_t bytes, int32_t write_quarters, int32_t iters, double *gbs);

/* Measured ceiling of random 8-byte gathers (gathers/s): n streamed int32
 * indices into a `table_bytes` table (1 MB: L2-resident, the best case of a
 * gather-bound SpMV), 8 gathers in flight per lane, best of 5 launches. */
int spmv_gather_probe(int32_t device, int64_t n, int64_t table_bytes, double *g_per_s);

/* Exactness guard of the BIN and CSS formats: `rounds` wave-wide atomic adds
 * of f64 into 64 LDS slots (one ds_add_f64 instruction each; lane l of round
 * r adds val[r*64+l] to slot[r*64+l]); out[64] = the slots afterwards.  BIN
 * and CSS are bit-identical to the sequential opt_crs sum only if lanes of
 * one instruction that hit the same slot are applied in lane order. */
int spmv_lds_order_probe(int32_t device, int32_t rounds, const int32_t *slot, const double *val,
                         double *out);

/* ---- execution ----------------------------------------------------------- */
#define SPMV_X_DEVICE 0x1u /* x is a device pointer (else host: H2D per call) */
#define SPMV_Y_DEVICE 0x2u /* y is a device pointer (else host: D2H per call).
                              COO plans add into y with device f64 atomics
                              (-munsafe-fp-atomics): a device y must be
                              ordinary (coarse-grained) device memory, as
                              hipMalloc returns -- not fine-grained or host-
                              mapped memory, where those atomics are not
                              performed atomically                            */
#define SPMV_ASYNC 0x4u    /* device x and y: return without synchronising    */
#define SPMV_X_STAGED 0x8u /* re-use the host x uploaded by the previous call
                              (x may be NULL); error if none was staged       */
#define SPMV_Y_STAGED 0x10u /* leave y in the plan's device staging buffer (y
                              may be NULL; no D2H copy): spmv_fetch_y copies it
                              to the host when the caller reads it -- the
                              per-call 8m-byte download of opt_cusparse
                              (src/opt_cusparse.cpp:82) leaves the timed loop */

/* Buffer contract of device x and y (tests/test_gpu_routes.py pins it on
 * guarded buffers for every format): x and y need the 8-byte alignment of a
 * double, no more -- a view one double into a 16-byte-aligned allocation is
 * as good as its base, and gives the same y bit for bit (DIA stores row pairs
 * as 16 bytes only where y is 16-byte aligned, BIN stages x by LDS-DMA only
 * where x is).  Nothing outside [x, x + n) influences y (padded slots
 * multiply 0 by an entry inside the range), and nothing outside [y, y + m)
 * is written.  This holds for spmv_execute, spmv_execute_alpha, spmv_time,
 * spmv_profile, spmv_graph_* and the k = 1, ldx = ldy = 1 case of
 * spmv_execute_multi, which runs the plan's kernels in place on X and Y.
 * n may be anything below 2^31 - 1: an x of 4 GiB and more (n >= 2^29) takes
 * 64-bit offsets in every format (tests/test_gpu_wide_x.py).  m may be
 * anything below 2^31 - 1 as well: a y of 4 GiB and more (m >= 2^29; for k
 * right-hand sides m * ldy >= 2^29) and per-row arrays beyond 4 GiB are
 * addressed in 64 bits in every format, and every execute writes all m
 * entries of y (tests/test_gpu_tall_y.py). */

/* y = A * x.  x holds n doubles, y holds m doubles. */
int spmv_execute(spmv_plan_t plan, const double *x, double *y, uint32_t flags);

/* Copy the y of the latest execute to host memory (m doubles); that execute
 * must have been SPMV_Y_STAGED (any other execute since then makes this
 * SPMV_ERROR_INVALID_VALUE instead of returning an older y). */
int spmv_fetch_y(spmv_plan_t plan, double *y_host);

/* y = alpha * A * x (the CSR5 handle's spmv(alpha, y),
 * CSR5_cuda/anonymouslib_cuda.h:262-284); alpha is applied to the finished
 * row sums (one rounded multiply), beta = 0 (beta != 0: spmv_execute_axpby). */
int spmv_execute_alpha(spmv_plan_t plan, double alpha, const double *x, double *y, uint32_t flags);

/* Kernels are launched on this stream (a hipStream_t; NULL = null stream). */
int spmv_set_stream(spmv_plan_t plan, void *hip_stream);

/* Bench helper: `iters` back-to-back executes (device x, device y) between two
 * hipEvents recorded on the plan's stream; *ms = elapsed milliseconds total. */
int spmv_time(spmv_plan_t plan, const double *x_dev, double *y_dev, int32_t iters,
              double *ms);

/* ---- multi-vector execute: Y = A X for k right-hand sides -----------------
 * Y[:, j] = A * X[:, j] for j in [0, k).  X and Y are row-major
 * ("interleaved") blocks: x_j[i] = X[i*ldx + j] (n rows), y_j[r] =
 * Y[r*ldy + j] (m rows), ldx >= k, ldy >= k.  beta = 0: the k used columns of
 * every row of Y are overwritten; columns [k, ldy) of Y are never written and
 * columns [k, ldx) of X are never read.  X and Y must not overlap.
 *
 * Per-column semantics: column j of Y depends on column j of X only and is,
 * bit for bit, what spmv_execute gives for that vector on this plan (COO:
 * within its atomics' order).  A NaN or Inf anywhere in column j' != j never
 * reaches column j; the non-finite rules of this header's opening comment
 * hold per column.
 *
 * Flags: SPMV_X_DEVICE, SPMV_Y_DEVICE and SPMV_ASYNC as for spmv_execute.
 * Host blocks are staged through plan-owned device buffers (hipMemcpy2DAsync;
 * only the k used columns travel) at a pitch of k rounded up to even.
 * SPMV_X_STAGED / SPMV_Y_STAGED, k < 1, k > SPMV_MULTI_MAX, ldx < k, ldy < k
 * and a NULL X or Y (with n, m > 0) return SPMV_ERROR_INVALID_VALUE before
 * any device work.  A multi execute clears the mark spmv_fetch_y needs, like
 * any other non-staged execute.
 *
 * Paths.  k is cut greedily into blocks of 8, 4 and 2 columns, then single
 * columns (block starts are even).  A block of width K >= 2 is ONE fused
 * launch -- the matrix is streamed once for K vectors -- when the plan is DIA,
 * ELL, or JDS without overflow rows, the block's X and Y addresses are
 * 16-byte aligned and ldx and ldy are even.  Every other block goes column by
 * column through the generic path, which serves every format: the column is
 * packed into a contiguous scratch vector (n + m doubles, allocated by the
 * first call that needs it; SPMV_ERROR_OUT_OF_MEMORY leaves the plan usable),
 * the plan's single-vector kernels run, and the result is written back into
 * its column (ld = 1: read / written in place).  The drop-in, the CSR5
 * handle, spmv_dist_*, HIP graphs and spmv_profile have no multi form. */
#define SPMV_MULTI_MAX 32
int spmv_execute_multi(spmv_plan_t plan, int32_t k, const double *X, int64_t ldx,
                       double *Y, int64_t ldy, uint32_t flags);

/* iters back-to-back device-resident multi executes between two events on
 * the plan's stream (the multi counterpart of spmv_time). */
int spmv_time_multi(spmv_plan_t plan, int32_t k, const double *X_dev, int64_t ldx,
                    double *Y_dev, int64_t ldy, int32_t iters, double *ms);

/* How the call above would be cut: widths[b] >= 2 is one fused launch over
 * that many consecutive columns, widths[b] == 1 is one column through the
 * generic path; the widths sum to k.  *n_blocks = the number of blocks
 * (widths beyond `cap` are not written).  A check and a documentation aid,
 * not a compute path. */
int spmv_multi_path(spmv_plan_t plan, int32_t k, const double *X, int64_t ldx,
                    const double *Y, int64_t ldy, uint32_t flags,
                    int32_t *widths, int32_t cap, int32_t *n_blocks);

/* ---- the BLAS form: y = alpha * A * x + beta * y ----------------------------
 * For every row r: y[r] = dadd_rn(dmul_rn(alpha, s[r]), dmul_rn(beta, y0[r]))
 * -- two rounded multiplies and one rounded add, never an FMA.  s[r] is, bit
 * for bit, the row sum spmv_execute gives on this plan (COO: within its
 * atomics' order); y0 is y on entry.  The non-finite rules of this header's
 * opening comment hold for s; a non-finite y0[r] with beta != 0 reaches row r
 * only.  x and y must not overlap.
 *
 * beta = 0 (either sign): y0 is never read -- a NaN there does not propagate --
 * and the call is spmv_execute_alpha: y = dmul_rn(alpha, s), bit for bit.
 * alpha = 0 is no shortcut: 0 * s is computed, NaN where s is not finite.
 *
 * Flags: SPMV_X_DEVICE, SPMV_Y_DEVICE, SPMV_ASYNC and SPMV_X_STAGED as for
 * spmv_execute.  y is an input: a host y with beta != 0 is uploaded into the
 * plan's y staging buffer first (H2D of m doubles), then downloaded, and
 * SPMV_Y_STAGED is refused.  Refusals come before any device work, all
 * SPMV_ERROR_INVALID_VALUE: a NULL plan; a NULL x or y (with n, m > 0; x may
 * be NULL with SPMV_X_STAGED); unknown flag bits; SPMV_Y_STAGED; SPMV_X_STAGED
 * without a staged x.  The call clears the mark spmv_fetch_y needs, like any
 * other non-staged execute.  The buffer contract above holds: 8-byte
 * alignment is enough, nothing outside [y, y + m) is read or written, nothing
 * outside [x, x + n) influences y.
 *
 * Paths (spmv_axpby_path).  Fused: the kernels with one writer per row -- CSR
 * (every kernel), ELL, DIA, and JDS without overflow rows -- apply alpha and
 * beta in their store epilogue, for one extra 8-byte read per row; the writer
 * loads y0[r] before it streams the row, with the very indexing its store
 * uses (DIA: the 16-byte row pair where y is 16-byte aligned).  Generic, every
 * other plan (SS, COO, CSS, BIN, HYB, JDS with overflow rows): the plan's own
 * kernels write the row sums into a plan-owned scratch vector (m doubles of
 * plain device memory, allocated by the first call that needs it and counted
 * in spmv_plan_info.device_bytes; SPMV_ERROR_OUT_OF_MEMORY leaves the plan
 * usable and y untouched), then one pass computes y from it.  A plan with
 * nothing stored (no diagonal, no entry) gives alpha * (+0.0) + beta * y0.
 *
 * Not covered: spmv_execute_multi, HIP graphs, spmv_profile, spmv_dist_*, the
 * drop-in (opt_hip.h) and the CSR5 handle have no alpha / beta form (the
 * handle keeps spmv_execute_alpha). */
int spmv_execute_axpby(spmv_plan_t plan, double alpha, const double *x,
                       double beta, double *y, uint32_t flags);

/* iters back-to-back device-resident axpby executes between two events on the
 * plan's stream (the axpby counterpart of spmv_time; y is updated in place
 * iters times). */
int spmv_time_axpby(spmv_plan_t plan, double alpha, const double *x_dev,
                    double beta, double *y_dev, int32_t iters, double *ms);

/* *fused = 1: the plan's kernel applies alpha and beta in its store epilogue;
 * 0: generic path.  A check and a documentation aid, like spmv_multi_path. */
int spmv_axpby_path(spmv_plan_t plan, int32_t *fused);

/* ---- execute with fused dot products: y = A x, w . y and y . y --------------
 * y = A * x, and from the same pass
 *   dots[0] = sum_r w[r] * y[r]   (w: m doubles; NULL: dots[0] = +0.0, nothing read)
 *   dots[1] = sum_r y[r] * y[r]
 * -- the inner products a Krylov iteration takes right after its SpMV (CG's
 * p . Ap, BiCGStab's t . s and t . t, the ||Av||^2 of GMRES and Lanczos),
 * without reading y back in two more launches.
 *
 * Results.  y[r] is, bit for bit, what spmv_execute gives on this plan (COO:
 * within its atomics' order).  t_r = dmul_rn(w[r], y[r]) and q_r =
 * dmul_rn(y[r], y[r]), from the y[r] that was stored; dots[0] is the sum of
 * the t_r and dots[1] the sum of the q_r over r < m, in rounded binary adds.
 * The order of the adds is a function of the plan and of the path alone: it
 * does not depend on the values, on what y or any plan-owned buffer held
 * before, or on timing, and no floating-point atomic takes part in the
 * reduction.  So the same plan with the same x and w gives the same 16 bytes
 * on every call (COO: given its y).  The two paths need not agree bit for bit
 * with each other, nor do different formats: a fused kernel's lane-to-row map
 * differs between them (DIA holds row pairs, JDS is permuted, adaptive CSR is
 * binned by length).  What is promised across all of them is
 *   |dots[0] - sum_r w[r] y[r]| <= (m + 8) * 2^-53 * sum_r |w[r] y[r]|
 * and likewise for dots[1] (one rounding per term, at most m - 1 adds in any
 * order, 8 for the second-order terms).
 * Rows >= m never contribute (padding, this header's opening comment): they
 * are dropped by a select, never by a zero weight.  There is no shortcut for
 * zeros: an empty row contributes w[r] * (+0.0), NaN where w[r] is not finite,
 * and a plan with nothing stored (nnz = 0) gives y = +0.0 and computes the
 * terms all the same.  m = 0 gives both dots as +0.0.  A non-finite term makes its dot
 * non-finite, with the class an IEEE sum gives.  w may be x itself (m = n,
 * CG's p . Ap); w and dots must not overlap y.  The buffer contract above
 * holds: 8-byte alignment of x, y and w is enough, the alignment of w is
 * independent of y's, and nothing outside [w, w + m) is read.
 *
 * Flags: SPMV_X_DEVICE, SPMV_Y_DEVICE, SPMV_X_STAGED and SPMV_ASYNC as for
 * spmv_execute; SPMV_W_DEVICE, SPMV_DOTS_DEVICE: w, dots are device pointers
 * on the plan's device (dots: 2 doubles, 8-byte aligned).  A host w is
 * uploaded into a plan-owned staging vector of m doubles, allocated at the
 * first use and counted in spmv_plan_info.device_bytes; host dots are copied
 * back (16 bytes) after the stream is synchronised.  SPMV_ASYNC needs device
 * x, y, w and dots.  Refusals come before any device work, all
 * SPMV_ERROR_INVALID_VALUE: a NULL plan; a NULL x or y (with n, m > 0; x may
 * be NULL with SPMV_X_STAGED); NULL dots; unknown flag bits; SPMV_Y_STAGED (y
 * always travels back, there is nothing to fetch later); SPMV_ASYNC without all of SPMV_X_DEVICE, SPMV_Y_DEVICE and
 * SPMV_DOTS_DEVICE (and SPMV_W_DEVICE when w is not NULL); SPMV_X_STAGED
 * without a staged x.  The call clears the mark spmv_fetch_y needs, like any
 * other non-staged execute.
 *
 * Paths (spmv_dot_path).  Every lane that stores a y[r] forms its terms, each
 * wave reduces them with a fixed butterfly, the workgroup's waves are added in
 * wave order, and one lane writes the pair with an ordinary store into the
 * workgroup's own slot of a plan-owned partials array (2 doubles per
 * workgroup of the plan's launch: plain device memory, allocated at the first
 * use and counted in device_bytes; SPMV_ERROR_OUT_OF_MEMORY for it or for the
 * w staging leaves the plan usable and y untouched).  Every workgroup writes
 * its slot on every call.  A last launch of ONE workgroup adds the slots in a
 * fixed order and writes dots.  Fused: the terms are formed in the store
 * epilogue of the plan's own kernel, for one extra 8-byte read per row (w[r],
 * loaded before the row is streamed, with the indexing the y store uses) --
 * CSR (every kernel), ELL, DIA, and JDS without overflow rows.  Generic, every
 * other plan (SS, COO, CSS, BIN, HYB, JDS with overflow rows, and any plan
 * with nnz = 0 after its zero fill): the plan's own kernels write y, one pass
 * streams y and w into the slots.
 *
 * Not covered: there is no dot form with alpha or beta, and none for
 * spmv_execute_multi, HIP graphs, spmv_profile, spmv_dist_*, the drop-in
 * (opt_hip.h) or the CSR5 handle. */
#define SPMV_W_DEVICE    0x80u   /* w is a device pointer on the plan's device      */
#define SPMV_DOTS_DEVICE 0x100u  /* dots is a device pointer (2 doubles, 8-byte aligned) */
int spmv_execute_dot(spmv_plan_t plan, const double *x, double *y,
                     const double *w, double *dots, uint32_t flags);

/* iters back-to-back device-resident dot executes (device x, y, w or NULL, and
 * dots) between two events on the plan's stream (the counterpart of spmv_time). */
int spmv_time_dot(spmv_plan_t plan, const double *x_dev, double *y_dev,
                  const double *w_dev, double *dots_dev, int32_t iters, double *ms);

/* *fused = 1: the plan's kernel forms the terms in its store epilogue; 0:
 * generic path.  A check and a documentation aid, like spmv_axpby_path. */
int spmv_dot_path(spmv_plan_t plan, int32_t *fused);

/* ---- conjugate gradients on a plan: solve A x = b, scalars on the device ---
 * spmv_cg_solve runs Hestenes-Stiefel conjugate gradients for a symmetric
 * positive definite A held by a square plan.  x is the initial guess on entry
 * and the iterate on exit; dinv is NULL or m doubles of a diagonal
 * preconditioner already inverted (Jacobi: 1 / a_ii -- the plan keeps no CSR,
 * so the caller supplies it).  The solve stops when rr <= rtol * rtol * bb
 * (rr = r . r of the recurrence, bb = b . b), tested before the first
 * iteration too, or after max_iters iterations.  The function returns
 * synchronised.
 *
 * The iteration.  Every operation is a rounded multiply, add or divide, never
 * an FMA.  Init: r = b; r = (-1) * A x + 1 * r through the plan's own
 * spmv_execute_axpby launches; z = dinv (.) r (no dinv: z = r), p = z, and rz
 * = r . z, rr, bb.  Per iteration:
 *   q = A p, pq = p . q    the plan's own spmv_execute_dot launches with x = w
 *                          = p: q has the bits spmv_execute gives on p, pq
 *                          the bits of spmv_execute_dot's dots[0]
 *   alpha = rz / pq;  x = x + alpha * p;  r = r - alpha * q;  z = dinv (.) r
 *   rz_new = r . z, rr = r . r;  beta = rz_new / rz;  p = z + beta * p
 * alpha, beta, rz, rr, pq, the iteration counter and the status live in a
 * plan-owned block of device memory: the kernels read them there, one lane
 * writes them with ordinary stores, and the host copies the block back once
 * per check_every (>= 1) iterations.  max_iters is enforced on the device, so
 * it need not be a multiple of check_every: once the solve is done the
 * launches left in a check interval return at once and move nothing in x, r,
 * p or the counter (the SpMV among them still runs, into the workspace q; the
 * host cuts the last interval at max_iters so that none runs past it).  The dot products are reduced as spmv_execute_dot's (lanes,
 * waves and workgroups in a fixed order, a function of m alone); no
 * floating-point atomic takes part, except the y-atomics COO plans already
 * have.  So x and info are a function of the plan, b, the x of entry, dinv,
 * rtol and max_iters: not of check_every, of SPMV_CG_GRAPH, of host or device
 * buffers, or of timing.
 *
 * Breakdown: if pq is not a finite number > 0 (an indefinite A, non-finite
 * data) no row of x, r or p moves in that iteration, the counter stays and
 * the status is SPMV_CG_BREAKDOWN.  Symmetry of A is the caller's
 * responsibility.
 *
 * Flags.  SPMV_CG_DEVICE: b, x and dinv are device pointers on the plan's
 * device (all or none; 8-byte alignment is enough, the buffer contract
 * above holds and nothing outside [v, v + m) is read or written); without it
 * they are host pointers, staged into plan-owned vectors.  SPMV_CG_GRAPH: one
 * check interval (check_every iterations, a linear chain) is captured once
 * into a HIP graph and launched per interval (a last interval cut at
 * max_iters is launched kernel by kernel); the graph is cached on the plan,
 * rebuilt when x's or dinv's device address or check_every changes (rtol and
 * max_iters travel through the scalar block) and destroyed with the plan.  No
 * device pointer moves on spmv_plan_update_values: a cached graph replays the
 * refreshed values.  CSS plans return SPMV_ERROR_NOT_SUPPORTED with the flag,
 * as spmv_graph_create does.
 *
 * Memory: r, p, q (3 m doubles), the partials (4 doubles per workgroup), the
 * scalar block and, for host pointers, the staging of b, x and dinv, besides
 * what the plan's axpby and dot executes own.  Plain device memory, allocated
 * at the first solve before any device work, counted in
 * spmv_plan_info.device_bytes, freed with the plan; SPMV_ERROR_OUT_OF_MEMORY
 * leaves the plan usable and x untouched.
 *
 * Refusals, all SPMV_ERROR_INVALID_VALUE before any device work, x untouched:
 * a NULL plan; NULL info; NULL b or x with m > 0; m != n; unknown flag bits
 * (every SPMV_X_* / SPMV_Y_* / SPMV_ASYNC bit included); max_iters < 0;
 * check_every < 1; rtol < 0 or NaN.  m = 0 gives SPMV_CG_CONVERGED with 0
 * iterations; max_iters = 0 runs the init only (CONVERGED or MAX_ITERS).  The
 * call clears the mark spmv_fetch_y needs, like any other non-staged execute.
 *
 * Not covered: other Krylov methods, non-symmetric A (an indefinite A ends in
 * SPMV_CG_BREAKDOWN), spmv_dist_*, the drop-in (opt_hip.h), the CSR5 handle, a
 * multi-vector or block form, spmv_profile phases. */
#define SPMV_CG_DEVICE 0x200u  /* b, x and dinv are device pointers on the plan's device (all or none) */
#define SPMV_CG_GRAPH  0x400u  /* replay each check interval as one hipGraph launch */

enum { SPMV_CG_CONVERGED = 0, SPMV_CG_MAX_ITERS = 1, SPMV_CG_BREAKDOWN = 2 };

typedef struct spmv_cg_info {
    int32_t status;      /* SPMV_CG_*                                        */
    int32_t iterations;  /* completed iterations (x updates applied)         */
    double rr, bb;       /* r.r of the recurrence at exit, b.b               */
    double rz;           /* r.z at exit (= rr without dinv)                  */
    double pq;           /* the last p.Ap the SpMV produced (+0.0 if none)   */
} spmv_cg_info_t;

int spmv_cg_solve(spmv_plan_t plan, const double *b, double *x, const double *dinv,
                  double rtol, int32_t max_iters, int32_t check_every,
                  uint32_t flags, spmv_cg_info_t *info);

/* *launches_per_iteration: the kernel launches one iteration enqueues (5 on a
 * plan whose dot path is fused: SpMV, dot finish, update, finish, direction).
 * A documentation aid, like spmv_dot_path. */
int spmv_cg_path(spmv_plan_t plan, int32_t *launches_per_iteration);

/* ---- value refresh: new values on a fixed sparsity pattern -----------------
 * Every layout decision of a plan (the format AUTO picks, slices, bins,
 * strips, tiles, windows, overflow rows, CSS lists) depends on (row_ptr,
 * col_idx) alone, so new values on the same pattern need no rebuild:
 * spmv_plan_update_prepare learns once where every CSR entry lives in the
 * plan's layout, spmv_plan_update_values then rewrites the value arrays.
 *
 * "The CSR the plan was created from" is the (row_ptr, col_idx) handed to
 * spmv_plan_create_csr / _csr32 (row pointers widened) / _csr_device; for
 * spmv_plan_create_coo it is the sorted COO as passed: its entry order and
 * spmv_coo_to_csr's row pointers.  For a plan of the transpose
 * (spmv_plan_create_csr_transposed / _csr_device_transposed) it is A's:
 * row_ptr has n + 1 entries in the plan's own (swapped) shape, and a pattern
 * that fails spmv_plan_create_csr's input check for A's shape is refused with
 * SPMV_ERROR_INVALID_VALUE like any wrong pattern.  (Prepare transposes the
 * pattern on the device: SPMV_ERROR_NOT_SUPPORTED from 2^31 - 1 entries on.)
 *
 * In place.  No device pointer of the plan changes: HIP graphs created before
 * an update replay the new values, fused and generic multi executes see them,
 * and the placement the plan drew at creation (VMM, SEARCH) is kept.
 *
 * Nothing but values moves.  The update rewrites CSR `val`, SS `val`,
 * ELL / HYB / JDS `ell_val` and `ovf_val`, DIA `val`, COO `val`, CSS `val` and
 * BIN `val1` (the names of spmv_plan_digest_name); every other array keeps
 * its digest.  Afterwards the plan is, byte for byte, the plan a fresh create
 * with these values and the same options would give.
 *
 * Padding stays what the builder wrote: +0.0 in ELL and DIA padding, the
 * kPad tails, BIN voids and slack, CSS and COO unit padding and SS tile
 * tails.  A NaN or Inf in val reaches only its own slot.  Where a builder
 * stores a function of the value, the refresh applies the same function: DIA
 * adds each entry into a +0.0 slot, so a -0.0 value is stored as +0.0.
 *
 * Refusals come before any device work, in this order: flag bits other than
 * the ones named at each function; a NULL plan; a NULL row_ptr, or a NULL
 * col_idx / val with nnz > 0; SPMV_ASYNC without SPMV_VAL_DEVICE -- all
 * SPMV_ERROR_INVALID_VALUE; then spmv_plan_update_values on a plan that was
 * not prepared: SPMV_ERROR_INVALID_VALUE, "not prepared" in spmv_last_error.
 *
 * Wrong pattern.  Prepare rebuilds the layout from the pattern it is given
 * (a transient shadow plan: the plan's resolved options, PLAIN placement,
 * values 1, 2, .., nnz) and compares every non-value array with the plan's
 * by digest; the plan's current non-zero values must also sit on slots the
 * pattern fills.  A pattern that does not reproduce the plan's layout returns
 * SPMV_ERROR_INVALID_VALUE with a message about the pattern; the plan stays
 * unprepared and fully usable.  (DIA stores no column indices: there the check
 * sees the diagonal offsets and the slots of the current non-zero values.)
 *
 * Layouts that merge entries.  Prepare succeeds only if every source index
 * 0 .. nnz-1 appears exactly once among the layout's value slots.  A DIA plan
 * built from rows with duplicate (row, col) entries adds several values into
 * one slot: no one-source-per-slot map exists, prepare returns
 * SPMV_ERROR_NOT_SUPPORTED and the plan stays usable (and unprepared).
 *
 * Empty plans (nnz = 0 or m = 0): both calls succeed and do nothing.
 *
 * Memory.  The map holds 4 bytes per value slot (8 where nnz >= 2^31 - 1),
 * allocated at prepare, counted in spmv_plan_info.device_bytes and freed with
 * the plan.  A host val is staged through a plan-owned buffer of nnz doubles,
 * allocated at the first host update; SPMV_ERROR_OUT_OF_MEMORY there leaves
 * the plan usable and its values untouched.  Prepare itself holds a second
 * plan and a device copy of the pattern while it runs.
 *
 * The drop-in (opt_hip.h), the CSR5 handle and spmv_dist_* have no update
 * form. */
#define SPMV_CSR_DEVICE 0x20u /* row_ptr / col_idx are device pointers on the plan's device */
#define SPMV_VAL_DEVICE 0x40u /* val is a device pointer on the plan's device               */

/* Teach the plan where every entry of the CSR it was created from lives in its
 * layout.  row_ptr (m + 1, int64) and col_idx (nnz) must be the pattern the
 * plan was built from, in the same entry order.  Costs about one plan build,
 * once.  Calling it again on a prepared plan is a cheap success (the pattern
 * is not looked at again).  Flags: SPMV_CSR_DEVICE. */
int spmv_plan_update_prepare(spmv_plan_t plan, const int64_t *row_ptr,
                             const int32_t *col_idx, uint32_t flags);

/* Replace the plan's values by val[0 .. nnz), in the order of that CSR.  The
 * plan's value arrays are rewritten in place, on the plan's stream.  Flags:
 * SPMV_VAL_DEVICE, and SPMV_ASYNC (device val only: return without
 * synchronising; val must stay valid until the stream has passed the update).
 * A device val needs the 8-byte alignment of a double, no more. */
int spmv_plan_update_values(spmv_plan_t plan, const double *val, uint32_t flags);

/* ---- HIP graph of the device-resident execute -----------------------------
 * The plan's launch sequence for (x_dev -> y_dev), captured `reps` times in a
 * row into one hipGraph (stream capture on a private stream) and
 * instantiated.  spmv_graph_launch enqueues all reps x n_kernels kernels on
 * the plan's current stream with one submission -- the per-call launch cost
 * that dominates small matrices, whose kernels are shorter than their
 * launches (the reference driver repeats SpMV until >= 1 s,
 * src/main.cpp:58-102).  Each rep computes exactly what spmv_execute does
 * (y bit-identical); x_dev and y_dev are fixed in the graph, so the caller
 * keeps them allocated until spmv_graph_destroy.  A graph replays the plan's
 * kernels on the plan's device arrays: destroy every graph of a plan before
 * the plan (launching a graph whose plan is gone is undefined; destroying it
 * is safe).  CSS plans (whose sweep
 * tags its progress flags with a per-launch sequence number) return
 * SPMV_ERROR_NOT_SUPPORTED. */
typedef struct spmv_graph_s *spmv_graph_t;
int spmv_graph_create(spmv_plan_t plan, const double *x_dev, double *y_dev, int32_t reps,
                      spmv_graph_t *graph);
/* flags: SPMV_ASYNC = return without synchronising the stream */
int spmv_graph_launch(spmv_graph_t graph, uint32_t flags);
/* `launches` back-to-back graph launches between two hipEvents on the plan's
 * stream; *ms = elapsed milliseconds total (launches x reps executes). */
int spmv_graph_time(spmv_graph_t graph, int32_t launches, double *ms);
int spmv_graph_destroy(spmv_graph_t graph);

typedef struct spmv_plan_info {
    int32_t format;          /* resolved spmv_format_t                         */
    int32_t device;
    int64_t m, n, nnz;
    int64_t stored_slots;    /* ELL/HYB/DIA slots incl. padding; CSR/SS = nnz   */
    int64_t device_bytes;    /* device memory held by the plan                 */
    int64_t algo_bytes;      /* compulsory bytes per execute (roofline model)  */
    int32_t row_ptr_bytes;   /* 4 or 8                                         */
    int32_t csr_lanes;       /* CSR / HYB overflow                             */
    int32_t ell_width;       /* ELL: max slice width; HYB: K                   */
    int32_t ss_sigma;
    int32_t n_diags;         /* DIA                                            */
    int32_t css_passes;      /* CSS: row passes, slabs per pass                */
    int32_t css_slabs;
    int32_t n_kernels;       /* launches per execute                           */
    int64_t overflow_nnz;    /* HYB: entries outside the ELL part              */
    int64_t empty_rows;
    int64_t css_split_rows;  /* CSS: rows split into pieces (long rows)       */
    char kernel[64];         /* name of the dominant kernel                    */
    int64_t bin_bins;        /* BIN: row bins (one Sum wave each), strips      */
    int64_t bin_strips;
    int32_t bin_strip_cols;  /* BIN: x strip width in columns                  */
    int32_t bin_pad;         /* BIN: segment padding (entries)                 */
    int32_t bin_sum_waves;   /* BIN: Sum waves per workgroup                   */
    int32_t bin_groups;      /* BIN: row groups (Mul launches)                 */
    int32_t placement;       /* BIN/DIA: the SPMV_PLACEMENT_* the build used   */
    int32_t placement_candidates; /* SEARCH: candidates timed                  */
    float placement_best_ms;  /* SEARCH: fastest / slowest candidate launch    */
    float placement_worst_ms;
    int32_t bin_long_len;     /* BIN: long-row threshold in use (0 = none)      */
    int32_t bin_product_order; /* BIN: SPMV_BIN_ORDER_SUM or _MUL (resolved)   */
    int64_t bin_long_rows;    /* BIN: rows on the run path, their run pieces    */
    int64_t bin_long_pieces;
    int64_t bin_products;     /* BIN: products + partials the Sum reads         */
    int64_t bin_long_entries; /* BIN: Mul entries in long blocks (with padding) */
    int64_t bin_sum_entries;  /* BIN: Sum-order positions (segments padded)     */
} spmv_plan_info_t;

int spmv_plan_info(spmv_plan_t plan, spmv_plan_info_t *info);

/* Layout digest (new; a check, not a compute path): one 64-bit hash per
 * device array of the plan (its logical bytes, position-keyed), so two plans
 * of one matrix -- e.g. a host build and a device build -- can be compared
 * array by array without copying them out.  *n_arrays = the plan's array
 * count (digests beyond `cap` are not written); spmv_plan_digest_name(plan,
 * k) names array k.  Every format (BIN: its entry, slot, destination and
 * run-path arrays and the small tables; not the product scratch). */
int spmv_plan_digest(spmv_plan_t plan, uint64_t *digests, int32_t cap, int32_t *n_arrays);
const char *spmv_plan_digest_name(spmv_plan_t plan, int32_t k);

/* *on_device = 1 when the plan's layout was built in HBM (by
 * spmv_plan_create_csr_device, or from a host CSR under
 * spmv_options_t::build), 0 when by the host builders. */
int spmv_plan_built_on_device(spmv_plan_t plan, int32_t *on_device);

const char *spmv_status_string(int status);
/* Detail of the last failure on the calling thread ("" if none). */
const char *spmv_last_error(void);

/* ---- multi-GPU in one process (new -- the reference is
 * single-device) -------------------------------------------------------------
 * The matrix is cut into nnz-balanced row ranges (spmv_partition_rows), one
 * plan per device over its rows with global column indices (n columns each).
 * x is copied to the first device and replicated by an RCCL broadcast over
 * xGMI; every device computes its rows; the y slices (padded to the longest
 * range) are all-gathered by RCCL into a full y on every device, and the
 * first device's copy is returned.  A C/C++ caller of the drop-in (the
 * reference driver, src/main.cpp:36,87) reaches config 5 through it; see
 * opt_hip.h SPMV_HIP_GPUS. */
typedef struct spmv_dist_s *spmv_dist_t;

/* The row cut a dist plan uses: cuts[parts+1] (spmv_partition_rows) and the
 * padded slice length (the longest range, >= 1).  Host only. */
int spmv_dist_layout(const int64_t *row_ptr, int64_t m, int32_t parts, int64_t *cuts, int64_t *slice_rows);

/* Host halves of a dist plan's data movement, exported so the reassembly can
 * be checked without a second GPU (the same code runs inside
 * spmv_dist_create_csr / spmv_dist_execute):
 *   spmv_dist_shard     part k's rows [cuts[k], cuts[k+1]): rp (rows + 1
 *                       entries) = row_ptr rebased to the part's first entry,
 *                       *entry0 = that entry (its col / val start there)
 *   spmv_dist_assemble  y (m doubles) from the all-gathered buffer of `parts`
 *                       slices of `slice` rows each (part k's rows at the
 *                       start of slice k, padding after them) */
int spmv_dist_shard(const int64_t *row_ptr, const int64_t *cuts, int32_t parts, int32_t k, int64_t *rp,
                    int64_t *entry0);
int spmv_dist_assemble(const double *gathered, const int64_t *cuts, int32_t parts, int64_t slice, double *y);

/* devices: n_devices distinct ordinals, or NULL for 0..n_devices-1.  opt
 * applies to every per-device plan (opt->device is ignored). */
int spmv_dist_create_csr(int32_t n_devices, const int32_t *devices, int64_t m, int64_t n, int64_t nnz,
                         const int64_t *row_ptr, const int32_t *col_idx, const double *val,
                         const spmv_options_t *opt, spmv_dist_t *dist);

/* y = A x with host x (n doubles) and host y (m doubles; NULL: the result
 * stays on the devices).  SPMV_X_STAGED: re-use the x broadcast by the
 * previous call (x may be NULL).  Returns after every device is done.  Any
 * other flag bit (SPMV_X_DEVICE, SPMV_Y_DEVICE, SPMV_ASYNC) is refused with
 * SPMV_ERROR_INVALID_VALUE. */
int spmv_dist_execute(spmv_dist_t dist, const double *x, double *y, uint32_t flags);

/* The full y of the last spmv_dist_execute (as assembled on the first
 * device) to host memory (m doubles) -- after a call made with y = NULL. */
int spmv_dist_fetch_y(spmv_dist_t dist, double *y_host);

/* Per-step times over `iters` steps with the staged x: the local SpMV (max
 * over devices of the event time on each device's stream) and, separately,
 * the all-gather of the y slices. */
int spmv_dist_time(spmv_dist_t dist, int32_t iters, double *spmv_ms, double *gather_ms);

/* n_devices, the row cuts (n_devices + 1, optional) and the per-device plans
 * (optional; owned by the dist plan). */
int spmv_dist_info(spmv_dist_t dist, int32_t *n_devices, int64_t *cuts, spmv_plan_t *plans);
int spmv_dist_destroy(spmv_dist_t dist);

/* ---- host utilities ------------------------------------------------------ */

/* LoadSparseMatrix semantics (src/util.cpp:30-66): skip leading '%' lines,
 * header "M N L", exactly L triplets, 1->0 based, stable row-major sort,
 * duplicates kept.  Arrays are malloc'd; release with spmv_free_host. */
int spmv_load_mtx(const char *path, int32_t *m, int32_t *n, int32_t *nnz,
                  int32_t **row_idx, int32_t **col_idx, double **val);
void spmv_free_host(void *p);

/* Banner-aware Matrix Market -> CSR with the CSR5 benchmark's semantics
 * (opt/Benchmark_SpMV_using_CSR5/CSR5_cuda/main.cu:157-306): needs a
 * "%%MatrixMarket matrix coordinate <field> <symmetry>" banner; field real |
 * integer | pattern (values 1.0); complex -> SPMV_ERROR_NOT_SUPPORTED;
 * symmetric/hermitian off-diagonal entries are mirrored (skew-symmetric is
 * not, as in the reference).  Rows keep file order (a mirrored entry right
 * after its original) unless SPMV_MTX_SORT_COLUMNS.  *info (optional) =
 * field (0 real, 1 integer, 2 pattern) | 4 if mirrored | 8 if skew. */
#define SPMV_MTX_SORT_COLUMNS 0x1u
#define SPMV_MTX_NO_EXPAND 0x2u
int spmv_load_mtx_csr(const char *path, uint32_t flags, int64_t *m, int64_t *n, int64_t *nnz,
                      int64_t **row_ptr, int32_t **col_idx, double **val, uint32_t *info);

/* Binary CSR cache ("SPMVCSR1": header, int64 row_ptr, int32 col, f64 val) so
 * a large Matrix Market file is parsed once.  Arrays from the loader are
 * malloc'd; release with spmv_free_host. */
int spmv_save_csr_bin(const char *path, int64_t m, int64_t n, int64_t nnz, const int64_t *row_ptr,
                      const int32_t *col_idx, const double *val);
int spmv_load_csr_bin(const char *path, int64_t *m, int64_t *n, int64_t *nnz, int64_t **row_ptr,
                      int32_t **col_idx, double **val);

/* glibc srand(seed) then out[i] = rand()/RAND_MAX -- CreateRandomVector
 * (src/util.cpp:92-102).  Consecutive calls continue the rand() stream. */
void spmv_srand(uint32_t seed);
void spmv_rand_vector(int32_t n, double *out);

/* VerifyResult (src/util.cpp:67-83): returns -1 if every row passes, else the
 * first failing row (abs_err > 1e-6 AND rel_err > 1e-6). */
int64_t spmv_verify_coo(int32_t m, int32_t nnz, const int32_t *row_idx,
                        const int32_t *col_idx, const double *val,
                        const double *x, const double *y);

/* COO (sorted rows) -> CSR, the linear scan of src/opt_crs.cpp:26-33. */
int spmv_coo_to_csr(int32_t m, int64_t nnz, const int32_t *row_idx, int64_t *row_ptr);

/* ---- synthetic matrices (BASELINE configs 2-5) ---------------------------- */
typedef enum spmv_gen_kind {
    SPMV_GEN_UNIFORM = 1,  /* `per_row` nnz per row, columns uniform on [0,n)   */
    SPMV_GEN_POWERLAW = 2, /* row length ~ P(k) ∝ k^-alpha on [1, max_len]      */
    SPMV_GEN_BANDED = 3    /* diagonals band_lo..band_hi (col - row), all present */
} spmv_gen_kind_t;

typedef struct spmv_gen_spec {
    int32_t kind;        /* spmv_gen_kind_t                                  */
    int32_t per_row;     /* UNIFORM                                          */
    int64_t m, n;        /* global shape                                     */
    int32_t max_len;     /* POWERLAW upper bound (10000 for config 3)        */
    double alpha;        /* POWERLAW exponent (2.0)                          */
    int32_t band_lo;     /* BANDED lowest offset  (-32 for config 4)         */
    int32_t band_hi;     /* BANDED highest offset (+31 for config 4)         */
    int32_t integer_values; /* 1: values in {0..9} (bitwise-exact sums)      */
    uint64_t seed;
} spmv_gen_spec_t;

/* Number of nonzeros of global rows [row_begin, row_end). */
int spmv_gen_count(const spmv_gen_spec_t *spec, int64_t row_begin, int64_t row_end,
                   int64_t *nnz);
/* Fill the CSR of rows [row_begin, row_end): row_ptr has (rows+1) entries and
 * starts at 0; columns are global, sorted within each row.  With col_idx and
 * val both NULL only row_ptr is filled (the row lengths are a function of
 * (seed, row) alone -- what an nnz-balanced shard cut needs). */
int spmv_gen_fill(const spmv_gen_spec_t *spec, int64_t row_begin, int64_t row_end,
                  int64_t *row_ptr, int32_t *col_idx, double *val);
/* x[i] for global indices [begin, begin+count): U[0,1) (or {0..9}). */
int spmv_gen_vector(uint64_t seed, int32_t integer_values, int64_t begin,
                    int64_t count, double *out);

/* nnz-balanced cut rows: cuts[k] = first row r with row_ptr[r] >= k*nnz/parts
 * (cuts[0] = 0, cuts[parts] = m). */
int spmv_partition_rows(const int64_t *row_ptr, int64_t m, int32_t parts, int64_t *cuts);

#ifdef __cplusplus
}
#endif
#endif /* SPMV_HIP_H */
