/*
 * gt4py_amd.h -- C ABI of the MI355X-native stencil-execution library (libgt4py_amd.so).
 *
 * This is the drop-in boundary for the hot path of gt4py.cartesian.  In the
 * reference every compiled backend exposes ONE native entry per stencil, generated at JIT time:
 *
 *     run_computation(std::array<uint_t,3> domain,
 *                     {py::buffer|py::object field, std::array<int_t,ndim> field_origin}...,
 *                     scalars by value..., py::object exec_info)
 *         -- /root/reference/src/gt4py/cartesian/backend/gtc_common.py:65-103  (bindings template)
 *         -- /root/reference/src/gt4py/cartesian/backend/gtcpp_backend.py:77-106 (argument marshalling)
 *         -- /root/reference/src/gt4py/cartesian/backend/gtc_common.py:30-62  (buffer -> SID, origin shift)
 *
 * The functions below are the same entry, one per hand-written kernel family, with the pybind11
 * objects replaced by plain pointers and sizes so that they can be bound from ctypes / cffi / any
 * FFI.  A field is described exactly by what `pybuffer_to_sid` extracts from the Python buffer
 * (pointer, shape, byte strides) plus the per-field origin the generated wrapper passes next to it.
 *
 * All pointers are DEVICE pointers (HIP, gfx950).  No function allocates or frees caller memory.
 * Every function returns 0 on success or a negative gt4mi_status; the message of the last failure
 * on the calling thread is available from gt4mi_last_error().  Launches are asynchronous on
 * `stream` (a hipStream_t passed as void*; NULL = the default stream); the caller synchronises
 * (the reference synchronises the device after every gt:gpu call unless device_sync=False --
 * backend/gtc_common.py:288-296; the Python host code does the same through gt4mi_stream_sync).
 */
#ifndef GT4PY_AMD_H
#define GT4PY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GT4MI_ABI_VERSION 8 /* 8: gt4mi_halo_fill (boundary conditions on the I/J ghost cells, one launch); 7: gt4mi_memory_write_probe (which memory group an allocation lives in); 6: GT4MI_PLAN_DIRECT_FENCED (release / acquire fences around the flags of the direct transport); 5: GT4MI_ERR_TIMEOUT (a direct-transport wait that runs out fails the plan, hard), GT4MI_PLAN_DIRECT_TIMEOUT_MS; 4: gt4mi_dist_lap5_f32, the direct transport (gt4mi_halo_plan_direct_*, GT4MI_PLAN_TRANSPORT), gt4mi_comm_create_local, schedules 2-4 */

typedef enum gt4mi_status {
    GT4MI_OK = 0,
    GT4MI_ERR_INVALID_ARGUMENT = -1, /* null pointer, bad enum, negative size ...              */
    GT4MI_ERR_OUT_OF_BOUNDS = -2,    /* origin/domain/halo do not fit in the field's shape     */
    GT4MI_ERR_UNSUPPORTED = -3,      /* combination not implemented by any kernel              */
    GT4MI_ERR_HIP = -4,              /* a HIP runtime call failed; see gt4mi_last_error()      */
    GT4MI_ERR_TIMEOUT = -5           /* direct transport: a neighbour never arrived; the plan has failed for good */
} gt4mi_status;

/* One stencil field argument.
 * Replaces the (py::buffer, origin) pair of run_computation (gtc_common.py:80-82, 30-62). */
typedef struct gt4mi_field {
    void* data;        /* device address of element [0,0,0]                                  */
    int64_t shape[3];  /* extent along I, J, K                                               */
    int64_t stride[3]; /* BYTE strides along I, J, K (any layout; I-contiguous is the fast one) */
    int64_t origin[3]; /* index of the first compute-domain point (the `_origin_[name]` entry) */
} gt4mi_field;

/* Optional timestamps, seconds of the monotonic clock (CLOCK_MONOTONIC = Python's time.perf_counter()).  May be NULL.
 *   run_cpp_*  the counterpart of exec_info["run_cpp_start_time"/"..end_time"] (gtc_common.py:83-99): they bracket
 *              the native call.  Launches are asynchronous here, so this is the time to ENQUEUE the work.
 *   run_hip_*  the time the work spent on the device, from a hipEvent pair on the launch stream: the interval ends
 *              when the host saw the stop event complete and is as long as the events measured.  Passing a
 *              non-NULL struct therefore makes the call wait for its own kernels (and only then).
 * Invariant: run_cpp_start_time <= run_hip_start_time <= run_hip_end_time. */
typedef struct gt4mi_exec_info {
    double run_cpp_start_time;
    double run_cpp_end_time;
    double run_hip_start_time;
    double run_hip_end_time;
} gt4mi_exec_info;

/* ---- library ------------------------------------------------------------------------------- */
int gt4mi_abi_version(void);
const char* gt4mi_last_error(void);
/* Writes a NUL-terminated description of the current HIP device (name, arch, CUs) into buf. */
int gt4mi_device_info(char* buf, size_t buflen);
int gt4mi_stream_sync(void* stream);

/* ---- 5-point star stencils (single statement, PARALLEL, interval(...)) ------------------------
 * Replaces run_computation of the stencils generated from
 *   variant 0: examples/lap_cartesian_vs_next.ipynb cell 7
 *              out = -4.0*inp[0,0,0] + inp[-1,0,0] + inp[1,0,0] + inp[0,-1,0] + inp[0,1,0]
 *   variant 1: docs/user/cartesian/index.rst:24-28
 *              out = -4.*inp + (inp[I+1] + inp[I-1] + inp[J+1] + inp[J-1])
 *   variant 2: tests/.../multi_feature_tests/test_suites.py:214 (Laplacian of horizontal diffusion)
 *              out = 4.0*inp - (inp[1,0,0] + inp[-1,0,0] + inp[0,1,0] + inp[0,-1,0])
 *   variant 3: tests/.../feature_tests/test_call_interface.py:159-164
 *              out = 0.25*(inp[0,1,0] + inp[0,-1,0] + inp[1,0,0] + inp[-1,0,0])
 * Expression trees are evaluated exactly as parsed (left-assoc, one rounding per op, no FMA).
 * `inp` needs a halo of 1 in I and J around the compute domain (field_info boundary
 * ((1,1),(1,1),(0,0)), module_generator.py:56-106); `inp` and `out` must not overlap
 * (gtir_to_oir.py:19-46 rejects such stencils). */
enum { GT4MI_LAP_NOTEBOOK = 0, GT4MI_LAP_DOCS = 1, GT4MI_LAP_SUITE = 2, GT4MI_LAP_AVG = 3 };
/* flags (f32 entry only): GT4MI_LAP_LITERAL_F32 = float literals typed float32
 * (literal_float_precision=32, frontend/gtscript_frontend.py:1250-1259): all arithmetic in float.
 * Default: literals are float64, so float fields are widened, computed in double and rounded once
 * on store (gtc/passes/gtir_upcaster.py:43-143). */
enum { GT4MI_LAP_LITERAL_F32 = 1 };

int gt4mi_lap5_f64(const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* out,
                   int variant, int flags, void* stream, gt4mi_exec_info* info);
int gt4mi_lap5_f32(const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* out,
                   int variant, int flags, void* stream, gt4mi_exec_info* info);

/* ---- horizontal diffusion ----------------------------------------------------------------------
 * Replaces run_computation of `horizontal_diffusion` (flux limiter) and
 * `simple_horizontal_diffusion` / TestHorizontalDiffusion (no limiter):
 *   tests/.../multi_feature_tests/stencil_definitions.py:316-328, :206-216; test_suites.py:212-220.
 * `in_field` needs a halo of 2 in I and J.  The diffusion coefficient is a field (coeff != NULL)
 * or a scalar parameter (coeff == NULL, value in coeff_scalar; for the f32 entry the scalar is
 * first rounded to float when GT4MI_HDIFF_COEFF_F32 is set, i.e. the parameter was declared
 * float32).  flags:
 *   GT4MI_HDIFF_LIMITER       apply the flux limiter (ternary -> select, npir_codegen.py:225)
 *   GT4MI_HDIFF_INTERNAL_F32  (f32 entry only) literals typed float32 (literal_float_precision=32):
 *                             all arithmetic in float.  Default follows the reference default
 *                             (float64 literals => lap/flx/fly in double, gtir_upcaster.py:43-143). */
enum { GT4MI_HDIFF_LIMITER = 1, GT4MI_HDIFF_INTERNAL_F32 = 2, GT4MI_HDIFF_COEFF_F32 = 4 };

int gt4mi_hdiff_f64(const int64_t domain[3], const gt4mi_field* in_field,
                    const gt4mi_field* out_field, const gt4mi_field* coeff, double coeff_scalar,
                    int flags, void* stream, gt4mi_exec_info* info);
int gt4mi_hdiff_f32(const int64_t domain[3], const gt4mi_field* in_field,
                    const gt4mi_field* out_field, const gt4mi_field* coeff, double coeff_scalar,
                    int flags, void* stream, gt4mi_exec_info* info);

/* The same stencils on a RING of the compute domain only (NEW: the boundary part of an IJ-decomposed apply, SURVEY.md
 * section 8e; one launch for up to four boxes).  widths / inner / outer are {low I, high I, low J, high J}.
 *   gt4mi_hdiff_ring_*: the points less than widths[side] away from a side of the domain (0 = that side has no ring);
 *                       same arguments, bounds and alias rules as gt4mi_hdiff_*.
 *   gt4mi_lap5_ring_*:  (the domain grown by outer[side]) minus (the domain shrunk by inner[side]); `inp` must be readable
 *                       one point beyond the grown domain.  outer > 0 is what communication-avoiding time stepping
 *                       computes redundantly inside its ghost region (gt4mi_dist_lap5_f64_skewed). */
int gt4mi_hdiff_ring_f64(const int64_t domain[3], const gt4mi_field* in_field, const gt4mi_field* out_field,
                         const gt4mi_field* coeff, double coeff_scalar, int flags, const int widths[4], void* stream,
                         gt4mi_exec_info* info);
int gt4mi_hdiff_ring_f32(const int64_t domain[3], const gt4mi_field* in_field, const gt4mi_field* out_field,
                         const gt4mi_field* coeff, double coeff_scalar, int flags, const int widths[4], void* stream,
                         gt4mi_exec_info* info);
int gt4mi_lap5_ring_f64(const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* out, int variant, int flags,
                        const int outer[4], const int inner[4], void* stream, gt4mi_exec_info* info);
int gt4mi_lap5_ring_f32(const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* out, int variant, int flags,
                        const int outer[4], const int inner[4], void* stream, gt4mi_exec_info* info);

/* ---- vertical tridiagonal (Thomas) solve --------------------------------------------------------
 * Replaces run_computation of `tridiagonal_solver` (stencil_definitions.py:219-232):
 * FORWARD sweep rewrites sup and rhs IN PLACE (they are READ_WRITE API fields), BACKWARD sweep
 * writes out.  domain[2] must be >= 2 (min_sequential_axis_size, gtir_k_boundary.py:78-109). */
int gt4mi_tridiag_f64(const int64_t domain[3], const gt4mi_field* inf, const gt4mi_field* diag,
                      const gt4mi_field* sup, const gt4mi_field* rhs, const gt4mi_field* out,
                      void* stream, gt4mi_exec_info* info);
int gt4mi_tridiag_f32(const int64_t domain[3], const gt4mi_field* inf, const gt4mi_field* diag,
                      const gt4mi_field* sup, const gt4mi_field* rhs, const gt4mi_field* out,
                      void* stream, gt4mi_exec_info* info);

/* ---- halo pack / unpack (NEW: the reference has no multi-device path) -----
 * Copies the box [lo, lo+extent) of `field` (indices relative to element [0,0,0], NOT to the
 * origin) to / from a dense buffer laid out I-fastest, then J, then K.  elem_size is 4 or 8. */
int gt4mi_halo_pack(const gt4mi_field* field, const int64_t lo[3], const int64_t extent[3],
                    void* buffer, int elem_size, void* stream);
int gt4mi_halo_unpack(const gt4mi_field* field, const int64_t lo[3], const int64_t extent[3],
                      const void* buffer, int elem_size, void* stream);

/* ---- boundary-condition halo fill (ABI 8; NEW: no reference counterpart -- gt4py leaves boundary conditions to array slicing on
 * its numpy / cupy storages) --------------------------------------------------------------------------------------------------
 * Fills the I/J ghost cells of `nfields` fields (each with its own pointer, strides and origin; all of item size `elem_size` =
 * 1, 2, 4 or 8) from their own compute domain [origin, origin + domain), in ONE kernel launch per 8 fields, on `stream`, without
 * synchronisation or allocation.  Bit patterns are moved, nothing is computed: bool and integer fields work, NaN payloads and
 * the sign of zero survive.  K is never extended; a Field[IJ] is domain[2] = 1 with K stride 0; a field whose I or J stride
 * is 0 is refused.
 *   halo     {lo_i, hi_i, lo_j, hi_j} >= 0, inside every array: lo <= origin, origin + domain + hi <= shape.
 *   mode_i, mode_j   per axis; the index (relative to the domain, n cells) a ghost cell at distance d >= 1 takes its value from:
 *              GT4MI_HALO_NONE           axis not touched
 *              GT4MI_HALO_PERIODIC       low: n - d      high: d - 1       (numpy.pad "wrap";      widths <= n)
 *              GT4MI_HALO_ZERO_GRADIENT  low: 0          high: n - 1       (numpy.pad "edge")
 *              GT4MI_HALO_SYMMETRIC      low: d - 1      high: n - d       (numpy.pad "symmetric"; widths <= n)
 *              GT4MI_HALO_REFLECT        low: d          high: n - 1 - d   (numpy.pad "reflect";   widths <= n - 1)
 *              GT4MI_HALO_CONSTANT       *value (one item of elem_size bytes for the call)         (numpy.pad "constant")
 *            A width beyond the bound of its mode is GT4MI_ERR_INVALID_ARGUMENT (numpy.pad iterates there; this does not).
 *   sides    bit mask of GT4MI_HALO_I_LO | _I_HI | _J_LO | _J_HI: a decomposed caller fills the sides without a neighbour.
 *            With GT4MI_HALO_DRY_RUN every check runs and *launches is set, nothing is enqueued.
 * The result is "the I sides first, then the J sides over the whole padded I range [origin - lo_i, origin + domain + hi_i)",
 * which is how numpy.pad treats axes: a corner cell is written iff its J side is selected and mode_j != NONE; it holds *value
 * for mode_j CONSTANT, else the cell (map_i(i), map_j(j)) (or *value for mode_i CONSTANT) where its I side is selected and
 * mode_i != NONE, else the CURRENT content of (i, map_j(j)): the ghost column as the caller left it, e.g. a halo exchange that
 * ran just before.  No other byte of the arrays changes.  The fields of one call must not overlap one another.
 * Every check runs before the first launch.  *launches (may be NULL) = the kernels the call enqueued. */
enum { GT4MI_HALO_NONE = 0, GT4MI_HALO_PERIODIC = 1, GT4MI_HALO_ZERO_GRADIENT = 2, GT4MI_HALO_SYMMETRIC = 3, GT4MI_HALO_REFLECT = 4,
       GT4MI_HALO_CONSTANT = 5 };
enum { GT4MI_HALO_I_LO = 1, GT4MI_HALO_I_HI = 2, GT4MI_HALO_J_LO = 4, GT4MI_HALO_J_HI = 8, GT4MI_HALO_ALL_SIDES = 15,
       GT4MI_HALO_DRY_RUN = 256 };
int gt4mi_halo_fill(const gt4mi_field* fields, int nfields, const int64_t domain[3], const int64_t halo[4], int mode_i,
                    int mode_j, int sides, const void* value, int elem_size, void* stream, int* launches);

/* ---- field statistics (NEW: no reference counterpart -- gt4py leaves reductions to numpy / cupy on its numpy / cupy storages) ------
 * One pass over the compute domain [origin, origin + domain) of `nfields` entries, 8 per launch, plus ONE finishing launch, on
 * `stream`, without synchronisation or allocation.  Entry n is fields[n] and, where `others` is not NULL and others[n].data is not
 * NULL, a second field others[n] of the same item size (`elem_size` = 4: float32, 8: float64).  x = a, or a - b rounded once in
 * float64; ALL arithmetic is float64.  result[n * 8 + slot] (device memory, float64):
 *   GT4MI_STATS_COUNT      number of domain points                      GT4MI_STATS_NONFINITE  points where x is NaN or +-Inf
 *   GT4MI_STATS_SUM        sum of x            GT4MI_STATS_SUM_ABS  sum of |x|            GT4MI_STATS_SUM_SQ  sum of x * x
 *   GT4MI_STATS_MIN / _MAX min / max of x: NaN if any x is NaN (as numpy.min; payload and sign unspecified), min(-0, +0) = -0 and
 *                          max(-0, +0) = +0, so they do not depend on the order
 *   GT4MI_STATS_DOT        sum of a * b with a second field, else 0
 * THE ORDER OF THE ADDITIONS IS PART OF THE CONTRACT: it is a function of `domain` alone (csrc/field_stats.hip.h states it,
 * tests/stats_ref.py restates it in numpy) -- not of pointers, strides, padding, alignment, the number of entries in the call or
 * anything about the device.  The same domain data gives the same bits, always.
 * A second field may have byte stride 0 along an axis: a lower-dimensional weight (an IJ cell-area field against an IJK field
 * for sum a * area), exempt from the shape check on that axis; `fields` may not.  With a weight the slots other than _DOT still
 * describe a - b: for sum a * w next to the statistics of `a` itself pass `a` twice, once alone and once with w (two entries, one
 * launch).
 *   workspace   device memory for the tiles' partial results, 8-byte aligned, *workspace_needed bytes (a function of nfields and
 *               domain; at most nfields * 256 KiB); `result` and `workspace` must not overlap the fields or one another
 *   flags       GT4MI_STATS_DRY_RUN: every check runs, *workspace_needed and *launches are set, nothing is enqueued; workspace and
 *               result may then be NULL (which is how to ask for the size)
 * Every check runs before the first launch; a refused call enqueues nothing.  *launches (may be NULL) = the kernels the call
 * enqueues: ceil(nfields / 8) + 1. */
enum { GT4MI_STATS_COUNT = 0, GT4MI_STATS_NONFINITE = 1, GT4MI_STATS_SUM = 2, GT4MI_STATS_SUM_ABS = 3, GT4MI_STATS_SUM_SQ = 4,
       GT4MI_STATS_MIN = 5, GT4MI_STATS_MAX = 6, GT4MI_STATS_DOT = 7, GT4MI_STATS_SLOTS = 8 };
enum { GT4MI_STATS_DRY_RUN = 1 };
int gt4mi_field_stats(const gt4mi_field* fields, const gt4mi_field* others, int nfields, const int64_t domain[3], int elem_size,
                      void* workspace, int64_t workspace_bytes, double* result, int flags, void* stream,
                      int64_t* workspace_needed, int* launches);

/* ---- per-level statistics, K profiles (NEW entry, additive: the ABI version stays 8; no reference counterpart -- GTScript has no
 * reduction over I and J, gt4py leaves `field.sum(axis=(0, 1))` to numpy / cupy on its numpy / cupy storages) --------------------------
 * gt4mi_field_stats for EVERY LEVEL k of the domain at once: the eight GT4MI_STATS_* slots over the plane (ni, nj) of level k, with
 * their meaning, NaN rules and signed-zero rules, plus the horizontal mean.  One pass over the field (8 entries per launch) plus ONE
 * finishing launch, on `stream`, without synchronisation or allocation.  Arguments, entries (a second field, which may be a
 * broadcast weight such as an IJ cell area), flags and checks are those of gt4mi_field_stats.
 *   workspace   partial[((entry * nk + k) * TL + t) * 8 + slot], *workspace_needed = nfields * nk * TL * 64 bytes
 *   result      result[(entry * 9 + row) * nk + k] (device memory, float64; nfields * 9 * nk * 8 bytes): rows 0-7 are the slots, row
 *               GT4MI_LEVEL_STATS_MEAN = SUM / COUNT (one IEEE division).  Slot-major: every profile is a contiguous run of nk
 *               doubles that a later kernel on the same stream can read as a K field.
 * THE ORDER OF THE ADDITIONS OF A LEVEL IS PART OF THE CONTRACT: it is a function of (ni, nj) alone (csrc/level_stats.hip.h states
 * it, tests/level_stats_ref.py restates it in numpy) -- not of nk or of which level it is, of pointers, strides, padding, alignment,
 * the number of entries in the call or anything about the device:
 *   rows    RW = ceil(nj / (4 * LT)) rows (one j each) per wave, LT = GT4MI_LEVEL_STATS_MAX_TILES; TL = ceil(nj / (4 * RW)) tiles of 4
 *           waves per level; wave w of tile t takes the rows [(4 t + w) RW, (4 t + w + 1) RW) that exist
 *   lane, wave, tile   as gt4mi_field_stats: lane l adds the columns with (i mod 256) div 4 == l from +0.0 in (row, i) order, a
 *           butterfly over the 64 lanes, the four waves left to right
 *   finish  the TL tile values of a level are halved level by level, new[i] = old[2i] (+) old[2i + 1], an odd last one carried up
 * The same plane gives the same bits, always; they are NOT the bits gt4mi_field_stats gives for that plane as a domain of its own.
 * A level of more than 2^40 points, and nk * TL of more than 2^24, are GT4MI_ERR_UNSUPPORTED.
 * Every check runs before the first launch; a refused call enqueues nothing.  *launches (may be NULL) = the kernels the call
 * enqueues: ceil(nfields / 8) + 1. */
#ifndef GT4MI_LEVEL_STATS_MAX_TILES
#define GT4MI_LEVEL_STATS_MAX_TILES 32 /* part of the bit contract; a build-time define only so that it could be measured */
#endif
enum { GT4MI_LEVEL_STATS_MEAN = 8, GT4MI_LEVEL_STATS_ROWS = 9 };
int gt4mi_level_stats(const gt4mi_field* fields, const gt4mi_field* others, int nfields, const int64_t domain[3], int elem_size,
                      void* workspace, int64_t workspace_bytes, double* result, int flags, void* stream,
                      int64_t* workspace_needed, int* launches);

/* ---- statistics along the lines of I, J or K (NEW entry, additive: the ABI version stays 8; no reference counterpart -- GTScript has no
 * reduction over I or J, gt4py leaves `field.sum(axis=0)` to numpy / cupy on its numpy / cupy storages) ------------------------------
 * gt4mi_field_stats for EVERY LINE of the domain along `axis` (0: I, the zonal mean; 1: J; 2: K) at once: the eight GT4MI_STATS_* slots
 * over the n = domain[axis] items of the line, with their meaning, NaN rules and signed-zero rules, plus the mean.  One pass over the
 * field (8 entries per launch) plus, where a line has more than one segment, ONE finishing launch, on `stream`, without
 * synchronisation or allocation.  Entries (a second field, which may be a broadcast weight such as an IJ cell area), flags and the
 * checks of fields, workspace and result are those of gt4mi_field_stats.
 *   workspace   *workspace_needed = nfields * lines * S * 8 * 8 bytes (lines = the product of the two other extents, S below)
 *   result      result[((entry * 9 + row) * nB + b) * nA + a] (device memory, float64; nfields * 9 * lines * 8 bytes), A < B the two
 *               remaining axes in I, J, K order: rows 0-7 are the slots, row GT4MI_LINE_STATS_MEAN = SUM / COUNT (one IEEE division).
 *               Every (entry, row) is one contiguous section that a later kernel on the same stream can read as a JK (axis I), IK
 *               (axis J) or IJ (axis K) field with strides (8, 8 * nA) bytes.
 * THE ORDER OF THE ADDITIONS OF A LINE IS PART OF THE CONTRACT: it is a function of n alone (csrc/line_stats.hip.h states it,
 * tests/line_stats_ref.py restates it in plain Python and in numpy) -- not of the axis, the layout, the path, pointers, strides, the
 * number of entries in the call, the grid or anything about the device:
 *   segments  G = GT4MI_LINE_STATS_SEGMENT items, S = ceil(n / G); segment s is the items m in [s G, min(n, (s + 1) G))
 *   inside    four accumulator sets, set p takes the items with m mod 4 == p in increasing m (sums from +0.0, min from +inf, max from
 *             -inf, counts from 0); a set whose sum |x| ended NaN sets min = max = NaN; the segment is (A0 (+) A1) (+) (A2 (+) A3),
 *             all four sets taking part, also one that owned no item
 *   across    the S segment values are halved level by level, new[i] = old[2i] (+) old[2i + 1], an odd last one carried up
 * The same line gives the same bits, always; they are NOT the bits gt4mi_field_stats gives for that line as a domain of its own.
 * *path (may be NULL) = which kernel the strides of the call select: GT4MI_LINE_STATS_PATH_LANES (an axis other than `axis` has unit
 * stride in every field, 0 allowed in a second field: lanes along it, every step a coalesced row), GT4MI_LINE_STATS_PATH_TILES (`axis`
 * itself has unit stride in every field: tiles of 64 lines x 128 bytes go through LDS), GT4MI_LINE_STATS_PATH_ITEMS (anything else:
 * item by item, uncoalesced).  The path changes how the items reach the registers, never the result.
 * Refused before anything is enqueued (GT4MI_ERR_INVALID_ARGUMENT unless noted): `fields` or `domain` NULL, nfields < 1, more than
 * 65535 fields (UNSUPPORTED), an axis other than 0, 1 or 2, an empty domain, an item size other than 4 or 8 (UNSUPPORTED), unknown flag
 * bits, what gt4mi_field_stats refuses of a field, the workspace or the result (NULL outside a dry run, too small, not aligned to 8
 * bytes, overlapping a field or one another), and more than 2^30 (line, segment) pairs (UNSUPPORTED).
 * *launches (may be NULL) = the kernels the call enqueues: ceil(nfields / 8), plus 1 where S > 1. */
#ifndef GT4MI_LINE_STATS_SEGMENT
#define GT4MI_LINE_STATS_SEGMENT 256 /* G: part of the bit contract; a build-time define only so that it could be measured */
#endif
enum { GT4MI_LINE_STATS_MEAN = 8, GT4MI_LINE_STATS_ROWS = 9 };
enum { GT4MI_LINE_STATS_PATH_LANES = 0, GT4MI_LINE_STATS_PATH_TILES = 1, GT4MI_LINE_STATS_PATH_ITEMS = 2 };
int gt4mi_line_stats(const gt4mi_field* fields, const gt4mi_field* others, int nfields, const int64_t domain[3], int axis, int elem_size,
                     void* workspace, int64_t workspace_bytes, double* result, int flags, void* stream, int64_t* workspace_needed,
                     int* launches, int* path);

/* ---- layout-converting field copy (NEW entry, additive: the ABI version stays 8.  Replaces what the reference does with numpy /
 * cupy slicing on its numpy / cupy storages and with `cp.asarray` (storage/cartesian/utils.py:187-189): moving a field between two
 * layouts, a storage and a dense buffer in numpy's C order among them) ------------------------------------------------------------
 * Copies the box [origin, origin + extent) of src[n] to the box [origin, origin + extent) of dst[n] (each side of each pair with its
 * own pointer, byte strides and origin, any layout) for `nfields` pairs, in ONE kernel launch per 8 pairs, on `stream`, without
 * synchronisation or allocation.  Items of equal size (1, 2, 4 or 8 bytes) are moved as bit patterns: bool and integer fields work,
 * NaN payloads and the sign of zero survive.  With GT4MI_COPY_CONVERT the sizes may be 8 -> 4 (float64 -> float32, ONE rounding to
 * nearest even) or 4 -> 8 (float32 -> float64, exact); a NaN stays a NaN of the same sign, its payload is unspecified.
 * The library picks a path per pair from strides and alignment (csrc/field_copy.hip.h) and reports it in paths[n] (may be NULL):
 *   GT4MI_COPY_PATH_ROWS    both sides have unit item stride along the same axis (of extent > 1): rows, 16-byte lanes where both allow
 *   GT4MI_COPY_PATH_TILES   unit item stride along different axes: a transpose, tiles through on-chip memory, coalesced on both sides
 *   GT4MI_COPY_PATH_ITEMS   anything else: a side without unit stride on an axis of extent > 1, a broadcast src
 * A src stride of 0 is allowed and broadcasts; a dst stride of 0 on an axis of extent > 1 is GT4MI_ERR_INVALID_ARGUMENT (reported
 * before an origin or extent outside the array along the same axis, as the other entries do).  The bytes
 * of a dst box (first to last item) must meet neither those of any src box nor of another dst box of the call
 * (GT4MI_ERR_UNSUPPORTED).  No byte outside the dst boxes changes.  An extent with a zero entry is GT4MI_OK, nothing enqueued.
 * Every check runs before the first launch; a refused call enqueues nothing.  With GT4MI_COPY_DRY_RUN the checks run, paths and
 * *launches are set and no device is touched.  *launches (may be NULL) = the kernels the call enqueues: ceil(nfields / 8). */
enum { GT4MI_COPY_PATH_ROWS = 0, GT4MI_COPY_PATH_TILES = 1, GT4MI_COPY_PATH_ITEMS = 2 };
enum { GT4MI_COPY_CONVERT = 1, GT4MI_COPY_DRY_RUN = 256 };
int gt4mi_field_copy(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const int64_t extent[3],
                     int dst_elem_size, int src_elem_size, int flags, void* stream, int* paths, int* launches);

/* ---- conservative vertical remapping (NEW entry, additive: the ABI version stays 8; no reference counterpart -- gt4py leaves remapping
 * a column from one set of levels to another to user stencils: a FORWARD sweep with a carried run-time index, a `while` and a read at
 * a run-time K index, one field per call) ---------------------------------------------------------------------------------------------
 * Remaps the cell means src[n] on the source levels of every column (i, j) of the box to cell means dst[n] on the target levels of
 * that column, for `nfields` pairs that share ONE pair of edge fields, in ONE kernel launch per 8 pairs, on `stream`, without
 * synchronisation or allocation.  The box is [origin, origin + extent_ij) in I and J of every field; along K a src holds `ns` levels
 * from its origin, a dst `nd`, src_edges `ns + 1` and dst_edges `nd + 1`.  `elem_size` (fields) and `edge_elem_size` (edge fields) are
 * 4 (float32) or 8 (float64).  An edge field may have byte stride 0 along I and / or J: a Field[K] of fixed levels broadcasts without a
 * copy and is exempt from the shape check on that axis.  A src stride of 0 broadcasts too; a dst stride of 0 on an extent above 1 is
 * GT4MI_ERR_INVALID_ARGUMENT.
 * THE ARITHMETIC IS PART OF THE CONTRACT (csrc/vertical_remap.hip.h states it again, tests/vertical_remap_ref.py restates it in plain
 * Python).  All of it is float64, one IEEE rounding per operation, no FMA; float32 items are widened exactly on load and the result is
 * rounded once on store.  Per column: source edges zs[0..ns], target edges zd[0..nd], both meant to increase strictly with k, source
 * means q[0..ns-1], target means out[0..nd-1].  The first source cell extends to -inf and the last to +inf: a target cell that reaches
 * outside the source range sees the end cell's mean there, the weights still sum to 1, nothing is extrapolated.  A source index k is
 * kept across the target cells of the column and never decreases.  For target cell m, lo = zd[m], hi = zd[m+1], d = hi - lo:
 *   1. advance: while k < ns-1 and not (zs[k+1] > lo): k += 1
 *   2. for each overlapping k, in increasing order:
 *        l = lo if k == 0    else max(lo, zs[k])     (max(a, b) = b if b > a else a)
 *        r = hi if k == ns-1 else min(hi, zs[k+1])   (min(a, b) = b if b < a else a)
 *        w = (r - l) / d, one IEEE division;  t = w * v_k
 *        the first term initialises the accumulator (a lone -0.0 survives), later terms are added in this order
 *        stop after the term for which k == ns-1 or zs[k+1] >= hi, otherwise k += 1
 *   3. out[m] is the accumulator: no final division, the weights carry 1/d
 *   GT4MI_REMAP_PCM (piecewise constant)        v_k = q[k]
 *   GT4MI_REMAP_PLM (piecewise linear, limited) v_k = q[k] + s[k] * (0.5 * (xl + xr) - 0.5),  h[k] = zs[k+1] - zs[k],
 *        xl = (l - zs[k]) / h[k],  xr = (r - zs[k]) / h[k];  the slope across the cell: s[0] = s[ns-1] = 0, and for 0 < k < ns-1 with
 *        dl = q[k] - q[k-1], dr = q[k+1] - q[k]:  if dl * dr > 0 then g = (q[k+1] - q[k-1]) / (0.5 * h[k-1] + h[k] + 0.5 * h[k+1]) * h[k]
 *        (left to right) and s[k] = copysign(min(|g|, 2|dl|, 2|dr|), g) (min as above, in this order), otherwise s[k] = 0
 * With zd identical to zs, pcm returns q bit for bit; plm too, except that -0.0 comes back as +0.0 (q + s * 0.0) where the slope is not
 * negative.  A column makes at most
 * ns + nd - 1 terms.  k only grows and every step of either loop stops or increments k, so both loops are bounded by integer counters
 * whatever the data holds: NaN, repeated and non-monotone edges give that column whatever IEEE arithmetic gives (0 / 0 = NaN for a
 * target cell of zero thickness) and affect no other column.  Edges that DECREASE with k are out of scope: negate the coordinate.
 * Refusals: null pointers, nfields < 1, ns < 1, nd < 1, an unknown method or flag (GT4MI_ERR_INVALID_ARGUMENT); an item size other
 * than 4 or 8, a misaligned field (GT4MI_ERR_UNSUPPORTED); a box that does not fit its field (GT4MI_ERR_OUT_OF_BOUNDS); the bytes of a
 * dst box (first to last item) meeting those of any src box, of an edge field or of another dst box (GT4MI_ERR_UNSUPPORTED, the rule of
 * gt4mi_field_copy).  No byte outside the dst boxes changes.  An extent with a zero entry is GT4MI_OK, nothing enqueued.
 * Every check runs before the first launch; a refused call enqueues nothing.  With GT4MI_REMAP_DRY_RUN the checks run, *launches is
 * set and no device is touched.  *launches (may be NULL) = the kernels the call enqueues: ceil(nfields / 8). */
enum { GT4MI_REMAP_PCM = 0, GT4MI_REMAP_PLM = 1 };
enum { GT4MI_REMAP_DRY_RUN = 256 };
int gt4mi_vertical_remap(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* src_edges,
                         const gt4mi_field* dst_edges, const int64_t extent_ij[2], int64_t ns, int64_t nd, int elem_size,
                         int edge_elem_size, int method, int flags, void* stream, int* launches);

/* ---- vertical interpolation to run-time levels (NEW entry, additive: the ABI version stays 8; no reference counterpart -- gt4py leaves
 * output on pressure, height or isentropic levels and the vertical half of a semi-Lagrangian step to user stencils: a `while` loop, a
 * carried run-time K index and reads at a run-time K index, one field per call, the search and the weights repeated for every field)
 * Writes to dst[n], at each of the `nd` target levels of every column (i, j) of the box, the POINT value of src[n] at the coordinate
 * that dst_coord holds for that level, src[n] given at the `ns` source levels whose coordinates src_coord holds, for `nfields` pairs
 * that share ONE pair of coordinate fields, in ONE kernel launch per 8 pairs, on `stream`, without synchronisation or allocation.  The
 * box is [origin, origin + extent_ij) in I and J of every field; along K a src and src_coord hold `ns` levels from their origin, a dst
 * and dst_coord `nd`.  `elem_size` (fields) and `coord_elem_size` (coordinate fields) are 4 (float32) or 8 (float64) and need not
 * match.  A coordinate field may have byte stride 0 along I and / or J: a Field[K] of fixed levels broadcasts without a copy and is
 * exempt from the shape check on that axis.  A src stride of 0 broadcasts too; a dst stride of 0 on an extent above 1 is
 * GT4MI_ERR_INVALID_ARGUMENT.  Source coordinates are meant to increase strictly with k (negate a coordinate that decreases); target
 * coordinates may come in ANY order (departure heights are not monotone).  Interpolation that is linear in ln p takes ln p as the
 * coordinate: the kernel computes no logarithm.
 * THE ARITHMETIC IS PART OF THE CONTRACT (csrc/vertical_interp.hip.h states it again, tests/vertical_interp_ref.py restates it in plain
 * Python and in numpy).  All of it is float64, one IEEE rounding per operation, no FMA; float32 items and coordinates are widened
 * exactly on load and the result is rounded once on store.  Per column: coordinates z[0..ns-1], targets x[0..nd-1], values q[0..ns-1]
 * of each field.  A bracket index k starts at 0 and is carried from one target of the column to the next, in the order m = 0, 1, ...,
 * nd-1.  For a target x:
 *   1. hunt:    while k < ns-2 and z[k+1] <= x: k += 1;  then  while k > 0 and z[k] > x: k -= 1.  k changes nowhere else.
 *   2. outside: below = x < z[0], above = x > z[ns-1].  With `outside` =
 *        GT4MI_VINTERP_OUTSIDE_FILL    store fill_value -- the double rounded once to the item type, a NaN as the canonical quiet NaN
 *                                      (0x7FC00000 / 0x7FF8000000000000) -- and go to the next target
 *        GT4MI_VINTERP_OUTSIDE_CLAMP   x = z[0] (below) or x = z[ns-1] (above) before step 3: the end level's value
 *        GT4MI_VINTERP_OUTSIDE_LINEAR  x stays, and step 3 uses the linear formula whatever the method: the end interval's line,
 *                                      extended; GT4MI_VINTERP_NEAREST moves item 0 (below) or item ns-1 (above)
 *   3. inside, with h = z[k+1] - z[k] and t = (x - z[k]) / h (one IEEE division):
 *        GT4MI_VINTERP_NEAREST         the ITEM q[k+1] if t >= 0.5, else q[k]: the bit pattern is moved (a NaN payload survives); if x is
 *                                      NaN the canonical quiet NaN is stored
 *        GT4MI_VINTERP_LINEAR          out = (1.0 - t) * q[k] + t * q[k+1], both products rounded before the addition; a weight of zero
 *                                      still multiplies (0 * inf = NaN on a source level next to an infinity)
 *        GT4MI_VINTERP_CUBIC           if k < 1 or k > ns-3 (the end intervals, and every interval when ns < 4) the linear formula;
 *                                      otherwise Lagrange on the four nodes z0..z3 = z[k-1..k+2] with q0..q3 = q[k-1..k+2]:
 *                                      w_a = (product of (x - z_b) for b != a, left to right in b) / (product of (z_a - z_b) for b != a,
 *                                      left to right in b), one division per weight, e.g. w1 = (((x - z0) * (x - z2)) * (x - z3)) /
 *                                      (((z1 - z0) * (z1 - z2)) * (z1 - z3));  out = ((w0*q0 + w1*q1) + w2*q2) + w3*q3
 *        GT4MI_VINTERP_CUBIC_MONOTONE  the cubic out, then -- only where the cubic formula was used -- out = mn if out < mn else (mx if
 *                                      out > mx else out), mn = min(q[k], q[k+1]), mx = max(q[k], q[k+1]), min(a, b) = b if b < a else
 *                                      a, max(a, b) = b if b > a else a; a NaN out stays NaN
 *   4. the bracket, t and the weights of a target are computed ONCE for all fields of the call.
 * Path independence: for strictly increasing z and a non-NaN x, step 1 ends at the largest k <= ns-2 with z[k] <= x, or at 0 when there
 * is none, wherever it started; a target's bits therefore depend on neither the other targets of the column nor their order, and not
 * on layout, strides, alignment, position in the call, number of fields in the call, Field[K] versus an IJK coordinate field with the
 * same items, or device.  The loops end whatever the data holds: the first only increments k below ns-2, the second only decrements it
 * above 0, so a target costs at most ns-2 steps each way and the target loop counts to nd; a NaN x leaves k where it was and yields NaN
 * through the arithmetic; NaN, repeated or non-monotone z change which comparisons hold (and give that column whatever IEEE arithmetic
 * gives), never the bounds, and affect no other column.  Every K index of a load is k-1 ... k+2 within 0 ... ns-1 by those integers, 0
 * or ns-1; every K index of a store is m < nd: no address depends on the data.
 * Refusals: null pointers, nfields < 1, ns < 2 (one level has nothing to interpolate between), nd < 1, an extent out of range, an
 * unknown method, outside value or flag (GT4MI_ERR_INVALID_ARGUMENT); an item size other than 4 or 8, a misaligned or wrongly strided
 * field (GT4MI_ERR_UNSUPPORTED); a box that does not fit its field (GT4MI_ERR_OUT_OF_BOUNDS); a dst stride of 0 on an extent above 1
 * (GT4MI_ERR_INVALID_ARGUMENT: only a src or a coordinate field may be broadcast); the bytes of a dst box (first to last item) meeting
 * those of any src box, of a coordinate field or of another dst box (GT4MI_ERR_UNSUPPORTED, the rule of gt4mi_field_copy).  No byte
 * outside the dst boxes changes.  An extent with a zero entry is GT4MI_OK, nothing enqueued.  Every check runs before the first launch;
 * a refused call enqueues nothing.  With GT4MI_VINTERP_DRY_RUN the checks run, *launches is set and no device is touched.  *launches
 * (may be NULL) = the kernels the call enqueues: ceil(nfields / 8). */
enum { GT4MI_VINTERP_NEAREST = 0, GT4MI_VINTERP_LINEAR = 1, GT4MI_VINTERP_CUBIC = 2, GT4MI_VINTERP_CUBIC_MONOTONE = 3 };
enum { GT4MI_VINTERP_OUTSIDE_CLAMP = 0, GT4MI_VINTERP_OUTSIDE_LINEAR = 1, GT4MI_VINTERP_OUTSIDE_FILL = 2 };
enum { GT4MI_VINTERP_DRY_RUN = 256 };
int gt4mi_vertical_interp(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* src_coord,
                          const gt4mi_field* dst_coord, const int64_t extent_ij[2], int64_t ns, int64_t nd, int elem_size,
                          int coord_elem_size, int method, int outside, double fill_value, int flags, void* stream, int* launches);

/* ---- horizontal interpolation at run-time positions (NEW entry, additive: the ABI version stays 8; no reference counterpart -- GTScript
 * takes compile-time horizontal offsets only, and gt4py leaves a gather at data-dependent I / J positions (semi-Lagrangian departure
 * points, sampling on a rotated, shifted or nested grid) to fancy indexing on its numpy / cupy storages) --------------------------------
 * For every point (i, j, k) of the box [origin, origin + extent) of every dst[n] -- the compute domain -- writes the value of src[n] at
 * level k and the horizontal position (x_i, x_j) that pos_i / pos_j hold for that point, for `nfields` pairs that share ONE pair of
 * position fields, in ONE kernel launch per 8 pairs, on `stream`, without synchronisation or allocation.  `elem_size` (fields) and
 * `pos_elem_size` (position fields) are 4 (float32) or 8 (float64) and need not match.  A position field may have byte stride 0 along K:
 * a Field[IJ] shared by every level broadcasts without a copy and is exempt from the shape check on that axis.
 * Positions are in index units of the compute domain: 0.0 is domain point 0 (the origin of src[n]).  With GT4MI_INTERP_RELATIVE they are
 * displacements: x = double(index) + p (what a stencil can produce: it has no I or J as a value).  The readable box of a src is the
 * domain grown by `reach` = {lo_i, hi_i, lo_j, hi_j} ghost cells; it must fit the array (origin - lo >= 0, origin + extent + hi <= shape).
 * THE ARITHMETIC IS PART OF THE CONTRACT (csrc/horizontal_interp.hip.h states it again, tests/horizontal_interp_ref.py restates it in
 * plain Python).  All of it is float64, one IEEE rounding per operation, no FMA; float32 items and positions are widened exactly on load
 * and the result is rounded once on store.  Per axis, with n domain points, xmin = -lo and xmax = n - 1 + hi as doubles:
 *   1. p = the position item; in relative mode p = double(index) + p
 *   2. x = xmin if p < xmin else (xmax if p > xmax else p): NaN passes through, +-inf clamps
 *   3. b = xmin if x != x else (int64) floor(x), t = x - double(b) (x is finite or NaN, the conversion is always defined)
 *   4. every index a method uses is clamped on its own to [xmin, xmax]: edge replication; b-1, b, b+1, b+2 for the cubics and b, b+1 for
 *      linear are each clamped separately.  No address depends on the data beyond these integers.
 *   GT4MI_INTERP_NEAREST         the index is floor(x + 0.5), clamped; the source item's bit pattern is moved (a NaN payload survives);
 *                                a NaN position stores the canonical quiet NaN (0x7FC00000 / 0x7FF8000000000000)
 *   GT4MI_INTERP_LINEAR          w0 = 1 - t, w1 = t per axis; at row b_j  r0 = w0i*v00 + w1i*v10, at row b_j + 1  r1 likewise;
 *                                out = w0j*r0 + w1j*r1, each product rounded before its addition
 *   GT4MI_INTERP_CUBIC           Lagrange on the nodes -1, 0, 1, 2; with a = t + 1, c = t - 1, d = t - 2:
 *                                w_-1 = -(((t*c)*d) / 6.0), w_0 = ((a*c)*d) / 2.0, w_1 = -(((a*t)*d) / 2.0), w_2 = ((a*t)*c) / 6.0;
 *                                the four row values r = ((w_-1*v_-1 + w_0*v_0) + w_1*v_1) + w_2*v_2 along I, the same expression
 *                                along J over the four r gives out
 *   GT4MI_INTERP_CUBIC_MONOTONE  the cubic out, then out = mn if out < mn else (mx if out > mx else out), mn = min(min(c00, c10),
 *                                min(c01, c11)) and mx likewise over the four corner items at the clamped indices b, b+1 of each axis,
 *                                min(a, b) = b if b < a else a, max(a, b) = b if b > a else a; a NaN out stays NaN
 * Consequences: a weight of zero still multiplies (0 * inf = NaN at an integer position next to an infinity); -0.0 may come back as
 * +0.0; a NaN position gives NaN in every field of that point and touches nothing else; the bits of a point do not depend on layout,
 * strides, alignment, position in the call, number of fields in the call, Field[IJ] versus an IJK position field with the same items,
 * or device.  Periodic wrap is not part of the kernel: fill the ghost cells with gt4mi_halo_fill first.
 * Refusals: null pointers, nfields < 1, an unknown method or flag, a negative reach (GT4MI_ERR_INVALID_ARGUMENT); an item size other
 * than 4 or 8, a misaligned field (GT4MI_ERR_UNSUPPORTED); a box that does not fit its field (GT4MI_ERR_OUT_OF_BOUNDS); the bytes of a
 * dst box (first to last item) meeting those of any src readable box, of a position field or of another dst box (GT4MI_ERR_UNSUPPORTED,
 * the rule of gt4mi_field_copy); a dst stride of 0 on an extent above 1 (GT4MI_ERR_INVALID_ARGUMENT).  No byte outside the dst boxes
 * changes.  An extent with a zero entry is GT4MI_OK, nothing enqueued.  Every check runs before the first launch; a refused call
 * enqueues nothing.  With GT4MI_INTERP_DRY_RUN the checks run, *launches is set and no device is touched.  *launches (may be NULL) =
 * the kernels the call enqueues: ceil(nfields / 8). */
enum { GT4MI_INTERP_NEAREST = 0, GT4MI_INTERP_LINEAR = 1, GT4MI_INTERP_CUBIC = 2, GT4MI_INTERP_CUBIC_MONOTONE = 3 };
enum { GT4MI_INTERP_RELATIVE = 1, GT4MI_INTERP_DRY_RUN = 256 };
int gt4mi_horizontal_interp(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* pos_i,
                            const gt4mi_field* pos_j, const int64_t extent[3], const int64_t reach[4], int elem_size,
                            int pos_elem_size, int method, int flags, void* stream, int* launches);

/* ---- 3-d departure-point interpolation (NEW entry, additive: the ABI version stays 8; no reference counterpart -- GTScript takes
 * compile-time horizontal offsets only, and gt4mi_horizontal_interp followed by gt4mi_vertical_interp is not this: the vertical entry
 * reads the column at (i, j), not the one at the horizontal departure position) ---------------------------------------------------
 * For every point (i, j, k) of the box [origin, origin + extent) of every dst[n] -- the compute domain -- writes the value of src[n] at
 * the position (x_i, x_j, x_k) that pos_i / pos_j / pos_k hold for that point, for `nfields` pairs that share ONE triple of position
 * fields, in ONE kernel launch per 8 pairs, on `stream`, without synchronisation or allocation.  `elem_size` (fields) and
 * `pos_elem_size` (position fields) are 4 (float32) or 8 (float64) and need not match.  pos_i and pos_j may have byte stride 0 along K
 * (a Field[IJ] shared by every level, exempt from the shape check on that axis); pos_k is a full IJK box.
 * All three positions are in index units of the compute domain: 0.0 is domain point 0 along I and J and level 0 along K.  With
 * GT4MI_INTERP_RELATIVE they are displacements on each of the three axes: x = double(own index) + p.  The readable box of a src is the
 * domain grown by `reach` = {lo_i, hi_i, lo_j, hi_j} ghost cells along I and J, over all levels 0 ... extent[2] - 1: K has no ghost levels.
 * THE ARITHMETIC IS PART OF THE CONTRACT (csrc/departure_interp.hip.h states it again, tests/departure_interp_ref.py restates it in
 * plain Python).  All of it is float64, one IEEE rounding per operation, no FMA; float32 items and positions are widened exactly on load
 * and the result is rounded once on store.
 *   Axes I and J   steps 1-4 of gt4mi_horizontal_interp unchanged: clamp to [-lo, n - 1 + hi], floor, t, every index clamped on its own.
 *   Axis K         the same four steps with lo = hi = 0: x_k is clamped to [0, nk - 1], b_k = floor(x_k) (0 for a NaN), t_k = x_k - b_k.
 *   Plane value    for a level kk, P(kk) is exactly gt4mi_horizontal_interp's `out` for that level before any limiter: the rows are
 *                  combined along I, then the same expression is applied along J.
 *   GT4MI_INTERP_NEAREST         the level index is floor(x_k + 0.5), clamped; the bit pattern of the item at the three nearest indices is
 *                                moved (a NaN payload survives); a NaN in any of the three positions stores the canonical quiet NaN
 *   GT4MI_INTERP_LINEAR          levels b_k and b_k + 1, each clamped; out = w0k*P(b_k) + w1k*P(b_k+1) with w0k = 1 - t_k, w1k = t_k
 *   GT4MI_INTERP_CUBIC           the rule of gt4mi_vertical_interp, not edge replication in K: where 1 <= b_k <= nk-3,
 *                                out = ((w_-1*P(b_k-1) + w_0*P(b_k)) + w_1*P(b_k+1)) + w_2*P(b_k+2) with the Lagrange weights of t_k (those
 *                                of gt4mi_horizontal_interp); otherwise (b_k < 1 or b_k > nk-3: the end intervals, and every interval
 *                                when nk < 4) the linear formula along K over the two CUBIC plane values P(b_k) and P(b_k+1), and only
 *                                those two planes are loaded.  nk = 1, 2 and 3 need no special case.
 *   GT4MI_INTERP_CUBIC_MONOTONE  the cubic out, then out = mn if out < mn else (mx if out > mx else out), at every point (the end
 *                                intervals of K included), with mn = min(min(min(c000, c100), min(c010, c110)), min(min(c001, c101),
 *                                min(c011, c111))) over the eight corner items at the clamped indices b, b+1 of the three axes, index
 *                                order (i, j, k), mx folded the same way; min(a, b) = b if b < a else a, max(a, b) = b if b > a else a;
 *                                a NaN out stays NaN
 * Consequences: a weight of zero still multiplies (0 * inf = NaN at an integer position next to an infinity); -0.0 may come back as
 * +0.0; a NaN position makes every field of that point NaN and touches nothing else; no address depends on data beyond the clamped
 * integers; the bits of a point do not depend on layout, strides, alignment, position in the call, number of fields in the call, or
 * Field[IJ] versus IJK position fields holding the same items.  Periodic wrap is not part of the kernel: fill the ghost cells with
 * gt4mi_halo_fill first.  A physical vertical coordinate is not either: convert it to a fractional level first.
 * Refusals: null pointers, nfields < 1, an unknown method or flag, a negative reach (GT4MI_ERR_INVALID_ARGUMENT); an item size other
 * than 4 or 8, a misaligned field (GT4MI_ERR_UNSUPPORTED); a box that does not fit its field (GT4MI_ERR_OUT_OF_BOUNDS); the bytes of a
 * dst box (first to last item) meeting those of any src readable box, of a position field or of another dst box (GT4MI_ERR_UNSUPPORTED);
 * a dst stride of 0 on an extent above 1 (GT4MI_ERR_INVALID_ARGUMENT).  No byte outside the dst boxes changes.  An extent with a zero
 * entry is GT4MI_OK, nothing enqueued.  Every check runs before the first launch; a refused call enqueues nothing.  With
 * GT4MI_INTERP_DRY_RUN the checks run, *launches is set and no device is touched.  *launches (may be NULL) = the kernels the call
 * enqueues: ceil(nfields / 8).  Methods and flags are those of gt4mi_horizontal_interp. */
int gt4mi_departure_interp(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* pos_i,
                           const gt4mi_field* pos_j, const gt4mi_field* pos_k, const int64_t extent[3], const int64_t reach[4],
                           int elem_size, int pos_elem_size, int method, int flags, void* stream, int* launches);

/* ---- sampling at a list of run-time positions (NEW entry, additive: the ABI version stays 8; no reference counterpart -- GTScript takes
 * compile-time horizontal offsets only and writes fields of the shape it reads: a station's sounding, a cross-section along a path or
 * the values along a track have another shape than the fields, and gt4py leaves them to fancy indexing on its numpy / cupy storages) ---
 * Samples `nfields` fields at `npoints` positions that ONE set of position arrays holds, in ONE kernel launch per 8 fields, on `stream`,
 * without synchronisation or allocation.  `extent` is the compute domain (ni, nj, nk) of every src[n], `reach` = {lo_i, hi_i, lo_j, hi_j}
 * the ghost cells a gather may read as for gt4mi_horizontal_interp: the readable box of a src is the domain grown by the reach along I
 * and J, over all levels; it must fit the array.
 * Column mode (pos_k == NULL): for every point p < npoints and every level k < extent[2], dst[n] at (p, k) is the value of src[n] at
 * level k and the horizontal position (pos_i[p], pos_j[p]): a sounding per point, a curtain per path.  THE ARITHMETIC IS THAT OF
 * gt4mi_horizontal_interp in absolute mode, all of it: steps 1-4 per axis, the four methods GT4MI_INTERP_NEAREST / LINEAR / CUBIC /
 * CUBIC_MONOTONE, the canonical quiet NaN at a NaN position for nearest, bit patterns moved for nearest.
 * Point mode (pos_k != NULL): dst[n] at p is the value of src[n] at the 3-d position (pos_i[p], pos_j[p], pos_k[p]), by THE ARITHMETIC
 * OF gt4mi_departure_interp in absolute mode, its K rule included: K has no ghost levels (pos_k is clamped to [0, nk - 1]) and the
 * cubics use the linear formula over the two cubic plane values in the end intervals.  A physical vertical coordinate is not a level:
 * convert it with gt4mi_vertical_interp first.  (csrc/point_sample.hip.h calls the device functions of the two interpolators, it
 * restates nothing; tests/point_sample_ref.py restates the contract through tests/horizontal_interp_ref.py and
 * tests/departure_interp_ref.py.)
 * A dst[n] is a gt4mi_field whose axis 0 is the point and axis 1 the level: its box is (npoints, extent[2], 1) in column mode and
 * (npoints, 1, 1) in point mode, any strides.  pos_i / pos_j / pos_k are 1-d: axis 0 is the point, the box is (npoints, 1, 1); their
 * items are `pos_elem_size` 4 (float32) or 8 (float64) whatever `elem_size` (the fields', 4 or 8) is.  Positions are in index units of
 * the compute domain: 0.0 is domain point 0 (the origin of src[n]) and level 0.  They are read at LAUNCH time, not at call time: a
 * caller may rewrite the arrays between two calls with the same arguments (a moving platform, a trajectory).
 * Flags: GT4MI_SAMPLE_FILL -- a point is FILLED if any of its position items satisfies p < xmin, p > xmax or p != p, with xmin = -lo and
 * xmax = n - 1 + hi as doubles along I and J and, in point mode, xmin = 0 and xmax = nk - 1 along K (a point exactly at xmin or xmax is
 * not filled, +-inf is); a filled point receives `fill_value`, rounded once to the item type, in every field and every level; every
 * other point receives exactly the bits it receives without the flag.  Without the flag the behaviour is the interpolators': positions
 * are clamped to the readable box and a NaN position gives NaN.  GT4MI_SAMPLE_DRY_RUN -- the checks run, *launches is set and no device
 * is touched.
 * Consequences: a weight of zero still multiplies (0 * inf = NaN at an integer position next to an infinity); -0.0 may come back as
 * +0.0; no address depends on data beyond the clamped integers (a filled point reads at its clamped position and drops what it read);
 * the bits of a sample do not depend on layout, strides or alignment, on the number of fields in the call or its position among
 * them, on the number or order of the points, or on the device; they are the bits gt4mi_horizontal_interp (column mode) or
 * gt4mi_departure_interp (point mode) writes for a point with the same position items.  Periodic wrap is not part of the kernel: fill
 * the ghost cells with gt4mi_halo_fill first.
 * Refusals: null pointers (pos_k excepted), nfields < 1, npoints < 0, an unknown method or flag, a negative reach
 * (GT4MI_ERR_INVALID_ARGUMENT); an item size other than 4 or 8, a misaligned field (GT4MI_ERR_UNSUPPORTED); a box that does not fit
 * its field -- for a src the readable box -- (GT4MI_ERR_OUT_OF_BOUNDS); the bytes of a dst box (first to last item) meeting those of any
 * src readable box, of a position array or of another dst box (GT4MI_ERR_UNSUPPORTED); a dst stride of 0 on an extent above 1
 * (GT4MI_ERR_INVALID_ARGUMENT).  No byte outside the dst boxes changes.  npoints == 0 or an extent with a zero entry is GT4MI_OK,
 * nothing enqueued.  Every check runs before the first launch; a refused call enqueues nothing.  *launches (may be NULL) = the kernels
 * the call enqueues: ceil(nfields / 8).  Methods are those of gt4mi_horizontal_interp. */
enum { GT4MI_SAMPLE_FILL = 2, GT4MI_SAMPLE_DRY_RUN = 256 };
int gt4mi_point_sample(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* pos_i, const gt4mi_field* pos_j,
                       const gt4mi_field* pos_k, int64_t npoints, const int64_t extent[3], const int64_t reach[4], int elem_size,
                       int pos_elem_size, int method, int flags, double fill_value, void* stream, int* launches);

/* ---- conservative horizontal remapping between rectilinear grids (NEW entries, additive: the ABI version stays 8; no reference
 * counterpart -- a GTScript destination point (i, j) reads sources at compile-time constant offsets from (i, j) only: not 2*i, not a
 * run-time range of source cells, not a source field of another horizontal shape) ---------------------------------------------------
 * Takes cell MEANS of `nfields` fields on one rectilinear horizontal grid to cell means on another (coarser, finer or shifted), level
 * by level.  Each of the I and J axes has ns + 1 source edges and nd + 1 destination edges; a 2-d overlap is the product of two 1-d
 * overlaps, so all geometry is two small per-axis tables, computed ONCE on the host by gt4mi_overlap_table and applied to every level of
 * up to 8 fields per launch by gt4mi_horizontal_remap.
 *
 * gt4mi_overlap_table (pure host code, no GPU): src_edges[0..ns], dst_edges[0..nd] are HOST float64 arrays, finite and strictly
 * increasing; the table goes to the caller's HOST arrays ptr[nd + 1], cell / w / h / c / den[capacity]; capacity >= ns + nd - 1 is
 * always enough; *nnz receives the number of terms.  h, c, den may all three be NULL (a table for GT4MI_HREMAP_PCM only).
 * THE ARITHMETIC IS PART OF THE CONTRACT and is gt4mi_vertical_remap's, per axis (tests/horizontal_remap_ref.py restates it in plain
 * Python): float64, one IEEE rounding per operation, no FMA.  With xs = src_edges, xd = dst_edges: the first source cell extends to
 * -inf and the last to +inf (edge replication: a destination cell that reaches outside the source range sees the end cell's mean there,
 * the weights of a destination cell still sum to 1, nothing is extrapolated).  A source index k is kept across the destination cells
 * and never decreases.  For destination cell m, lo = xd[m], hi = xd[m+1], d = hi - lo:
 *   1. advance: while k < ns-1 and not (xs[k+1] > lo): k += 1
 *   2. for each overlapping k, in increasing order, one TERM:
 *        l = lo if k == 0    else max(lo, xs[k])     (max(a, b) = b if b > a else a)
 *        r = hi if k == ns-1 else min(hi, xs[k+1])   (min(a, b) = b if b < a else a)
 *        cell = k,  w = (r - l) / d
 *        h = xs[k+1] - xs[k],  xl = (l - xs[k]) / h,  xr = (r - xs[k]) / h,  c = 0.5 * (xl + xr) - 0.5
 *        den = 0.5 * h[k-1] + h[k] + 0.5 * h[k+1] (left to right), 1.0 in the two end cells (k == 0 or k == ns-1)
 *        stop after the term for which k == ns-1 or xs[k+1] >= hi, otherwise k += 1
 *   ptr[m] .. ptr[m+1] are the terms of destination cell m (ptr[0] = 0, ptr[nd] = *nnz); nd <= *nnz <= ns + nd - 1; with identical grids
 *   every cell has one term with w exactly 1.0.
 * Refusals of gt4mi_overlap_table, each with a message: a null pointer (h, c, den: only some of the three), ns < 1 or nd < 1, edges that
 * are not finite and strictly increasing (GT4MI_ERR_INVALID_ARGUMENT); a capacity that is too small (GT4MI_ERR_OUT_OF_BOUNDS). */
typedef struct gt4mi_overlap_axis {
    int32_t ns, nd, nnz;  /* source cells, destination cells, terms                            */
    const int32_t* ptr;   /* nd + 1: the terms of destination cell m are ptr[m] .. ptr[m+1]    */
    const int32_t* cell;  /* nnz: the source cell k of a term                                  */
    const double* w;      /* nnz: its weight                                                   */
    const double* h;      /* nnz: the thickness of source cell k       (GT4MI_HREMAP_PLM only) */
    const double* c;      /* nnz: where the overlap's centre lies in it (GT4MI_HREMAP_PLM only) */
    const double* den;    /* nnz: the centred difference's denominator (GT4MI_HREMAP_PLM only) */
} gt4mi_overlap_axis;
int gt4mi_overlap_table(const double* src_edges, int ns, const double* dst_edges, int nd, int32_t* ptr, int32_t* cell, double* w,
                        double* h, double* c, double* den, int capacity, int* nnz);

/* gt4mi_horizontal_remap: the table pointers of axis_i / axis_j are DEVICE pointers (the two structs themselves are host memory).  The
 * dst box is (axis_i->nd, axis_j->nd, nk) from the origin of each dst[n], the src box (axis_i->ns, axis_j->ns, nk) from the origin of
 * each src[n]; ONE kernel launch per 8 pairs, on `stream`, without synchronisation or allocation.  `elem_size` is 4 (float32) or 8
 * (float64); any strides and any two layouts; a src stride of 0 broadcasts; a dst stride of 0 on an extent above 1 is
 * GT4MI_ERR_INVALID_ARGUMENT.
 * THE VALUES ARE PART OF THE CONTRACT (csrc/horizontal_remap.hip.h states them again).  Everything is float64, items are widened exactly
 * on load, the result is rounded once on store, each product is rounded before its addition.  For a destination point the outer loop
 * runs over the J terms b in table order, the inner loop over the I terms a in table order; q[a, b] is the item of the level at source
 * cell (cell_i[a], cell_j[b]):
 *   GT4MI_HREMAP_PCM   row_b = sum_a wi_a * q[a, b];  out = sum_b wj_b * row_b.  The first term of each sum IS the accumulator, so with
 *                      identical grids q comes back bit for bit, -0.0 included.
 *   GT4MI_HREMAP_PLM   the same two sums over v = (q[a, b] + si * ci_a) + sj * cj_b, with si / sj the limited centred slopes of source
 *                      cell (a, b) along I / J, formula and order of gt4mi_vertical_remap: with q-, q+ the neighbours along the axis,
 *                      dl = q - q-, dr = q+ - q: if dl * dr > 0 then g = (q+ - q-) / den * h and the slope is
 *                      copysign(min(|g|, 2|dl|, 2|dr|), g) (min(a, b) = b if b < a else a, in this order), otherwise 0.  The slope is 0
 *                      when the cell is the first or last of that axis of the source BOX: nothing outside the box is ever read.
 *                      The limiter acts per axis: plm is conservative and reproduces fields linear in x and y away from the end cells,
 *                      but it is not strictly monotone in 2-d (the two corrections add up at a corner of the overlap).
 * Both methods conserve the integral over the grid when the outer edges of the two grids coincide.  The bits of a point do not depend
 * on layout, strides, position in the call or number of fields in the call.
 * SAFETY: the only data that reaches an address are table integers.  The kernel clamps each ptr value to [0, nnz], takes a
 * non-increasing pair as zero terms, and clamps every cell and cell +- 1 to the source box: a corrupt table gives unspecified values,
 * never an address outside the boxes the host has checked.  No loop bound depends on field data.
 * Refusals: null pointers (h, c, den may be NULL for GT4MI_HREMAP_PCM), nfields < 1, nk < 1, ns < 1 or nd < 1, an unknown method or
 * flag, nnz outside [nd, ns + nd - 1] (GT4MI_ERR_INVALID_ARGUMENT); an item size other than 4 or 8, a misaligned field or table array
 * (GT4MI_ERR_UNSUPPORTED); a box that does not fit its field (GT4MI_ERR_OUT_OF_BOUNDS); the bytes of a dst box (first to last item)
 * meeting those of any src box, of another dst box or of any table array (GT4MI_ERR_UNSUPPORTED, the rule of gt4mi_field_copy).  No byte
 * outside the dst boxes changes.  Every check runs before the first launch; a refused call enqueues nothing.  With
 * GT4MI_HREMAP_DRY_RUN the checks run, *launches is set and no device is touched.  *launches (may be NULL) = the kernels the call
 * enqueues: ceil(nfields / 8). */
enum { GT4MI_HREMAP_PCM = 0, GT4MI_HREMAP_PLM = 1 };
enum { GT4MI_HREMAP_DRY_RUN = 256 };
int gt4mi_horizontal_remap(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_overlap_axis* axis_i,
                           const gt4mi_overlap_axis* axis_j, int64_t nk, int elem_size, int method, int flags, void* stream,
                           int* launches);

/* ---- tridiagonal line solves along I, J or K (NEW entry, additive: the ABI version stays 8; the reference has one Thomas solve, the
 * K-only `tridiagonal_solver` stencil behind gt4mi_tridiag_*, which takes one right-hand side, rewrites its coefficients and has no
 * periodic closure; GTScript cannot write a recurrence along I or J) ------------------------------------------------------------------
 * For every line along `axis` (0 = I, 1 = J, 2 = K) of the box [origin, origin + extent) solves
 *   a[m] x[m-1] + b[m] x[m] + c[m] x[m+1] = d[m],  m = 0 .. n-1,  n = extent[axis],
 * with a = lower, b = diag, c = upper, d = rhs[k], x = out[k], for `nfields` (out, rhs) pairs that share ONE set of coefficients, in
 * ONE kernel launch per 8 pairs, on `stream`, without synchronisation or allocation; the elimination factors of a line are formed
 * once for all its right-hand sides.  `elem_size` is 4 (float32) or 8 (float64) and is the item size of EVERY field.  The
 * coefficients are never written.  A coefficient may have byte stride 0 along the two axes other than `axis`: a 1-d array of n
 * items that every line shares broadcasts without a copy and is exempt from the shape check on those axes.  A rhs stride of 0
 * broadcasts too; an out stride of 0 on an extent above 1 is GT4MI_ERR_INVALID_ARGUMENT.
 * out[k] may BE rhs[k] -- the same first item and the same strides: an in-place solve.  Every other meeting of the bytes of an out box
 * (first to last item) with a rhs box, another out box or a coefficient, and of any field with the workspace, is refused.
 * THE ARITHMETIC IS PART OF THE CONTRACT (csrc/line_solve.hip.h states it again, tests/line_solve_ref.py restates it in plain Python).
 * All of it is in the fields' type, one IEEE rounding per operation, no FMA; division is IEEE division, there is no reciprocal.
 * Without GT4MI_LINE_PERIODIC (a[0] and c[n-1] are never read):
 *   m = 0 :  cp[0] = c[0] / b[0]                     dp[0] = d[0] / b[0]
 *   m >= 1:  den = b[m] - a[m] * cp[m-1]
 *            cp[m] = c[m] / den   (not for m = n-1)  dp[m] = (d[m] - a[m] * dp[m-1]) / den
 *   x[n-1] = dp[n-1] ;  x[m] = dp[m] - cp[m] * x[m+1]   for m = n-2 .. 0
 * which is the arithmetic of gt4mi_tridiag_*: one right-hand side gives the bits of that solve on the permuted data.
 * With GT4MI_LINE_PERIODIC the line is closed: a[0] couples point 0 to point n-1, c[n-1] couples point n-1 to point 0; n >= 3.
 * Sherman-Morrison with alpha = c[n-1], beta = a[0], gamma = -b[0]:
 *   bb[0] = b[0] - gamma ;  bb[n-1] = b[n-1] - (alpha * beta) / gamma ;  bb[m] = b[m] otherwise
 *   q = the solution of the non-periodic system with diagonal bb and right-hand side (gamma, 0, ..., 0, alpha)   [once per line]
 *   y = the solution of the same system with right-hand side d                                                   [per field]
 *   fact = (y[0] + (beta * y[n-1]) / gamma) / ((1 + q[0]) + (beta * q[n-1]) / gamma)
 *   x[m] = y[m] - fact * q[m]
 * The elimination of the periodic system reads c[n-1] only as alpha, cp[n-1] is not formed; the zeros of q's right-hand side take
 * part as written (0 - a[m] * qp[m-1]).  No pivoting.  Every loop counts to n; no loop bound and no address depends on field data: a
 * zero or NaN pivot gives its line what IEEE arithmetic gives and changes nothing in any other line.
 * `workspace` holds the elimination factors (and q): its layout is private to the library, its size depends on extent, axis,
 * elem_size and flags and is reported in *workspace_needed (may be NULL); it is aligned to 8 bytes; the result never depends on what
 * it held before the call.  No byte outside the out boxes and the workspace is written.
 * *path (may be NULL) = which kernel the strides of the call select: GT4MI_LINE_PATH_LANES (an axis other than `axis` has unit stride
 * in every field: lanes along it, every step a coalesced row), GT4MI_LINE_PATH_TILES (`axis` itself has unit stride in every field: a
 * lane owns a line, tiles of 64 lines x 128 bytes go through LDS), GT4MI_LINE_PATH_ITEMS (anything else: one lane per line, item by
 * item, correct and slow).  The bits do not depend on the path.
 * Refusals: null pointers, nfields < 1, an invalid extent or axis, an unknown flag, a periodic line of fewer than 3 points, a
 * workspace that is too small (GT4MI_ERR_INVALID_ARGUMENT); an item size other than 4 or 8, a misaligned field or workspace, a
 * forbidden overlap (GT4MI_ERR_UNSUPPORTED); a box that does not fit its field (GT4MI_ERR_OUT_OF_BOUNDS).  An extent with a zero
 * entry is GT4MI_OK, nothing enqueued.  Every check runs before the first launch; a refused call enqueues nothing.  With
 * GT4MI_LINE_DRY_RUN the checks run, *workspace_needed, *path and *launches are set and no device is touched; `workspace` may then
 * be NULL (a workspace that is passed is checked).  *launches (may be NULL) = the kernels the call enqueues: ceil(nfields / 8). */
enum { GT4MI_LINE_PATH_LANES = 0, GT4MI_LINE_PATH_TILES = 1, GT4MI_LINE_PATH_ITEMS = 2 };
enum { GT4MI_LINE_PERIODIC = 1, GT4MI_LINE_DRY_RUN = 256 };
int gt4mi_line_solve(const gt4mi_field* out, const gt4mi_field* rhs, int nfields, const gt4mi_field* lower, const gt4mi_field* diag,
                     const gt4mi_field* upper, const int64_t extent[3], int axis, int elem_size, int flags, void* workspace,
                     int64_t workspace_bytes, void* stream, int64_t* workspace_needed, int* path, int* launches);

/* ---- prefix scans along I, J or K (NEW entry, additive: the ABI version stays 8; the reference has no scan: its users slice a storage and
 * call numpy / cupy `cumsum` or `maximum.accumulate` on the slice -- one call and one fresh array per field, the order of the float
 * additions whatever the library picks -- or write a FORWARD / BACKWARD stencil, which exists along K only and takes one field) ----------
 * For every line along `axis` (0 = I, 1 = J, 2 = K) of the box [origin, origin + extent) and each of `nfields` (dst, src) pairs, dst gets
 * the running sum, maximum or minimum (`op`) of src along the line, at every point of it, in ONE kernel launch per 8 pairs, on `stream`,
 * without synchronisation, allocation or workspace.  `elem_size` is 4 (float32) or 8 (float64) and is the item size of EVERY field.
 * `weight` (may be NULL; GT4MI_SCAN_SUM only) holds the terms' factors -- the grid spacing of an integral -- and is never written; it
 * may have byte stride 0 along the two axes other than `axis`: a 1-d array of n items that every line shares broadcasts without a copy
 * and is exempt from the shape check on those axes.  A src stride of 0 broadcasts too; a dst stride of 0 on an extent above 1 is
 * GT4MI_ERR_INVALID_ARGUMENT.
 * dst[k] may BE src[k] -- the same first item and the same strides: an in-place scan.  Every other meeting of the bytes of a dst box (first
 * to last item) with a src box, another dst box or the weight is refused.
 * THE ARITHMETIC IS PART OF THE CONTRACT (csrc/line_scan.hip.h states it again, tests/line_scan_ref.py restates it in plain Python and in
 * numpy).  T is the fields' type; A is double where GT4MI_SCAN_WIDE is set, op is GT4MI_SCAN_SUM and T is float, else T (GT4MI_SCAN_WIDE
 * has no effect on float64 fields or on MAX and MIN).  x[0 .. n), n = extent[axis], is the line in scan order: from the low end, with
 * GT4MI_SCAN_REVERSE from the far end (the BACKWARD sweep); w is the weight in the same order.
 *   SUM  t[m] = A(x[m]), or A(x[m]) * A(w[m]) with one rounding in A
 *        s[0] = t[0]   (NOT 0 + t[0]: a leading -0.0 stays -0.0, as in numpy.cumsum)
 *        s[m] = s[m-1] + t[m]   one rounding in A, no FMA, strictly sequential
 *   MAX  s[0] = x[0] ;  s[m] = s[m-1] if (s[m-1] != s[m-1] or s[m-1] > x[m]) else x[m]
 *        a NaN, once met, stays; on a tie (signed zeros included) the newer item is taken; it is a select: bit patterns (NaN payloads)
 *        are moved, not computed.  Not fmax / fmin, which drop NaNs.
 *   MIN  the same with <.
 *   dst[m] = T(s[m]) ;  with GT4MI_SCAN_EXCLUSIVE dst[0] = the identity (+0.0 for SUM, -inf for MAX, +inf for MIN) and dst[m] = T(s[m-1])
 * dst is written at the item's own index, also in a reverse scan.  The float sum is numpy.cumsum along that axis bit for bit, with
 * GT4MI_SCAN_WIDE numpy.cumsum(x, dtype=float64).astype(float32).  The order is sequential because lines are plentiful: parallelism comes
 * across lines; a box of few, long lines is served correctly and not fast (a segmented parallel scan, whose order of additions would
 * depend on the length, is out of scope).  Every loop counts to n; no loop bound and no address depends on field data: a NaN or an inf
 * reaches the rest of its line as written above and no other line.  No byte outside the dst boxes is written.
 * *path (may be NULL) = which kernel the strides of the call select, by the rule of gt4mi_line_solve: GT4MI_SCAN_PATH_LANES (an axis
 * other than `axis` has unit stride in every field: lanes along it, every step a coalesced row), GT4MI_SCAN_PATH_TILES (`axis` itself has
 * unit stride in every field: a lane owns a line, tiles of 64 lines x 128 bytes go through LDS), GT4MI_SCAN_PATH_ITEMS (anything else:
 * one lane per line, item by item, correct and slow).  The bits do not depend on the path.
 * Refusals: null pointers, nfields < 1, an invalid extent, axis or op, an unknown flag, a weight with MAX or MIN
 * (GT4MI_ERR_INVALID_ARGUMENT); an item size other than 4 or 8, a misaligned field, a forbidden overlap (GT4MI_ERR_UNSUPPORTED); a box
 * that does not fit its field (GT4MI_ERR_OUT_OF_BOUNDS).  An extent with a zero entry is GT4MI_OK, nothing enqueued.  Every check runs
 * before the first launch; a refused call enqueues nothing.  With GT4MI_SCAN_DRY_RUN the checks run, *path and *launches are set and no
 * device is touched.  *launches (may be NULL) = the kernels the call enqueues: ceil(nfields / 8). */
enum { GT4MI_SCAN_SUM = 0, GT4MI_SCAN_MAX = 1, GT4MI_SCAN_MIN = 2 };
enum { GT4MI_SCAN_PATH_LANES = 0, GT4MI_SCAN_PATH_TILES = 1, GT4MI_SCAN_PATH_ITEMS = 2 };
enum { GT4MI_SCAN_EXCLUSIVE = 1, GT4MI_SCAN_REVERSE = 2, GT4MI_SCAN_WIDE = 4, GT4MI_SCAN_DRY_RUN = 256 };
int gt4mi_line_scan(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* weight, const int64_t extent[3], int axis,
                    int elem_size, int op, int flags, void* stream, int* path, int* launches);

/* ---- first-crossing and extremum search along I, J or K (NEW entry, additive: the ABI version stays 8; the reference has no search: its
 * users write a FORWARD stencil with a carried flag -- one field per call, along K only -- or chain cupy passes: a compare, `argmax` of the
 * mask, two gathers and the arithmetic, each with fresh arrays) --------------------------------------------------------------------------
 * For every line along `axis` (0 = I, 1 = J, 2 = K) of the box [origin, origin + extent) and each of `nfields` fields, finds WHERE on the
 * line something happens (`what`): where the line first crosses level[k] (GT4MI_FIND_CROSSING), or where its maximum / minimum lies
 * (GT4MI_FIND_ARGMAX / GT4MI_FIND_ARGMIN), in ONE kernel launch per 8 fields, on `stream`, without synchronisation, allocation or
 * workspace.  `elem_size` is 4 (float32) or 8 (float64) and is the item size of EVERY field and of the coord.  No field is written.
 * `coord` (may be NULL) is the coordinate along the line (a height); it may have byte stride 0 along the two axes other than `axis`: a 1-d
 * array of n items that every line shares broadcasts without a copy and is exempt from the shape check on those axes.  A field stride of
 * 0 on an extent above 1 is GT4MI_ERR_INVALID_ARGUMENT.  `level` (GT4MI_FIND_CROSSING only, NULL otherwise) points to `nfields` doubles in
 * HOST memory, read during the call and passed to the kernels by value; `missing` is what a line without a crossing gets.
 * `result` holds nfields x 3 x nB x nA doubles, result[((k * 3 + row) * nB + b) * nA + a], A < B the two axes other than `axis` (the layout
 * of gt4mi_line_stats): row GT4MI_FIND_POSITION, GT4MI_FIND_COORD, GT4MI_FIND_EXTRA (the value at an extremum, the number of crossings of
 * a line).  It is aligned to 8 bytes and meets no field and not the coord.  No byte outside it is written.
 * THE CONTRACT (csrc/line_find.hip.h states it again, tests/line_find_ref.py restates it in plain Python and in numpy).  All comparisons and
 * arithmetic are IEEE float64 on the items converted exactly, one rounding per operation, no FMA.  n = extent[axis]; y[q] = x[q], with
 * GT4MI_FIND_REVERSE x[n-1-q]: the line in scan order; zc[q] the coord's item at the same place; idx(q) = q, reverse n-1-q: positions stay
 * in the forward index units of the box.
 *   ARGMAX    the candidate starts as item 0; item q replaces it if the candidate is not a NaN and (y[q] is a NaN or y[q] > candidate).  So
 *             the first NaN met wins and stays, the first of equal items stays (-0.0 == +0.0): numpy.argmax of y.  ARGMIN: the same with <.
 *             position = double(idx(q*)) ;  coord = zc[q*], without a coord = position ;  value = double(y[q*]) (a NaN is a NaN; its
 *             payload is not part of the contract)
 *   CROSSING  pair q in [0, n-1) rises through L if y[q] < L && y[q+1] >= L and falls if y[q] > L && y[q+1] <= L; `direction` selects
 *             GT4MI_FIND_RISING, GT4MI_FIND_FALLING or either (GT4MI_FIND_ANY), in scan order.  y[0] == L counts as found at q = 0 with
 *             t = 0 for every direction: position = double(idx(0)), coord = zc[0].  A comparison with a NaN is false: a NaN item makes no
 *             crossing, a NaN level finds nothing.  crossings = the number of selected pairs on the whole line, plus one if y[0] == L.
 *             At the first found pair:  t = (L - y[q]) / (y[q+1] - y[q])   (the denominator is not zero by the condition)
 *               position = double(q) + t, reverse double(n-1-q) - t ;  coord = zc[q] + t * (zc[q+1] - zc[q]), without a coord = position
 *             A line with none: position = coord = missing, crossings = 0.  n = 1 has no pair: only y[0] == L finds something.
 * Every loop counts to n, there is no early exit; no loop bound and no address depends on field data.  A line's three items depend on
 * that line alone: not on layout, axis, path, the other fields of the call or the device.
 * *path (may be NULL) = which kernel the strides of the call select, by the rule of gt4mi_line_solve with every field strict and the coord
 * loose: GT4MI_LINE_PATH_LANES, GT4MI_LINE_PATH_TILES or GT4MI_LINE_PATH_ITEMS.  The result does not depend on the path.
 * Refusals: null pointers, nfields < 1, an invalid extent, axis, `what` or `direction`, an unknown flag, a level or a direction with an
 * extremum, no level with a crossing, a result that is null, misaligned or meets a field or the coord (GT4MI_ERR_INVALID_ARGUMENT); an item
 * size other than 4 or 8, a misaligned field, more lines than one launch counts (GT4MI_ERR_UNSUPPORTED); a box that does not fit its field
 * (GT4MI_ERR_OUT_OF_BOUNDS).  An extent with a zero entry is GT4MI_OK, nothing enqueued.  Every check runs before the first launch; a
 * refused call enqueues nothing.  With GT4MI_FIND_DRY_RUN the checks run, *path and *launches are set and no device is touched; `result`
 * may then be NULL (a result that is passed is checked).  *launches (may be NULL) = the kernels the call enqueues: ceil(nfields / 8). */
enum { GT4MI_FIND_CROSSING = 0, GT4MI_FIND_ARGMAX = 1, GT4MI_FIND_ARGMIN = 2 };
enum { GT4MI_FIND_ANY = 0, GT4MI_FIND_RISING = 1, GT4MI_FIND_FALLING = 2 };
enum { GT4MI_FIND_POSITION = 0, GT4MI_FIND_COORD = 1, GT4MI_FIND_EXTRA = 2, GT4MI_FIND_ROWS = 3 };
enum { GT4MI_FIND_REVERSE = 1, GT4MI_FIND_DRY_RUN = 256 };
int gt4mi_line_find(const gt4mi_field* fields, int nfields, const gt4mi_field* coord, const int64_t extent[3], int axis, int elem_size,
                    int what, int direction, const double* level, double missing, double* result, int flags, void* stream, int* path,
                    int* launches);

/* ---- histograms of fields, whole box or per level (NEW entry, additive: the ABI version stays 8; the reference has no reduction and no
 * result of another shape than its fields: its users call numpy / cupy `histogram`, or `searchsorted` + `bincount` per field and level, on
 * storages that ARE numpy / cupy arrays) ------------------------------------------------------------------------------------------------
 * Counts how the items of the box [origin, origin + extent) of each of `nfields` fields (1 .. GT4MI_HISTOGRAM_MAX_FIELDS) are distributed
 * over `nbins` bins (1 .. GT4MI_HISTOGRAM_MAX_BINS) in ONE pass and ONE kernel launch, on `stream`, without synchronisation, allocation or
 * workspace.  `elem_size` is 4 (float32) or 8 (float64) and is the item size of EVERY field.  No field is written; a field stride of 0 on an
 * extent above 1 is GT4MI_ERR_INVALID_ARGUMENT.  `by` = GT4MI_HISTOGRAM_WHOLE: one row of counters per field for the whole box;
 * GT4MI_HISTOGRAM_BY_K: one row per level k of the box (nrows = extent[2]).
 * `edges` is a DEVICE pointer to float64 edges: nbins + 1 that every field shares, or with GT4MI_HISTOGRAM_EDGES_PER_FIELD nfields sets of
 * nbins + 1.  `edges_host` points to the same values in HOST memory; the dry run, and only the dry run, reads it and checks the edges:
 * finite and strictly increasing.  A call without the dry-run flag reads neither pointer on the host.
 * `result` holds nfields x nrows x (nbins + 3) int64 counters, result[(k * nrows + row) * (nbins + 3) + slot]: the bins, then
 * GT4MI_HISTOGRAM_BELOW, GT4MI_HISTOGRAM_ABOVE and GT4MI_HISTOGRAM_NAN at nbins + 0, 1, 2.  It is aligned to 8 bytes and meets no field and
 * not the edges.  No byte outside it is written.  Without GT4MI_HISTOGRAM_ACCUMULATE it is zeroed first, in stream order, by a
 * small kernel on `stream` (not a hipMemsetAsync: replays of a captured call were seen to leave other words than zero with it,
 * for a reason that was not found); with the flag the counts are ADDED to what it holds (a run-long PDF: one call per step into
 * one result).
 * THE CONTRACT (csrc/field_histogram.hip.h states it again, tests/histogram_ref.py restates it in plain Python and in numpy).  Every item x
 * of a row's box is converted exactly to float64 and lands in exactly one counter of the row:
 *   nan      if x != x
 *   below    if x < e[0]          (-inf included)
 *   above    if x > e[nbins]      (+inf included)
 *   bin nbins - 1 if x == e[nbins]: the last bin is closed, as in numpy.histogram
 *   else the bin b with e[b] <= x < e[b+1]; -0.0 == 0.0 as IEEE compares them
 * For finite items in range the bins are numpy.histogram(x.astype(float64), bins=e)[0] bit for bit.  The counters of a row sum to the items
 * of its box; items outside the box (pads, ghost cells) are never read.  The counters are integers, so the result is exact and the same bits
 * for any layout, path, launch shape, device or decomposition: the sum of the histograms of the parts of a box IS the histogram of the box.
 * The count depends on the edges alone: the kernel guesses the bin with one multiply, accepts the guess only if the comparisons against e[]
 * hold and bisects otherwise; every search loop is bounded by a constant, so any content of the edges buffer terminates.
 * *path (may be NULL) = GT4MI_HISTOGRAM_PATH_ROWS if every field has unit item stride along an axis of a row's box that is longer than 1 (it
 * is walked in 16-byte lanes where the other strides allow), GT4MI_HISTOGRAM_PATH_ITEMS if any field goes item by item (per level a
 * K-contiguous field does: a level holds no line of it).  The result does not depend on the path.
 * GT4MI_HISTOGRAM_MAX_BINS is what the kernels' LDS plan carries: the float64 edges and one uint32 counter per slot of 4096 bins are 49 184
 * bytes per workgroup (padded to 16), three workgroups per CU (csrc/field_histogram.hip.h).  A box holds at most 2^31 - 1 items, so that no on-chip
 * counter can wrap.
 * NOT OFFERED: weighted histograms (float sums would need a fixed order), rows along I or J, two-dimensional (joint) histograms, edges
 * changed after the dry run has checked them.
 * Refusals: null pointers, nfields outside 1 .. 8, nbins outside 1 .. GT4MI_HISTOGRAM_MAX_BINS, an invalid or empty extent, an invalid `by`,
 * an unknown flag, edges that are not finite or not strictly increasing (the message names the first offending index), edges or a result
 * that are misaligned, a result that meets a field or the edges (GT4MI_ERR_INVALID_ARGUMENT); an item size other than 4 or 8, a misaligned
 * field, more than 2^31 - 1 items or 2^24 levels (GT4MI_ERR_UNSUPPORTED); a box that does not fit its field (GT4MI_ERR_OUT_OF_BOUNDS).
 * Every check runs before anything is enqueued.  With GT4MI_HISTOGRAM_DRY_RUN the checks run (those of the edges among them), *path and
 * *launches are set and no device is touched; `edges` and `result` may then be NULL (what is passed is checked).  *launches (may be NULL) =
 * the counting kernels the call enqueues: 1 (the zeroing is not counted). */
enum { GT4MI_HISTOGRAM_MAX_FIELDS = 8, GT4MI_HISTOGRAM_MAX_BINS = 4096, GT4MI_HISTOGRAM_EXTRA = 3 };
enum { GT4MI_HISTOGRAM_BELOW = 0, GT4MI_HISTOGRAM_ABOVE = 1, GT4MI_HISTOGRAM_NAN = 2 };
enum { GT4MI_HISTOGRAM_WHOLE = 0, GT4MI_HISTOGRAM_BY_K = 1 };
enum { GT4MI_HISTOGRAM_PATH_ROWS = 0, GT4MI_HISTOGRAM_PATH_ITEMS = 1 };
enum { GT4MI_HISTOGRAM_ACCUMULATE = 1, GT4MI_HISTOGRAM_EDGES_PER_FIELD = 2, GT4MI_HISTOGRAM_DRY_RUN = 256 };
int gt4mi_field_histogram(const gt4mi_field* fields, int nfields, const int64_t extent[3], int elem_size, int nbins, const double* edges,
                          const double* edges_host, int by, int64_t* result, int flags, void* stream, int* path, int* launches);

/* ---- Fourier filtering along periodic lines of I, J or K (NEW entry, additive: the ABI version stays 8; the reference has nothing in
 * wavenumber space: a stencil reads its neighbours at compile-time offsets, a Fourier coefficient reads the whole line.  Its users leave
 * for an FFT library: rfft, a multiply and irfft per field -- three launches and more, complex intermediates of the field's size, the
 * order of the arithmetic whatever the library picks) ---------------------------------------------------------------------------------
 * Every line along `axis` (0 = I, 1 = J, 2 = K) of the box [origin, origin + extent) is taken as periodic of length n = extent[axis], a
 * power of two with 2 <= n <= 4096; nh = n / 2 + 1.  ONE kernel launch per 8 fields, on `stream`, without synchronisation, allocation
 * or workspace.  `elem_size` is 4 (float32) or 8 (float64) and is the item size of EVERY field.  A, B are the two axes other than `axis`
 * in IJK order, nA, nB the box's extents along them.
 * `mode` = GT4MI_FILTER_APPLY: for each of `nfields` (dst, src) pairs the line of src is transformed, wavenumber m is multiplied by the real
 * response[m] and the line is transformed back into dst.  `response` is a DEVICE pointer to response_extent[0] x response_extent[1] x nh
 * float64, C-ordered; response_extent[0] is 1 or nA, response_extent[1] is 1 or nB: an extent of 1 broadcasts ({1, 1}: one response for
 * every line; {nj, 1} on axis I: the polar filter, one response per latitude).  It is read when the kernel runs, never written, and its
 * values are not checked.  dst[k] may BE src[k] -- the same first item and the same strides: in place.  Every other meeting of the
 * bytes of a dst box with a src box, another dst box, the response or the twiddles is refused.  `result` is NULL.
 * `mode` = GT4MI_FILTER_SPECTRUM: the forward transform of each of the `nfields` fields `src` alone.  `dst`, `response` and `response_extent`
 * are NULL.  `result` holds nfields x 2 x nA x nB x nh float64, result[(((k * 2 + part) * nA + a) * nB + b) * nh + m], part 0 the real and
 * part 1 the imaginary part of wavenumber m = 0 .. n/2: the same shape on every path.  It is aligned to 8 bytes and meets no field and
 * not the twiddles.  No byte outside it is written.
 * `twiddles` is a DEVICE pointer to n float64 that the CALLER has computed: wr[j] = cos(2 pi j / n) at [j] and wi[j] = -sin(2 pi j / n)
 * at [n/2 + j] for j < n/2, with w[0] = (1, 0) and w[n/4] = (0, -1) set exactly.  The device never evaluates a sine or a cosine.
 * THE ARITHMETIC IS PART OF THE CONTRACT (csrc/line_filter.hip.h states it again, tests/line_filter_ref.py restates it in plain Python and
 * in numpy).  All of it is IEEE float64 on the items converted exactly, one rounding per operation, no FMA; one rounding to the fields'
 * type on the store.  L = log2 n; x[p] = (item p of the line, +0.0).
 *   FORWARD   radix-2 decimation in frequency, natural order in, bit-reversed order out.  For h = n/2, n/4, .. 1, for every block start
 *             (a multiple of 2h) and j < h:  p = start + j, q = p + h, w = w[j * n / (2h)], a = x[p], b = x[q]:
 *               u = a - b ;  a' = a + b ;  b'.re = wr * u.re - wi * u.im ;  b'.im = wr * u.im + wi * u.re
 *   MULTIPLY  in place: the slot at p holds wavenumber m = bitrev_L(p); both parts are multiplied by response[min(m, n - m)].
 *   INVERSE   radix-2 decimation in time, bit-reversed order in, natural order out, with conj(w).  For h = 1, 2, .. n/2, p, q, w, a, b
 *             as above:  t.re = wr * b.re + wi * b.im ;  t.im = wr * b.im - wi * b.re ;  a' = a + t ;  b' = a - t
 *             dst[p] = T(x[p].re * (1.0 / n)), the factor exact; the imaginary part is dropped.  No permutation is executed.
 *   SPECTRUM  after FORWARD the slot at p is stored at m = bitrev_L(p) where m <= n/2.
 * A kernel may fuse stages in registers only where every bit of the result stays the same, signed zeros included: the shipped one fuses
 * up to three and leaves out nothing, no trivial twiddle and no zero imaginary part (1 * x - 0 * y is not x for every x and y).  A
 * line's result depends on that line, its response row and n alone: not on layout, axis, path, the other fields and lines of the call or
 * the device; a NaN or an infinity stays in its line.  Every loop bound and every address follows from n, the extents and the strides.
 * *path (may be NULL) = which way the strides of the call select for the loads and stores, by the rule of gt4mi_line_solve with every
 * field strict and the response loose (it counts as unit along `axis` and allows another axis only where it is broadcast along it):
 * GT4MI_LINE_PATH_TILES (`axis` has unit stride in every field: lanes along the line, 16 bytes each where every line is aligned so),
 * GT4MI_LINE_PATH_LANES (another axis has: a workgroup takes neighbouring lines along it, a load covers runs along that axis),
 * GT4MI_LINE_PATH_ITEMS (anything else: item by item, correct and slow).  The bits do not depend on the path.
 * NOT OFFERED: lengths that are not a power of two (mixed radix), lengths above 4096 (one line is all a workgroup's 64 KiB hold), a
 * complex response, a line that is split over ranks.
 * Refusals: null pointers, nfields < 1, an invalid extent, axis or mode, an unknown flag, a dst, response or result with the wrong mode,
 * a response extent that is neither 1 nor the box's, a response, twiddles or result that is misaligned, a result that meets a field or
 * the twiddles (GT4MI_ERR_INVALID_ARGUMENT); an item size other than 4 or 8, a line length that is not a power of two from 2 to 4096
 * (the message names it), a misaligned field, a forbidden overlap, more lines than one launch counts (GT4MI_ERR_UNSUPPORTED); a box that
 * does not fit its field (GT4MI_ERR_OUT_OF_BOUNDS).  An extent with a zero entry along another axis is GT4MI_OK, nothing enqueued.  Every
 * check runs before the first launch; a refused call enqueues nothing.  With GT4MI_FILTER_DRY_RUN the checks run, *path and *launches are
 * set and no device is touched; `response`, `twiddles` and `result` may then be NULL (what is passed is checked).  *launches (may be
 * NULL) = the kernels the call enqueues: ceil(nfields / 8). */
enum { GT4MI_FILTER_APPLY = 0, GT4MI_FILTER_SPECTRUM = 1 };
enum { GT4MI_FILTER_DRY_RUN = 256 };
int gt4mi_line_filter(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const double* response, const int64_t* response_extent,
                      const double* twiddles, double* result, const int64_t extent[3], int axis, int elem_size, int mode, int flags,
                      void* stream, int* path, int* launches);

/* ---- multi-GPU: RCCL halo exchange driven from native code (NEW, no reference counterpart) --------
 * One process per GPU.  gt4mi_comm wraps an RCCL communicator created from a 128-byte unique id
 * (gt4mi_comm_unique_id on one rank, distributed by the host program, e.g. torch.distributed).
 * A gt4mi_halo_plan holds, for one field shape, the boxes to send/receive in the (up to) two phases of the
 * exchange and owns the dense device staging buffers.  Two message tables are in use (the host builds them):
 *   two-phase     phase 0: I faces, phase 1: J faces including the I-halo columns (corners for free, 4 neighbours,
 *                 two dependent rounds of pack -> send/recv -> unpack);
 *   single-phase  everything in phase 0: 4 faces + 4 corner boxes to up to 8 neighbours, ONE round -- half the
 *                 latency; on a fully connected xGMI node the diagonal neighbours have links of their own.
 * Within a phase the k-th send to a peer pairs with the k-th receive that peer posts from this rank (RCCL
 * point-to-point ordering); at most 8 boxes per phase and direction. */
typedef struct gt4mi_comm gt4mi_comm;
typedef struct gt4mi_halo_plan gt4mi_halo_plan;

typedef struct gt4mi_halo_msg {
    int32_t peer;      /* rank of the neighbour                                                  */
    int32_t phase;     /* 0 or 1                                                                  */
    int64_t lo[3];     /* box start, in indices of the field array (NOT relative to the origin)  */
    int64_t extent[3]; /* box size                                                                */
} gt4mi_halo_msg;

int gt4mi_comm_unique_id(void* id128);
int gt4mi_comm_create(const void* id128, int nranks, int rank, gt4mi_comm** comm);
/* A communicator WITHOUT RCCL behind it (ranks that RCCL cannot join: two processes on one device; or no librccl at all):
 * plans created on it move their messages through the direct transport only (gt4mi_halo_plan_direct_*). */
int gt4mi_comm_create_local(int nranks, int rank, gt4mi_comm** comm);
int gt4mi_comm_destroy(gt4mi_comm* comm);
/* What RCCL reports for the communicator (ncclCommCount, ncclCommUserRank, ncclCommCuDevice); any pointer may be NULL.
 * Lets a benchmark line state how many ranks RCCL really joined. */
int gt4mi_comm_info(gt4mi_comm* comm, int* nranks, int* rank, int* device);
int gt4mi_halo_plan_create(gt4mi_comm* comm, int elem_size, const gt4mi_halo_msg* sends, int nsends,
                           const gt4mi_halo_msg* recvs, int nrecvs, gt4mi_halo_plan** plan);
int gt4mi_halo_plan_destroy(gt4mi_halo_plan* plan);
/* How the fused distributed steps (gt4mi_dist_*) built on this plan are scheduled; value -1 = the entry point's default.
 *   GT4MI_PLAN_SCHEDULE             GT4MI_SCHEDULE_JOIN:  main: pack, interior, [join], ring;  side: send/recv, unpack
 *                                   GT4MI_SCHEDULE_CHAIN: main: interior only;  side: pack, send/recv, unpack, ring -- no
 *                                   cross-stream wait on the critical path as long as the chain fits under the interior
 *                                   GT4MI_SCHEDULE_SWAP (gt4mi_dist_lap5_f64 and gt4mi_dist_hdiff_*): main: pack, send/recv, unpack,
 *                                   ring back to back;  side: the interior kernel; the caller's stream joins the interior at
 *                                   the end -- for shares so small that the chain, not the interior, is the critical path
 *                                   GT4MI_SCHEDULE_SWAP_PACKED: the same, the interior kernel forking off AFTER the pack (the
 *                                   pack of strided I faces runs alone, the send/recv kernel starts ahead of the interior)
 *                                   GT4MI_SCHEDULE_INLINE: everything on the caller's stream, no event: pack, interior, the rest
 *                                   of the exchange, ring -- made for the direct transport, whose pack kernel IS the transfer:
 *                                   the faces travel while the interior kernel runs and the unpack finds them there
 *   GT4MI_PLAN_INTERIOR_WG_PER_CU   at most this many workgroups of the INTERIOR kernel per CU while the exchange runs
 *                                   next to it (0 = no limit): an HBM-saturating kernel at full occupancy keeps tens of MB
 *                                   in flight and the send/recv kernel beside it waits ~10 us per memory access
 *   GT4MI_PLAN_DEFER_JOIN           1 (chain schedule only): gt4mi_dist_hdiff_* / gt4mi_dist_lap5_f64 return WITHOUT making
 *                                   the caller's stream wait for the side stream's chain; the caller joins with
 *                                   gt4mi_halo_exchange_end before anything consumes the result.  For INDEPENDENT applies:
 *                                   the interior of the next apply runs next to the exchange and ring of this one.
 *   GT4MI_PLAN_EDGE_COLUMNS         gt4mi_dist_hdiff_* / gt4mi_dist_lap5_f64: width of the W / E boxes left to the ring kernel
 *                                   (even; default 16, 8 for local domains narrower than 256 columns; the Laplacian's at most
 *                                   16): what the ring computes is taken off the interior kernel, a box of whole cache lines
 *                                   costs the memory system less than the 1 - 2 columns the stencil's reach requires, and the
 *                                   interior kernel keeps its 16-byte alignment.  gt4mi_dist_lap5_*: effective ONLY where
 *                                   gt4mi_dist_lap5_query reports edge_units = 0 -- where the edge units of csrc/lap5_edge.hip.h
 *                                   run (one receiving round, I-contiguous 16-byte aligned rows) the W / E boxes are exactly one
 *                                   16-byte lane wide on every schedule and transport, whatever this option says
 * Which combination is fastest depends on the links; bench.py measures them (config.calibration_ms_per_apply).
 *   GT4MI_PLAN_DIRECT_TIMEOUT_MS    direct transport: how long a device-side wait for a neighbour may take (milliseconds; 0 = the
 *                                   default: GT4MI_DIRECT_TIMEOUT_MS of the environment, else 30 000) before the plan FAILS, see below
 *   GT4MI_PLAN_DIRECT_FENCED        direct transport, 0 (default) / 1: FENCED MODE.  By default a pushed face is ordered before its
 *                                   flag by write-through stores + their acknowledgement, and the receiver's loads behind its flag
 *                                   load by issue order and cache-bypassing loads -- no fence, because a system-scope release next
 *                                   to an HBM-saturating interior kernel is expensive.  With 1 the pushing side
 *                                   does a system-scope RELEASE fence before it raises the flag and the receiving side a system-scope
 *                                   ACQUIRE fence behind its flag load: the ISA's own message-passing recipe, for links on which
 *                                   the default's assumptions have not been verified.  Both sides of a message must agree only
 *                                   in that each may be fenced or not independently (the modes interoperate); bench.py steps
 *                                   direct -> direct-fenced -> RCCL when its epoch-stamped self-check fails. */
enum { GT4MI_PLAN_SCHEDULE = 0, GT4MI_PLAN_INTERIOR_WG_PER_CU = 1, GT4MI_PLAN_DEFER_JOIN = 2, GT4MI_PLAN_EDGE_COLUMNS = 3,
       GT4MI_PLAN_TRANSPORT = 4, GT4MI_PLAN_DIRECT_TIMEOUT_MS = 5, GT4MI_PLAN_DIRECT_FENCED = 6 };
enum { GT4MI_TRANSPORT_RCCL = 0, GT4MI_TRANSPORT_DIRECT = 1 };
enum { GT4MI_SCHEDULE_JOIN = 0, GT4MI_SCHEDULE_CHAIN = 1, GT4MI_SCHEDULE_SWAP = 2, GT4MI_SCHEDULE_SWAP_PACKED = 3,
       GT4MI_SCHEDULE_INLINE = 4 };
int gt4mi_halo_plan_set_option(gt4mi_halo_plan* plan, int option, int value);
/* The DIRECT transport (GT4MI_PLAN_TRANSPORT = GT4MI_TRANSPORT_DIRECT; csrc/direct.hip.h): the pack kernel stores every face
 * straight into the neighbour's receive buffer (mapped with hipIpcOpenMemHandle; the neighbour may be this rank itself, another
 * process on this device, or another device of the node) and raises a flag there; the neighbour's unpack kernel waits for its
 * flags.  No send/recv kernel, two launches per phase.  Set-up, once per plan, by the host side that knows who the peers are:
 *   1. _direct_prepare on every rank: moves the plan's receive buffers into one exportable pool of fine-grained device memory
 *      (its first page holds the flag words) and fills `info` -- plain bytes to hand to the peers over any channel;
 *   2. _direct_layout: where receive (phase, index) sits in this rank's pool and which flag belongs to a message -- for the peers;
 *   3. _direct_connect for every message: sends[phase][index] lands at `peer_pool_offset` of the peer's pool and raises the peer's
 *      flag `peer_flag_index` (is_send = 1); after unpacking recvs[phase][index] this rank raises the SENDER's flag
 *      `peer_flag_index` (is_send = 0).  The k-th send to a peer pairs with the k-th receive that peer posted for this rank (RCCL's
 *      matching rule); `peer` = NULL: this rank itself;
 *   4. gt4mi_halo_plan_set_option(plan, GT4MI_PLAN_TRANSPORT, GT4MI_TRANSPORT_DIRECT) after every rank has connected.
 * FAILURE IS HARD: a device-side wait that runs out of time (GT4MI_PLAN_DIRECT_TIMEOUT_MS) copies and signals nothing and sets
 * the plan's error word (host memory the device writes); the NEXT call on the plan that touches the exchange -- gt4mi_halo_exchange*,
 * gt4mi_dist_*, gt4mi_halo_exchange_end -- reads it without synchronising and returns GT4MI_ERR_TIMEOUT, and so does every call
 * after it.  The call that enqueued the failing exchange has returned GT4MI_OK long before (everything is asynchronous): check
 * the status of the call that CONSUMES the result (_end, the next step, or _direct_status) before trusting ghost cells.
 * _direct_status synchronises the device first: whether a wait of any exchange started so far ran out of time.
 * DESTROYING a prepared plan is collective in effect: the neighbours' kernels write into this plan's pool ("consumed" adds, the
 * next pushes); call gt4mi_halo_plan_destroy only after every rank has finished its last exchange ON THE DEVICE (each rank
 * synchronises, then the ranks meet once on the host's control channel; gt4py_amd/distributed/native.py close()). */
typedef struct gt4mi_direct_info {
    char pool_handle[64];  /* hipIpcMemHandle_t of the pool: a page of flag words, then the receive buffers */
    int64_t pool_bytes, flag_words;
    int32_t pid, device;
} gt4mi_direct_info;
int gt4mi_halo_plan_direct_prepare(gt4mi_halo_plan* plan, gt4mi_direct_info* info);
int gt4mi_halo_plan_direct_layout(gt4mi_halo_plan* plan, int phase, int is_send, int index, int64_t* pool_offset, int* flag_index);
int gt4mi_halo_plan_direct_connect(gt4mi_halo_plan* plan, int phase, int is_send, int index, const gt4mi_direct_info* peer,
                                   int64_t peer_pool_offset, int peer_flag_index);
int gt4mi_halo_plan_direct_status(gt4mi_halo_plan* plan, int* timed_out, unsigned* exchanges);
/* 1 = the plan's side stream was verified to run concurrently with the caller's stream, 0 = no
 * concurrent stream could be found (the exchange still works, serialised), 2 = not probed yet.
 * HIP multiplexes streams onto a few hardware queues; the overlapped entry points probe on first use
 * and replace a side stream that shares the caller's queue. */
int gt4mi_halo_plan_concurrent(gt4mi_halo_plan* plan);
/* Enqueue the whole exchange of `field` on `stream` (stream-ordered, returns immediately). */
int gt4mi_halo_exchange(gt4mi_halo_plan* plan, const gt4mi_field* field, void* stream);
/* Overlapped form: _begin makes the plan's side stream wait for `main_stream`, enqueues the exchange
 * there and records completion; _end makes `main_stream` wait for that completion.  Work enqueued on
 * `main_stream` between the two calls (the interior kernel) runs concurrently with the exchange. */
int gt4mi_halo_exchange_begin(gt4mi_halo_plan* plan, const gt4mi_field* field, void* main_stream);
/* Optional: mark the fork point on `main_stream` NOW and enqueue the exchange later.  Lets the
 * caller enqueue the interior kernel before _begin, so the GPU is already busy while the host is
 * still issuing the pack / RCCL / unpack sequence; the next _begin then waits only for work that
 * was on `main_stream` before the fork. */
int gt4mi_halo_exchange_fork(gt4mi_halo_plan* plan, void* main_stream);
int gt4mi_halo_exchange_end(gt4mi_halo_plan* plan, void* main_stream);
/* One distributed apply of a 5-point stencil in a single call: exchange of `inp`'s halo (width 1)
 * overlapped with the interior kernel, then the boundary strips.  `sides` = bit mask of the sides
 * that have a neighbour: 1 = low I (W), 2 = high I (E), 4 = low J (S), 8 = high J (N).  Schedule (GT4MI_PLAN_SCHEDULE):
 * default GT4MI_SCHEDULE_SWAP (GT4MI_SCHEDULE_INLINE on the direct transport); whatever the schedule, work enqueued on `main_stream` after the call sees the whole result
 * (unless GT4MI_PLAN_DEFER_JOIN says otherwise).  Where the plan receives in ONE round (a single-phase table, or a grid cut along one
 * axis) and the fields are I-contiguous with 16-byte aligned rows, the unpack and the boundary strips are one kernel of units that read
 * the receive buffers themselves, and on the direct transport's GT4MI_SCHEDULE_INLINE the whole apply is ONE launch (csrc/lap5_edge.hip.h).
 * After the call `inp` has its ghost cells, as after gt4mi_halo_exchange. */
int gt4mi_dist_lap5_f64(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* inp,
                        const gt4mi_field* out, int variant, int sides, void* main_stream);
/* Which launches gt4mi_dist_lap5_* would make for these arguments (nothing is enqueued): *edge_units = 1 when the unpack and the
 * boundary strips are the edge units of csrc/lap5_edge.hip.h (and, on the direct transport's GT4MI_SCHEDULE_INLINE, the whole apply
 * ONE launch), 0 when they are separate unpack and ring launches (two receiving rounds, a width that is no multiple of the 16-byte
 * lane, a layout without unit I stride ...).  The plan's item size selects float64 / float32. */
int gt4mi_dist_lap5_query(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* out, int sides,
                          int* edge_units);
/* The same for float32 fields (a plan created for 4-byte items); `flags` as for gt4mi_lap5_f32 (GT4MI_LAP_LITERAL_F32). */
int gt4mi_dist_lap5_f32(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* inp,
                        const gt4mi_field* out, int variant, int flags, int sides, void* main_stream);

/* One distributed apply of horizontal diffusion (the stencil of gt4mi_hdiff_*; BASELINE configs[4]) in a single call:
 *   main stream: pack of in_field's faces -> interior kernel (the domain minus a ring 2 points deep on every side
 *                that has a neighbour) ................................. join -> ring kernel (one launch, four boxes)
 *   side stream:                             RCCL send/recv -> unpack (-> second phase of a two-phase plan)
 * The plan must exchange faces 2 deep and include the corner cells (either message table above).  `sides` as above. */
int gt4mi_dist_hdiff_f64(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* in_field,
                         const gt4mi_field* out_field, const gt4mi_field* coeff, double coeff_scalar, int flags, int sides,
                         void* main_stream);
int gt4mi_dist_hdiff_f32(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* in_field,
                         const gt4mi_field* out_field, const gt4mi_field* coeff, double coeff_scalar, int flags, int sides,
                         void* main_stream);

/* Time-stepping form (out of step n is inp of step n+1): each call
 *   1. joins the exchange that delivered `inp`'s ghost cells (started by the previous call, or once by
 *      gt4mi_halo_exchange_begin(plan, first_input, ...) before the first step),
 *   2. computes the boundary strips of `out`,
 *   3. starts the exchange of `out`'s ghost cells on the plan's side stream,
 *   4. computes the interior of `out` concurrently with that exchange.
 * Nothing on the main stream ever waits for an exchange that has not had a whole interior kernel to
 * complete.  After the last step `out`'s ghost cells are (being) refreshed; gt4mi_halo_exchange_end
 * joins. */
int gt4mi_dist_lap5_f64_pipelined(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* inp,
                                  const gt4mi_field* out, int variant, int sides, void* main_stream);
/* Communication-avoiding generalisation: the fields carry ghost regions `halo` >= 1 cells deep (the
 * plan exchanges faces that deep) and ONE exchange serves `halo` consecutive steps.  Call with
 * phase = 0, 1, ..., halo-1, 0, 1, ... :
 *   phase 0            joins the exchange that delivered `inp`'s ghost cells;
 *   phase < halo-1     one launch over the compute domain grown by (halo-1-phase) cells towards every
 *                      neighbour -- the ghost results it writes are valid inputs of the next step, no
 *                      communication at all;
 *   phase == halo-1    the pipelined step above: boundary strips (halo deep) of `out`, pack, then the
 *                      exchange of `out`'s ghost cells next to the interior kernel.
 * Per-step overhead of the exchange choreography is divided by `halo` for (halo-1)/2 redundant rows
 * per side on average.  halo = 1 is gt4mi_dist_lap5_f64_pipelined. */
int gt4mi_dist_lap5_f64_wide(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* inp,
                             const gt4mi_field* out, int variant, int sides, int halo, int phase,
                             void* main_stream);

/* Time-skewed form of the same: ONE call runs a whole cycle of `halo` steps, field_a -> field_b -> field_a ... (the
 * result is in field_b for odd `halo`, in field_a for even), boundary first:
 *   1. joins the exchange that delivered field_a's ghost cells (previous cycle, or gt4mi_halo_exchange_begin once);
 *   2. for step s = 1 .. halo: the band from halo - s points outside the domain to 2 halo - s points inside it
 *      (one ring launch each) -- after the last band the halo-deep faces of the result are final;
 *   3. packs them and starts their exchange on the side stream;
 *   4. for step s = 1 .. halo: the interior (the domain shrunk by 2 halo - s), `halo` kernels that all run next to the
 *      exchange.
 * Same redundant rows as the _wide form, but the exchange has `halo` interior kernels to hide behind instead of one.
 * Two buffers suffice: band s overwrites only what interior s - 1 no longer reads. */
int gt4mi_dist_lap5_f64_skewed(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* field_a,
                               const gt4mi_field* field_b, int variant, int sides, int halo, void* main_stream);

/* ---- run-time compiled stencils (generic executor) --------------------------------------------
 * Replaces the reference's per-stencil JIT build: setuptools + nvcc building a pybind11 extension
 * (/root/reference/src/gt4py/cartesian/backend/pyext_builder.py:176-303, driven by
 * backend/gtc_common.py:226-275) and that extension's `run_computation`
 * (backend/gtc_common.py:65-103).  The host generates HIP source for stencils outside the hand-written
 * families (gt4py_amd/cartesian/backend/hip_codegen.py); these entries compile it in-process with
 * hiprtc for gfx950 (always with -O3 -std=c++17 -ffp-contract=off; `options` are appended), load the
 * code object and launch kernels from it.  Compilation needs no GPU; load/launch do.
 *
 * gt4mi_rtc_compile: *code is malloc'ed by the library, release it with gt4mi_rtc_free.  `log`
 * (optional) receives the compiler log, truncated to log_size.
 * gt4mi_launch: `args` is the kernel-argument block (the generated kernel takes ONE struct by value;
 * the host lays it out with C rules), copied at launch.  grid is in workgroups. */
typedef struct gt4mi_module gt4mi_module;
int gt4mi_rtc_compile(const char* source, const char* name, const char* const* options, int n_options,
                      void** code, size_t* code_size, char* log, size_t log_size);
int gt4mi_rtc_free(void* code);
int gt4mi_module_load(const void* code, gt4mi_module** module);
int gt4mi_module_unload(gt4mi_module* module);
int gt4mi_module_function(gt4mi_module* module, const char* name, void** function);
/* What the compiler made of a loaded kernel: registers per lane, bytes of scratch (spills) per lane, static LDS bytes
 * per workgroup.  The host uses it to refuse kernel variants that spill.  Any pointer may be NULL. */
int gt4mi_function_info(void* function, int* registers, int* scratch_bytes, int* lds_bytes);
int gt4mi_launch(void* function, const uint32_t grid[3], const uint32_t block[3], const void* args,
                 size_t args_size, void* stream, gt4mi_exec_info* info);
/* The launches of one stencil call in one crossing of the boundary, in order, on one stream: n kernels,
 * grids / blocks as n consecutive triples, one argument block (of the same size) per launch.  A stencil of
 * several stages -- or one whose sequential block runs plane by plane, two launches per K level -- otherwise
 * pays the host language's call overhead per kernel.  Stops at the first failing launch. */
int gt4mi_launch_batch(int n, void* const* functions, const uint32_t* grids, const uint32_t* blocks,
                       const void* const* args, size_t args_size, void* stream, gt4mi_exec_info* info);

/* ---- measurement helper ---------------------------------------------------------------------
 * Streaming device copy of nbytes (multiple of 16) with 16-byte lanes: the "achievable HBM"
 * yardstick printed next to the stencil numbers. */
int gt4mi_stream_copy(const void* src, void* dst, size_t nbytes, void* stream);

/* ---- memory groups (ABI 7; new: the reference allocates through cupy and knows nothing of the device's memory system) -------------
 * MI355X's memory is not one uniformly interleaved pool: two big allocations either share a group of memory channels or they do
 * not, and nothing in the HIP API says which.  Kernels feel it -- two 1.3 GB fields written side by side: 5.0-6.4 TB/s in one group,
 * 6.8-7.0 TB/s in two; the fp64 Laplacian 512^3 +2.3 % with `in` and `out` in different groups; the tridiagonal solve 0.70 of the
 * HBM peak with its five fields dealt over two groups, 0.61 with all five in one (profiles/r5_memory_groups.txt).  This probe
 * measures it: ONE kernel writes both buffers the way a column kernel does; *gbs = bytes written to both per second / 1e9.
 * `b` may be NULL (one buffer alone).  OVERWRITES the first `bytes` (rounded down to planes of 8 MiB, at least 192 MiB) of both
 * buffers; synchronous on `stream`.  gt4py_amd/storage/placement.py uses it to deal big fields over the groups. */
int gt4mi_memory_write_probe(void* a, void* b, size_t bytes, int iterations, void* stream, double* gbs);

#ifdef __cplusplus
}
#endif
#endif /* GT4PY_AMD_H */
