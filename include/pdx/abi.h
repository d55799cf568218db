/*
 * pdx/abi.h -- C ABI of libpdx_hip.so: the MI355X (gfx950) execution backend that replaces the
 * Arrow-CPU compute underneath PandasArrow's vectorized operator path.
 *
 * Drop-in boundary.  In the reference every numeric operation on this
 * path is a forward to
 *     arrow::compute::CallFunction("<kernel-name>", {Datum...}, FunctionOptions*)
 * or to arrow::compute::Grouper::{Make,Consume,MakeGroupings,ApplyGroupings,GetUniques}.
 * Each entry point below cites the reference call site(s) it replaces (file:line relative to the
 * reference repository).  INTEGRATION.md shows the binding a maintainer adds at those sites.
 *
 * Conventions
 *   - Columns are Arrow-layout raw buffers that live in DEVICE memory (HBM): a contiguous values
 *     buffer plus an optional validity bitmap (1 bit/row, LSB first), both addressed with an element
 *     `offset` exactly like a sliced arrow::ArrayData.  PDX_BOOL values are bit-packed.
 *   - Inputs are borrowed and never mutated.  Outputs whose size is known up front are written into
 *     caller-provided buffers (pdx_mut_column); data-dependent results (group-by, resample) live in
 *     an opaque handle owned by the library until pdx_*_destroy.
 *   - Every function returns a pdx_status.  No exception crosses this boundary; the C++ facade
 *     (pandasarrow_amd/cpp) rethrows std::runtime_error(pdx_last_error()) the way the reference's
 *     ReturnOrThrowOnFailure does (src/core.h:181-194).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are ordered on
 *     that stream; entry points that return host-visible results (scalars, counts) synchronise it.
 *   - Threading (the reference calls this boundary from tbb::parallel_for workers, src/pd_core_macros.h:21,56,94,122): every
 *     entry point may be called concurrently from several host threads, each on its own stream (or all on the same one).  The
 *     only shared state is the scratch pool, which is kept per device and is stream ordered: a block freed by a call on stream S
 *     is reused at once by later calls on S, and by calls on other streams / threads only after the work queued on S at the time
 *     of the free has completed.  A handle (pdx_groupby, pdx_grouped) must not be used by two threads at the same time, and calls
 *     that use one handle on different streams must be ordered by the caller (the handle's buffers are not stream-synchronised).
 *     pdx_last_error is thread local.  Tested by tests/test_gpu_threads.py.
 */
#ifndef PDX_ABI_H
#define PDX_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDX_ABI_VERSION 1

typedef enum pdx_status {
  PDX_OK = 0,
  PDX_INVALID = 1,      /* arrow::Status::Invalid: type/length mismatch, integer divide by zero, bad argument */
  PDX_INDEX_ERROR = 2,  /* arrow::Status::IndexError: take index out of bounds */
  PDX_OOM = 3,          /* device allocation failed */
  PDX_DEVICE = 4,       /* HIP runtime error */
  PDX_NOT_IMPLEMENTED = 5
} pdx_status;

typedef enum pdx_dtype {
  PDX_INT64 = 0,
  PDX_FLOAT64 = 1,
  PDX_BOOL = 2,         /* bit-packed, LSB first */
  PDX_UINT64 = 3,
  PDX_TIMESTAMP_NS = 4, /* int64 nanoseconds since epoch */
  /* 4 bytes per value (`offset` still counts elements).  Accepted by pdx_binary, pdx_compare, pdx_if_else, pdx_unary (not
   * pdx_power), pdx_cast, pdx_aggregate, pdx_filter, pdx_take, pdx_scatter, pdx_concat, pdx_cumulative, pdx_fill_null, pdx_shift, pdx_quantile, pdx_mode, pdx_sort_indices, pdx_select_k, pdx_partition_nth, pdx_row_aggregate,
   * the lookups (pdx_is_in ... pdx_dictionary_encode), pdx_join_create (PDX_INT32 keys)
   * and the selection / multiplexing calls (pdx_coalesce ... pdx_all_valid_mask); every other entry point returns
   * PDX_NOT_IMPLEMENTED naming the dtype (the group-by does not take 4-byte keys yet, so value_counts of such a column is refused too).  In a pdx_scalar an INT32 value is held sign-extended in v.i64, a FLOAT32 value
   * widened (exactly) in v.f64. */
  PDX_INT32 = 5,
  PDX_FLOAT32 = 6
} pdx_dtype;

/* immutable input column (mirrors the fields of arrow::ArrayData the kernels read) */
typedef struct pdx_column {
  int32_t dtype;        /* pdx_dtype */
  int32_t reserved;
  int64_t length;       /* rows */
  int64_t offset;       /* element offset into values; bit offset into validity (and bool values) */
  int64_t null_count;   /* 0 => validity may be NULL; -1 => unknown */
  const void* validity; /* device pointer or NULL */
  const void* values;   /* device pointer */
} pdx_column;

/* caller-allocated output column; offset is always 0.  validity may be NULL when the caller knows the
 * result cannot contain nulls (then a would-be null is an error PDX_INVALID). */
typedef struct pdx_mut_column {
  int32_t dtype;
  int32_t reserved;
  int64_t length;       /* capacity in rows on input; rows written on output */
  int64_t null_count;   /* written by the library (exact), -1 if not computed */
  void* validity;       /* device pointer to (length+7)/8 bytes (+8 bytes slack), or NULL */
  void* values;         /* device pointer */
} pdx_mut_column;

/* host-visible scalar result (arrow::Scalar analogue) */
typedef struct pdx_scalar {
  int32_t dtype;
  int32_t is_valid;     /* 0 => null (e.g. sum of an empty / all-null array, min_count = 1) */
  union {
    int64_t i64;
    uint64_t u64;
    double f64;
  } v;
  int64_t count;        /* number of valid inputs that produced it */
} pdx_scalar;

typedef enum pdx_binary_op {
  PDX_ADD = 0, PDX_SUB = 1, PDX_MUL = 2, PDX_DIV = 3,
  /* integer operands only: BINARY_OPERATOR(| & ^ << >>) src/series.cpp:237-245, BINARY_OPERATOR_DF src/dataframe.cpp:553-561.
   * Shifts are Arrow's unchecked kernels: an amount that is negative or >= 63 (the precision of int64) returns the left operand
   * unchanged; shift_right is arithmetic; shift_left wraps. */
  PDX_BIT_OR = 4, PDX_BIT_AND = 5, PDX_BIT_XOR = 6, PDX_SHIFT_LEFT = 7, PDX_SHIFT_RIGHT = 8
} pdx_binary_op;
/* element-wise functions of one column (pdx_unary) */
typedef enum pdx_unary_op { PDX_NEGATE = 0, PDX_ABS = 1, PDX_SIGN = 2, PDX_SQRT = 3, PDX_EXP = 4, PDX_BIT_NOT = 5 } pdx_unary_op;
/* running accumulations of one column (pdx_cumulative) */
typedef enum pdx_cum_op { PDX_CUM_SUM = 0, PDX_CUM_PROD = 1, PDX_CUM_MAX = 2, PDX_CUM_MIN = 3 } pdx_cum_op;
typedef enum pdx_compare_op { PDX_EQ = 0, PDX_NE = 1, PDX_LT = 2, PDX_LE = 3, PDX_GT = 4, PDX_GE = 5 } pdx_compare_op;
typedef enum pdx_logical_op { PDX_AND = 0, PDX_OR = 1 } pdx_logical_op;
/* which operand of pdx_binary / pdx_compare is a length-1 column that is broadcast (the `b_is_scalar` argument) */
typedef enum pdx_scalar_side { PDX_SCALAR_NONE = 0, PDX_SCALAR_RHS = 1, PDX_SCALAR_LHS = 2 } pdx_scalar_side;
typedef enum pdx_agg_kind {
  PDX_AGG_SUM = 0, PDX_AGG_MEAN = 1, PDX_AGG_MIN = 2, PDX_AGG_MAX = 3, PDX_AGG_COUNT = 4,
  /* group-by only (pdx_groupby_agg; SURVEY 8(f)-3, the reference's GROUPBY_NUMERIC_AGG(variance|stddev), GROUPBY_AGG(product),
   * GroupBy::first/last, src/dataframe.cpp:1516-1536, 1698-1810).  variance/stddev: Arrow defaults (ddof = 0, nulls skipped,
   * null for a group without valid values), two pairwise passes -> float64.  product: one multiply per valid value in row
   * order, int64 wraps, null without valid values -> value dtype.  first/last: the group's first / last ROW (null if that row
   * is null) -> value dtype. */
  PDX_AGG_VARIANCE = 5, PDX_AGG_STDDEV = 6, PDX_AGG_PRODUCT = 7, PDX_AGG_FIRST = 8, PDX_AGG_LAST = 9,
  /* GROUPBY_NUMERIC_AGG(all | any, bool) and GROUPBY_NUMERIC_AGG(count_distinct, int64_t), src/dataframe.cpp:1520-1526.
   * all / any: PDX_BOOL values -> PDX_BOOL result (nulls skipped; a group without a valid value is null, so the output needs a
   * validity buffer).  count_distinct: the number of distinct VALID values per group -> PDX_INT64, never null; float64 values
   * are distinct when their bit patterns are (0.0 / -0.0 and NaN payloads count separately, like Arrow's memo table).
   * GroupBy::min_max (src/dataframe.cpp:1602-1696) is {PDX_AGG_MIN, PDX_AGG_MAX} in one call. */
  PDX_AGG_ALL = 10, PDX_AGG_ANY = 11, PDX_AGG_COUNT_DISTINCT = 12,
  /* pdx_row_aggregate only (every other entry point refuses it): count with CountOptions::ONLY_NULL, the null cells of a row */
  PDX_AGG_COUNT_NULL = 13
} pdx_agg_kind;
typedef enum pdx_origin {
  PDX_ORIGIN_EPOCH = 0, PDX_ORIGIN_START_DAY = 1, PDX_ORIGIN_START = 2, PDX_ORIGIN_END = 3, PDX_ORIGIN_END_DAY = 4, PDX_ORIGIN_CUSTOM = 5,
  /* OR-ed into origin_type by a multi-GPU caller whose `ts` is one row-range shard of a longer axis (bins made whole by the caller,
   * origin passed as PDX_ORIGIN_CUSTOM from the whole axis): the rows < bins test ("upSampling") belongs to the whole axis, which
   * the caller has already checked, so it is not applied to the shard */
  PDX_ORIGIN_SHARD = 0x100
} pdx_origin;

/* ---------------------------------------------------------------- runtime */
int pdx_abi_version(void);
/* "pdx-hip abi <version> gfx950 sources <digest>": the digest (sha256 prefix over the .hip / .hpp files under csrc and this header, computed by
 * __graft_entry__.build()) names the source tree the loaded library was compiled from; tests/test_abi_symbols.py compares it with the
 * tree, so a stale in-tree .so cannot pass for a build of the current sources. */
const char* pdx_build_info(void);
/* Select the HIP device for the calling thread and create the scratch pool.  Idempotent. */
int pdx_init(int device);
int pdx_shutdown(void);
/* Thread-local message of the last non-OK status returned on this thread ("" if none). */
const char* pdx_last_error(void);
/* Device memory helpers for callers that hand over HOST buffers (the reference builds everything from
 * host std::vector / arrow builders; cudf precedent: src/cudf/cudf_utils.h:118-141). */
int pdx_malloc(void** dptr, size_t bytes);
int pdx_free(void* dptr);
int pdx_to_device(void* dst_device, const void* src_host, size_t bytes, void* stream);
int pdx_to_host(void* dst_host, const void* src_device, size_t bytes, void* stream);
int pdx_stream_synchronize(void* stream);
/* Release cached scratch memory back to the driver. */
int pdx_trim_pool(void);

/* Optional per-kernel timing: when enabled, HIP events bracket each kernel family on its launch stream.
 * pdx_profile_report writes one "tag count total_ms" line per kernel family. Used by bench.py for the roofline line. */
int pdx_profile_enable(int on);
int pdx_profile_reset(void);
int pdx_profile_report(char* buf, size_t buf_len);

/* ---------------------------------------------------------------- synthetic inputs
 * Counter-based generators, bit-identical to oracle/pdx_oracle.c orc_synth_*; used by bench.py/tests. */
int pdx_synth_keys(int64_t start, int64_t n, int64_t num_keys, int64_t* out, void* stream);
int pdx_synth_vals(int64_t start, int64_t n, uint64_t seed_off, double* out, void* stream);
int pdx_synth_ts(int64_t start, int64_t n, int64_t t0_ns, int64_t step_ns, int64_t* out, void* stream);

/* ---------------------------------------------------------------- element-wise
 * Replaces CallFunction("add"|"subtract"|"multiply"|"divide", {lhs, rhs}) at src/series.cpp:19-33 (macro
 * BINARY_OPERATOR, instantiated 229-235), src/scalar.cpp:24-36 (Scalar rhs/lhs) and the DataFrame form
 * src/dataframe.cpp:233-275.  a,b: PDX_INT64 or PDX_FLOAT64 (mixed => float64 result, like Arrow's implicit
 * promotion).  b_is_scalar is a pdx_scalar_side: PDX_SCALAR_RHS (1): b has length 1 and is broadcast (`series - 2`,
 * src/series.cpp:25-28); PDX_SCALAR_LHS (2): a has length 1 and is broadcast (`2 - series`, `2 / series`:
 * Scalar::operator op(Series) -> BinaryImpl -> CallFunction(name, {scalar, s.array()}), src/scalar.cpp:24-36; the result has
 * b's length).  Integer arithmetic wraps; integer divide truncates toward zero, INT64_MIN / -1 == 0, a zero divisor at a valid
 * slot fails the whole call with PDX_INVALID "divide by zero".  out null where either input is null.
 * PDX_BIT_OR .. PDX_SHIFT_RIGHT take int64 operands only (PDX_NOT_IMPLEMENTED otherwise: Arrow has no floating-point kernels). */
int pdx_binary(int op, const pdx_column* a, const pdx_column* b, int b_is_scalar, pdx_mut_column* out, void* stream);
/* Replaces CallFunction("equal"|"not_equal"|"less"|"less_equal"|"greater"|"greater_equal") at
 * src/series.cpp:247-257 and, with PDX_SCALAR_LHS, Scalar::operator{>,>=,<,<=,==,!=}(Series) at src/scalar.cpp:48-56.
 * out: PDX_BOOL (bit-packed). */
int pdx_compare(int op, const pdx_column* a, const pdx_column* b, int b_is_scalar, pdx_mut_column* out, void* stream);
/* Replaces CallFunction("and"|"or") (non-Kleene) at src/series.cpp:259-260 and "invert" at src/series.cpp:319. */
int pdx_logical(int op, const pdx_column* a, const pdx_column* b, pdx_mut_column* out, void* stream);
int pdx_invert(const pdx_column* a, pdx_mut_column* out, void* stream);
/* Replaces arrow::compute::IfElse(cond, a, b): Series::if_else / Series::where(cond, other) with a Series or Scalar `other`
 * (src/series.cpp:1203-1209, 1247-1253; pinned by tests/series_indexing_test.cpp:36-52).  cond: PDX_BOOL of the result's length;
 * a, b: PDX_INT64 or PDX_FLOAT64 (mixed => float64); scalar_side (pdx_scalar_side): RHS = b has length 1, LHS = a has length 1.
 * out[i] = cond[i] ? a[i] : b[i]; null where cond is null or the chosen operand is null (the other operand's nulls do not count). */
int pdx_if_else(const pdx_column* cond, const pdx_column* a, const pdx_column* b, int scalar_side, pdx_mut_column* out, void* stream);
/* Replaces CallFunction("negate" | "abs" | "sign" | "sqrt" | "exp" | "bit_wise_not", {array}): DataFrame::unary (operator-,
 * operator~) and the UNARY_FUNCTION macros src/dataframe.cpp:251-275, 919-935, src/dataframe.h:494-502; Series::abs / exp /
 * sign / sqrt src/series.h:89-109.  a: PDX_INT64, PDX_UINT64 or PDX_FLOAT64; out null where a is null.
 *   NEGATE, ABS : the input type; integers wrap (negate(INT64_MIN) == abs(INT64_MIN) == INT64_MIN; uint64: negate wraps, abs is
 *                 the identity)
 *   SIGN        : float64 -> float64 (-1, 0, 1; NaN stays NaN); integers -> PDX_INT64 values -1 / 0 / 1 (Arrow returns int8:
 *                 this backend's integer columns are 64 bits wide)
 *   BIT_NOT     : integers only (PDX_NOT_IMPLEMENTED for float64, as Arrow has no such kernel)
 *   SQRT, EXP   : -> PDX_FLOAT64.  Integer input is cast first the way Arrow's implicit cast does: a valid value outside
 *                 +-2^53 fails the whole call with PDX_INVALID "Integer value ... not in range".  sqrt of a negative number
 *                 is NaN.  SQRT is correctly rounded (bit-identical to the reference); EXP follows the device's libm and can
 *                 differ from the reference's host libm in the last place (the reference's own result depends on its glibc
 *                 build): the only element-wise result on this path that is not bit-reproducible. */
int pdx_unary(int op, const pdx_column* a, pdx_mut_column* out, void* stream);
/* Replaces arrow::compute::Cast(column, float64()): the promotion of same-named int64 / float64 columns in pd::concat (src/concat.cpp:116-132:
 * default CastOptions = the SAFE cast: checked = 1, a valid int64 value outside +-2^53 fails the call with PDX_INVALID "Integer value ... not in
 * range: -9007199254740992 to 9007199254740992" -- the same check Arrow's DispatchBest applies when pdx_binary / pdx_compare / pdx_if_else
 * meet an int64 and a float64 operand) and the value-by-value static_cast<double> of Arrow's `mean` over int64 input (checked = 0: the
 * frame-level DataFrame::mean sums int64 chunks as doubles, src/ndframe.h:329-335).  a: PDX_INT64 (or PDX_FLOAT64: a copy); nulls carried over. */
int pdx_cast_f64(const pdx_column* a, int checked, pdx_mut_column* out, void* stream);
/* Replaces CallFunction("power", {array, Datum(double)}): Series::pow / DataFrame::pow (src/dataframe.cpp:267-270).  Integer input
 * is cast to float64 as in pdx_unary(SQRT); out: PDX_FLOAT64 = pow(a, exponent), last-place caveat as for EXP. */
int pdx_power(const pdx_column* a, double exponent, pdx_mut_column* out, void* stream);

/* ---------------------------------------------------------------- 32-bit columns (PDX_INT32, PDX_FLOAT32)
 * pdx_binary / pdx_compare / pdx_if_else follow Arrow's implicit promotion (Arrow C++ 25, tests/golden/narrow_golden.npz):
 *   int32 (+) int32 -> int32 (wraps; shifts: an amount < 0 or >= 31 returns the left operand), float32 (+) float32 -> float32
 *   (rounded in fp32), int32 (+) int64 -> int64, int32 / float32 (+) float64 -> float64 (exact), int32 / int64 (+) float32 ->
 *   float32 through a CHECKED cast: a valid integer outside +-2^24 fails the call with PDX_INVALID "Integer value ... not in
 *   range: -16777216 to 16777216" (the first such row is named).
 * pdx_unary: NEGATE / ABS / SIGN / BIT_NOT keep int32 (SIGN of float32 stays float32); SQRT of int32 -> float64, SQRT / EXP of
 *   float32 -> float32.
 * pdx_aggregate: sum(int32) -> int64 (exact); sum(float32) -> float64 (each value widened, then the float64 pairwise tree);
 *   mean -> float64; min / max keep the input dtype; count -> int64. */
/* Arrow's safe Cast between numeric columns: int32 -> int64 / float64, float32 -> float64 (exact), int32 / int64 -> float32 (checked
 * as above), and the identity for any supported dtype.  out->dtype names the target; nulls are carried over. */
int pdx_cast(const pdx_column* a, pdx_mut_column* out, void* stream);

/* ---------------------------------------------------------------- cumulative scans, fill_null, shift (order-dependent transforms)
 * Common rules: out->dtype equals a's, out->length >= a->length; input validity and offset are arbitrary (bit offsets that are not
 * multiples of 8 included); length is int64 (no 2^31 limit); an empty input gives PDX_OK and length 0.  out->validity may be NULL only
 * when the result cannot hold a null (PDX_INVALID otherwise); out->null_count is exact; value bytes under a null output row are
 * unspecified.  `out` must not alias `a` (in place is not supported: equal value pointers are refused with PDX_INVALID).  The calls are
 * asynchronous on `stream` except where they read the null count back: pdx_cumulative and pdx_fill_null when the input carries a validity
 * bitmap with null_count != 0, pdx_shift when such an input keeps at least one of its rows.
 *
 * pdx_cumulative replaces CumulativeSum / Prod / Max / Min(array, CumulativeOptions{start, skip_nulls}): Series::cumsum / cumprod / cummax /
 * cummin (src/series.cpp:321-339).  a: PDX_INT64, PDX_UINT64, PDX_FLOAT64, PDX_INT32, PDX_FLOAT32; PDX_TIMESTAMP_NS and PDX_BOOL return
 * PDX_NOT_IMPLEMENTED "Function 'cumulative_sum' has no kernel matching input types (timestamp[ns])".  Integer sums and products wrap;
 * float32 accumulates in fp32.  `start` is cast to the column's type by Arrow's safe cast before anything is launched: PDX_INVALID "Float
 * value 1.500000 was truncated converting to int64" for a fraction, NaN or a value outside the type's range; float32 rounds it to nearest.
 * The reference always passes a start, so it is a required argument (Arrow's own default for cumulative_max of float64,
 * numeric_limits<double>::min(), is not reproduced).  skip_nulls != 0: a null row is null in the output and the accumulation goes on behind
 * it; skip_nulls == 0: every row from the first null on is null.  max / min skip NaN values (a NaN start included) and the LATER operand
 * wins a tie (signed zeros).
 * Bit-exact against the reference: integer sum / product, max / min of every dtype.  NOT bit-reproducible: the float64 / float32 SUM and
 * PRODUCT -- the reference adds left to right, and a chain of rounded additions has no parallel evaluation with the same bits.  Their contract:
 * (1) deterministic: the bits are a function of values, validity and start alone (the evaluation tree is defined by the row index relative
 * to the slice's first row: any offset, stream, run or PDX_SCAN_CHUNK_ROWS gives the same bits); (2) equal to the reference wherever every
 * order of evaluation gives one result (all partial results exactly representable); (3) within the a-priori bound of any summation order,
 * |got_i - exact_i| <= (k_i - 1) u / (1 - (k_i - 1) u) * (|start| + sum |x_j|), k_i = valid terms up to row i with the start, u = 2^-53
 * (2^-24) -- for the product the same factor times |exact_i|, absent overflow / underflow; (4) NaN and infinities from the VALUES appear where
 * the reference has them (NaN sign / payload not compared); an intermediate overflow of finite values is the exception: the reference's
 * running sum can reach infinity where a tree's partial sums stay finite, and the other way round.
 *
 * pdx_fill_null replaces fill_null_forward / fill_null_backward: Series / DataFrame::ffill / bfill (src/series.cpp:748-750,
 * src/dataframe.cpp:1292-1294).  a: the five dtypes above and PDX_TIMESTAMP_NS (PDX_BOOL: PDX_NOT_IMPLEMENTED).  Leading (backward:
 * trailing) nulls stay null; a slice is filled from its own rows only.
 *
 * pdx_shift replaces Series::shift(periods, fill) (src/series.cpp:702-736): out[i] = a[i - periods] where that row exists, else the fill
 * (fill == NULL or fill->is_valid == 0: null).  periods > 0 moves rows toward the end, 0 is a copy, |periods| >= length gives a column of
 * fills (the reference's builder fails there).  Same dtypes as pdx_fill_null; fill->dtype must equal a's (PDX_INVALID), 4-byte values as
 * pdx_scalar documents (v.i64 sign-extended, v.f64 widened).  One pass over the data. */
int pdx_cumulative(int op, const pdx_column* a, double start, int skip_nulls, pdx_mut_column* out, void* stream);
int pdx_fill_null(int backward, const pdx_column* a, pdx_mut_column* out, void* stream);
int pdx_shift(const pdx_column* a, int64_t periods, const pdx_scalar* fill /* NULL: nulls */, pdx_mut_column* out, void* stream);

/* ---------------------------------------------------------------- whole-array aggregates
 * Replaces CallFunction("sum"|"mean"|"min"|"max"|"count", {array}, ScalarAggregateOptions{skip_nulls=true,
 * min_count=1}) at src/ndframe.cpp:26-31 (macro), 119, 162-166, 220, and MinMax at src/resample.cpp:223.
 * fp64 sum reproduces Arrow's pairwise tree bit-for-bit (16-value leaves per valid run, binary-counter merge).
 * Synchronises `stream`. */
int pdx_aggregate(int kind, const pdx_column* a, pdx_scalar* out, void* stream);

/* ---------------------------------------------------------------- row-wise aggregates (axis = Columns)
 * Replaces DataFrame::forAxis(name, AxisType::Columns, options) (src/dataframe.cpp:138-175: one GetScalar per cell, one ScalarArray::Make and
 * one CallFunction per row) behind DataFrame::sum / mean / min / max / count / count_na / product / first / last / all / any / std / var
 * (AxisType, ...) (src/dataframe.cpp:177-229).  For every row i, out[i] is what Arrow C++ 25.0.0's scalar aggregate `kind` returns for the
 * ncols-element array [cols[0][i], ..., cols[ncols - 1][i]] under ScalarAggregateOptions{skip_nulls, min_count} (variance / stddev:
 * VarianceOptions{ddof, skip_nulls, min_count}; count kinds take no option), bit for bit (tests/golden/rowagg_golden.npz) -- except the
 * payload of a NaN that min / max / product / variance / stddev return.
 *   kind : pdx_agg_kind SUM .. ANY and PDX_AGG_COUNT_NULL; PDX_AGG_COUNT_DISTINCT returns PDX_NOT_IMPLEMENTED.
 *   cols : 1 <= ncols <= 2046 columns of ONE dtype and one length (PDX_INVALID otherwise: the reference's ScalarArray::Make fails on a row
 *          of mixed types).  int64, uint64, float64, int32, float32: every kind but ALL / ANY (variance / stddev: int64 and float64, as
 *          pdx_groupby_agg); bool: ALL, ANY, COUNT, COUNT_NULL; timestamp[ns]: MIN, MAX, FIRST, LAST, COUNT, COUNT_NULL.  Any other pair
 *          returns PDX_NOT_IMPLEMENTED "Function 'sum' has no kernel matching input types (timestamp[ns])".  Any offset, validity at any
 *          bit offset, null_count -1; a column without validity is all valid; length is int64.
 *   out  : SUM, PRODUCT -> int64 for int64 / int32 (wrapping), uint64 for uint64, float64 for floats; MEAN, VARIANCE, STDDEV -> float64;
 *          MIN, MAX, FIRST, LAST -> the input dtype; COUNT, COUNT_NULL -> int64, never null; ALL, ANY -> bool.  out->length >= the
 *          columns' length, out->dtype as listed (PDX_INVALID otherwise).  out->validity may be NULL only when no row can be null for these
 *          options and columns (PDX_INVALID otherwise).  Rows, bytes and validity bits of `out` beyond the columns' length are untouched;
 *          value bytes under a null row are zero.
 *   rules: a row is null when skip_nulls == 0 and it holds a null cell, or when fewer than min_count cells are valid; MIN / MAX / FIRST /
 *          LAST also without a valid cell, VARIANCE / STDDEV with no more than ddof.  With min_count 0 a row without valid cells sums to 0,
 *          multiplies to 1 and averages to NaN.  fp64 SUM / MEAN: Arrow's pairwise tree over the row in column order (float32 widened per
 *          value, MEAN of integers over the values as doubles).  MIN / MAX skip NaN cells unless all are NaN; of 0.0 / -0.0 MIN keeps the
 *          first, MAX the first in a row without null cells and the last in a row with one.  FIRST / LAST with skip_nulls == 0 are the first
 *          / last CELL (null when that cell is null).  ALL / ANY with skip_nulls == 0: a valid false (true) decides the row, else a null
 *          cell makes it null.
 * One kernel launch reads every input byte once (twice for VARIANCE / STDDEV).  Nothing can fail at run time: the call is asynchronous on
 * `stream`, except that out->null_count (always exact) is read back, as pdx_cumulative does, when a column carries a validity bitmap with
 * null_count != 0 and the kind and options admit a null row. */
int pdx_row_aggregate(int kind, const pdx_column* cols, int ncols, int skip_nulls, int64_t min_count, int ddof, pdx_mut_column* out, void* stream);

/* ---------------------------------------------------------------- exact quantiles
 * Replaces CallFunction("quantile", {array}, QuantileOptions{q, interpolation, skip_nulls, min_count}): NDFrame::quantile
 * (src/ndframe.h:259-263, src/ndframe.cpp:202-212), the per-percentile calls of DataFrame::describe (src/dataframe.cpp:983-1030) and, per
 * group, GroupBy::quantile (src/group_by.h:123-124, src/dataframe.cpp:1867-1931).  Semantics = Arrow C++ 25.0.0, bit for bit
 * (tests/golden/quantile_golden.npz):
 *   - a: PDX_INT64, PDX_UINT64, PDX_FLOAT64, PDX_INT32, PDX_FLOAT32 (pdx_groupby_quantile: the three 8-byte dtypes).  PDX_TIMESTAMP_NS and
 *     PDX_BOOL return PDX_NOT_IMPLEMENTED "Function 'quantile' has no kernel matching input types (timestamp[ns])".
 *   - nulls and NaN values take no part; n = number of valid non-NaN values = `count` of the scalar.  The result is null (is_valid = 0 /
 *     validity bit clear) when n == 0, when fewer than min_count rows are non-null (Arrow counts NaN rows here), or when skip_nulls == 0 and
 *     the input (the group) holds a null.
 *   - every q in [0, 1], else (NaN too; Arrow itself lets a NaN q through) PDX_INVALID "Quantile must be between 0 and 1"; nq <= 0: PDX_INVALID "Requires quantile argument"; both
 *     before anything is launched.
 *   - with v = the n values ascending, index = (n - 1) * q in double, lo = (uint64) index, f = index - lo, hi = lo + 1 when f != 0 else lo:
 *       LINEAR   -> float64: f == 0 ? (double) v[lo] : f * (double) v[hi] + (1 - f) * (double) v[lo]   (each product rounded, no FMA)
 *       MIDPOINT -> float64: f == 0 ? (double) v[lo] : v[lo] / 2 + v[hi] / 2                           (halves first: no overflow)
 *       LOWER v[lo], HIGHER v[hi], NEAREST f < 0.5 ? v[lo] : f > 0.5 ? v[hi] : v[lo + (lo & 1)]        (a tie goes to the even index)
 *     LOWER / HIGHER / NEAREST keep the input dtype (4-byte values in a pdx_scalar as pdx_dtype documents).
 *   - -0.0 and 0.0 are equal in the order: where a result is a zero of a column that holds both, it is the zero that comes first in
 *     pdx_argsort's stable order, i.e. v's zeros keep their ROW order (Arrow returns whichever zero its nth_element left there).
 * pdx_quantile: the ranks of all nq quantiles are located from ONE histogram read of the column (64 per read beyond that); unless that read
 * already settles them (one distinct value) a second read copies out the bins that hold them, and a result that is a zero of a float column
 * costs a third.  Scratch: the copied bins, in the worst case (every row in one bin, e.g. two distinct values) one key per row, held until
 * the call returns.  Length is int64 without a 2^31 limit, every
 * count and rank is 64 bits wide; any offset, validity at any bit offset, null_count -1; deterministic (same bits on any stream / run).
 * Synchronises `stream` like pdx_aggregate.  outs: nq scalars.
 * pdx_groupby_quantile: per group the same rule over the group's rows; handles from pdx_groupby_create / pdx_resample_create /
 * pdx_downsample_create, the handle's row limit.  outs: nq columns of >= G rows, PDX_FLOAT64 (LINEAR / MIDPOINT) or the values' dtype;
 * validity is required when a group result is null (PDX_INVALID otherwise), null_count is exact.  Neither the bound-column cache nor
 * pdx_groupby_last_plan is touched. */
/* arrow::compute::QuantileOptions::Interpolation, same numbering */
typedef enum pdx_interpolation { PDX_INTERP_LINEAR = 0, PDX_INTERP_LOWER = 1, PDX_INTERP_HIGHER = 2,
                                 PDX_INTERP_NEAREST = 3, PDX_INTERP_MIDPOINT = 4 } pdx_interpolation;
int pdx_quantile(const pdx_column* a, const double* q, int nq, int interpolation, int skip_nulls, int64_t min_count,
                 pdx_scalar* outs /* nq */, void* stream);

/* ---------------------------------------------------------------- filter / take
 * Replaces CallFunction("filter", {RecordBatch, mask}, FilterOptions{EMIT_NULL}) + CallFunction("array_filter",
 * {index, mask}) at src/dataframe.cpp:461-475 and src/series.cpp:130-144.  mask: PDX_BOOL of the same length as
 * every column (else PDX_INVALID).  Two calls: count (host-visible) then fill; the facade hides the pair.
 * Output validity bitmaps: give them a capacity rounded up to a multiple of 4 bytes and a 4-byte aligned start (any device
 * allocation has both): null rows clear their bit with a 32-bit atomic on the word that holds it.  A bitmap that does not start on
 * a 4-byte boundary is still served (row-id gather path), only slower. */
int pdx_filter_count(const pdx_column* mask, int emit_null, int64_t* out_count, void* stream);
int pdx_filter(const pdx_column* cols, int ncols, const pdx_column* mask, int emit_null, pdx_mut_column* outs, void* stream);
/* Replaces CallFunction("take", {RecordBatch, indices}) + "array_take" at src/dataframe.cpp:477-492 and
 * src/series.cpp:146-159.  indices: PDX_INT64.  Out-of-range index => PDX_INDEX_ERROR "Index k out of bounds". */
int pdx_take(const pdx_column* cols, int ncols, const pdx_column* indices, pdx_mut_column* outs, void* stream);

/* Inverse of take: outs[c][indices[j]] = cols[c][j] (indices must be distinct and in [0, outs[c].length)); rows of outs
 * that no index names are left untouched.  Used to place per-owner group results by global group id. */
int pdx_scatter(const pdx_column* cols, int ncols, const pdx_column* indices, pdx_mut_column* outs, void* stream);

/* ---------------------------------------------------------------- selection / multiplexing and null handling
 * Replaces the Arrow kernels behind DataFrame::coalesce (src/dataframe.cpp:1210-1225: "coalesce"), Series::clip (src/series.cpp:874-880:
 * MaxElementWise over MinElementWise), Series::replace_with_mask (src/series.cpp:752-761), Series::indices_nonzero (src/series.cpp:365) and
 * Series / DataFrame::drop_na (src/series.cpp:363, src/dataframe.cpp:1244-1252: "drop_null").  Semantics = Arrow C++ 25.0.0, bit for bit
 * (tests/golden/multiplex_golden.npz).  Common to all: any offset, validity at any bit offset, null_count -1, a column without validity
 * is all valid, int64 lengths; an empty input gives PDX_OK and length 0; out->length >= the result length and out->dtype as stated
 * (PDX_INVALID otherwise); rows, bytes and validity bits of `out` beyond the result length are untouched; value bytes under a null row are
 * zero; out->null_count is exact; deterministic.  The calls are asynchronous on `stream` except where a count is read back (named below).
 *
 * pdx_coalesce: out[i] = the first non-null of cols[0][i] .. cols[ncols - 1][i], null when every cell of the row is.  1 <= ncols <= 2046
 *   columns of ONE dtype (any of the seven; the cells are copied as bits, so NaN payloads and -0.0 survive) and one length.  Mixed dtypes
 *   return PDX_NOT_IMPLEMENTED naming the pair (Arrow would promote: cast first); unequal lengths PDX_INVALID.  out->validity may be NULL only
 *   when cols[0] is all valid.  One launch: a wave reads the validity words of its rows first and loads values only from the columns that
 *   give a row of them its value, so a frame whose first column is mostly valid moves about one column.  The null count is read back when
 *   every column up to the last one that can matter carries a bitmap.
 *
 * pdx_element_wise_minmax: min_element_wise (is_max == 0) / max_element_wise of the operands under ElementWiseAggregateOptions{skip_nulls}.
 *   Operands: 1 .. 2046 columns of ONE dtype -- int64, uint64, float64, int32, float32, timestamp[ns]; bool returns PDX_NOT_IMPLEMENTED
 *   "Function 'min_element_wise' has no kernel matching input types (bool, bool)"; two dtypes PDX_NOT_IMPLEMENTED (the caller promotes) --
 *   of length n = the longest, or of length 1 while n > 1: those are Arrow's scalars, broadcast.  Rules: with skip_nulls a row is null when
 *   every operand is, without it when any is.  A NaN loses to any number and beats a null that is skipped; the result is NaN when every
 *   valid cell is NaN; the payload of a returned NaN is not specified.  Arrow folds the scalars first and then the arrays, each in their
 *   order, through fmin / fmax (accumulator, cell): of 0.0 / -0.0 the earlier of that order stays -- except that a float32 ARRAY cell
 *   replaces an equal accumulator (the later stays) -- and a signalling NaN makes the accumulator NaN until a later number replaces it (a
 *   signalling first scalar: for good).  out->validity may be NULL only when no row can be null (skip_nulls: an operand without validity;
 *   otherwise no operand with validity).  The null count is read back when a row can be null.
 * pdx_clip: max_element_wise(min_element_wise(x, hi), lo) -- the reference's nesting, each level applying skip_nulls on its own -- in one
 *   read of x.  lo and hi are columns of length 1 (the reference's scalars), which may be null: with skip_nulls a null bound does not
 *   bound, without it every row is null.  lo > hi gives lo; a NaN bound does not bound.  Same dtypes, same kernel template.
 *
 * pdx_replace_with_mask: out[i] = repl[k] where mask[i] is valid and true, k = the number of valid true mask rows before i (null where
 *   repl[k] is null); null where mask[i] is null; a[i] otherwise.  All seven dtypes.  PDX_INVALID: mask->length != a->length "Mask must be
 *   of same length as array (expected N items but got M items)"; repl->length below the number of valid true mask rows "Replacement array
 *   must be of appropriate length (expected N items but got M items)" (a longer repl is accepted, its tail ignored; `out` is unspecified
 *   after this failure); repl->dtype != a->dtype, as Arrow has no kernel for a mixed pair.  The count of valid true mask rows is read back
 *   once, together with the null count: the call's only host wait.
 *
 * pdx_indices_nonzero_count / pdx_indices_nonzero: the ascending row indices, PDX_UINT64 and never null, of the rows that are valid and not
 *   zero (bool: true; floats: NaN counts, -0.0 does not).  int64, uint64, float64, int32, float32, bool; timestamp[ns] returns
 *   PDX_NOT_IMPLEMENTED "Function 'indices_nonzero' has no kernel matching input types (timestamp[ns])".  Two calls as pdx_filter_count /
 *   pdx_filter: the count (host-visible), then the fill into out->length >= count rows; both wait for the count.
 *
 * pdx_all_valid_mask: out_mask is a PDX_BOOL column without nulls (its validity is not touched, null_count = 0) whose bit i is set when
 *   every column is valid at row i: the rows drop_null keeps.  1 .. 2046 columns of any dtypes and one length.  drop_na = this mask, then
 *   pdx_filter with emit_null = 0. */
int pdx_coalesce(const pdx_column* cols, int ncols, pdx_mut_column* out, void* stream);
int pdx_element_wise_minmax(int is_max, const pdx_column* cols, int ncols, int skip_nulls, pdx_mut_column* out, void* stream);
int pdx_clip(const pdx_column* x, const pdx_column* lo, const pdx_column* hi, int skip_nulls, pdx_mut_column* out, void* stream);
int pdx_replace_with_mask(const pdx_column* a, const pdx_column* mask, const pdx_column* repl, pdx_mut_column* out, void* stream);
int pdx_indices_nonzero_count(const pdx_column* a, int64_t* out_count, void* stream);
int pdx_indices_nonzero(const pdx_column* a, pdx_mut_column* out, void* stream);
int pdx_all_valid_mask(const pdx_column* cols, int ncols, pdx_mut_column* out_mask, void* stream);

/* ---------------------------------------------------------------- group-by
 * pdx_groupby_create replaces GroupBy::makeGroups (src/dataframe.cpp:1571-1600): Grouper::Make + Consume
 * (dense group ids in FIRST-OCCURRENCE order, a null key is its own group) + GetUniques.  The reference's eager
 * MakeGroupings/ApplyGroupings of every column (src/dataframe.cpp:1539-1569) is deferred to pdx_groupby_agg.
 * GROUP ORDER: exactly first occurrence (group g's first row precedes group g+1's).  Arrow's Grouper::Consume (Arrow C++ 25.0.0, one
 * call over the column, as src/dataframe.cpp:1580 makes it) differs from that by a BOUNDED permutation, and only so: it walks the batch
 * in mini-batches of 128, 256, 512 and then 1024 rows (row boundaries 128, 384, 896, 1920, 2944, ...); the keys first seen in a
 * mini-batch receive ONE CONTIGUOUS BLOCK of ids -- the same block first-occurrence numbering gives them -- permuted inside the block
 * (the insertion rounds of its swiss table).  So: the reference's own tests (<= 17 rows) and any input with at most one new key per
 * mini-batch are exactly first occurrence; group g here and group g there first appear in the same mini-batch, always; per key every
 * aggregate is bit-identical; DataFrame::sort_index (src/dataframe.cpp:1062-1071; both facades) makes two results row-identical.
 * Held against live Arrow on inputs spanning thousands of mini-batches by tests/test_oracle_golden_r4.py (oracle/arrow_order.cpp) and,
 * with this library's own ids, by tests/cpp/arrow_bridge_test.cpp; measured sizes of the permutation: 51 of 97 groups at 1e5 rows / 97
 * keys, 10 145 of 43 107 at 1e5 / 5e4, 23 825 of 993 353 at 5e6 / 1e6 (tests/golden/group_order_arrow25.npz freezes two such cases).
 * key: PDX_INT64 / PDX_TIMESTAMP_NS / PDX_UINT64.  Limits: length < 2^31 rows per call (row ids are 32 bits wide inside the handle;
 * pdx_groupby_sum_mean_count_chunked serves longer inputs for the headline query by an exact merge of chunks); keys that do not span a dense integer
 * range go through a hash table of at most 2^30 slots (about 7e8 distinct keys; the LDS-resident build covers 2.7e8). */
typedef struct pdx_groupby pdx_groupby;
int pdx_groupby_create(const pdx_column* key, void* stream, pdx_groupby** out);
int pdx_groupby_destroy(pdx_groupby* gb);
int64_t pdx_groupby_num_groups(const pdx_groupby* gb);
int64_t pdx_groupby_num_rows(const pdx_groupby* gb);
/* uniqueKeys (GroupBy::unique(), src/group_by.h:52-55): G rows, first-occurrence order; validity marks the null key. */
int pdx_groupby_unique_keys(const pdx_groupby* gb, pdx_mut_column* out, void* stream);
/* Grouper::Consume output: uint32 group id per input row (out_ids: device pointer to num_rows uint32). */
int pdx_groupby_group_ids(pdx_groupby* gb, uint32_t* out_ids, void* stream);
/* out[i] = map[group_id(i)] for every input row: routes rows by a per-group attribute (global id, owner rank) in the
 * multi-GPU merge.  map: device pointer to G int64; out: device pointer to num_rows int64. */
int pdx_groupby_map_ids(pdx_groupby* gb, const int64_t* map, int64_t* out, void* stream);
/* first_row[g] = index of the first row of group g (device pointer to G int64) */
int pdx_groupby_first_rows(const pdx_groupby* gb, int64_t* out_rows, void* stream);
/* Grouper::MakeGroupings (src/dataframe.cpp:1546, 1562; what GroupBy::group / MakeSubDataFrame / apply walk, src/group_by.h:39-77):
 * out_rows (n int64, device) = the rows of group 0, then of group 1, ... each ascending; out_offsets (G + 1 int64, device): group g
 * owns out_rows[out_offsets[g] .. out_offsets[g + 1]).  Not part of pdx_groupby_create: only callers that walk groups pay for it. */
int pdx_groupby_groupings(pdx_groupby* gb, int64_t* out_rows, int64_t* out_offsets, void* stream);
/* Replaces GROUPBY_AGG(sum|min|max) and GROUPBY_NUMERIC_AGG(mean|count) (src/pd_core_macros.h:5-147, instantiated
 * src/dataframe.cpp:1512-1534): for every group, the scalar aggregate over the group's rows IN ROW ORDER.
 * `kinds`/`outs` have nk entries and are all computed from one grouped pass over `values` (sum/mean/count of the
 * headline query share one pass).  Output dtypes: SUM -> dtype of values (int64 wraps), MEAN -> FLOAT64, MIN/MAX ->
 * dtype of values, COUNT -> INT64.  outs[k].length must be >= G.  A group with no valid value yields a null
 * (validity required in that case) except COUNT. */
int pdx_groupby_agg(pdx_groupby* gb, const pdx_column* values, const int* kinds, int nk, pdx_mut_column* outs, void* stream);
/* The grouped layout of one column, built once and reused: what GroupBy's constructor does for every column of the frame
 * (processEach, src/dataframe.cpp:1539-1554: MakeGroupings + ApplyGroupings), so that gb.sum(c); gb.mean(c); gb.count(c)
 * (src/group_by.h:85-139 -- the reference has no multi-kind call) cost ONE value sort and ONE reduce instead of three of each.
 * pdx_groupby_bind registers `values` with the handle: the first pdx_groupby_agg of the column sorts it by group and keeps the
 * result (plus the per-group sum / count / min / max it computes) in the handle; every later pdx_groupby_agg whose `values` has
 * the same values pointer, offset, dtype and validity pointer is served from it.  Contract: the column's buffers stay alive and UNCHANGED until pdx_groupby_unbind /
 * pdx_groupby_destroy (Arrow buffers are immutable; the facades' GroupBy holds the frame).  Nothing is cached for columns that
 * were not bound.  values == NULL in unbind: every bound column.  The bound layouts of one handle are limited to
 * pdx_groupby_bind_limit bytes (default: a quarter of the device's memory, or PDX_BIND_MAX_BYTES): the least recently used
 * one is dropped first -- its next aggregation simply sorts again.  pdx_groupby_bound_bytes: device bytes held right now. */
int pdx_groupby_bind(pdx_groupby* gb, const pdx_column* values, void* stream);
int pdx_groupby_unbind(pdx_groupby* gb, const pdx_column* values);
int pdx_groupby_bind_limit(pdx_groupby* gb, size_t max_bytes);
int64_t pdx_groupby_bound_bytes(const pdx_groupby* gb);
/* The path the last pdx_groupby_agg on this handle took, as "key=value" words (diagnostic; tests assert it so that a moved
 * threshold fails a test instead of silently changing which kernels run):
 *   slots=dense|hash_lds|hash_part|hash_part2|hash_global|runs|bins   how keys became slots (pdx_groupby_create)
 *   sort=narrow:7+7|narrow_part:8+6|lsd:skip6|lsd|none[+finish]       the value sort (narrowing 4->2->1 byte keys, ...)
 *   layout=fused [side=<runs>] | full [skew=1]                        fused last digit vs fully sorted.  side: that many runs longer than
 *                                                                     2^19 rows (hot keys) were reduced from a side copy of their rows;
 *                                                                     skew: too many / too heavy long runs, the whole column was sorted on
 *   reducer=flr_reduce_dense|flr_reduce|flr_wave|seg_reduce|seg_reduce_nullable|none
 *   bound=0|1 [cache=fill|hit] */
int pdx_groupby_last_plan(const pdx_groupby* gb, char* buf, size_t buf_len);
/* GroupBy::quantile (src/group_by.h:123-124, src/dataframe.cpp:1867-1931): see "exact quantiles" above. */
int pdx_groupby_quantile(pdx_groupby* gb, const pdx_column* values, const double* q, int nq, int interpolation,
                         int skip_nulls, int64_t min_count, pdx_mut_column* outs /* nq columns of >= G rows */, void* stream);

/* ---------------------------------------------------------------- value frequencies
 * pdx_mode replaces CallFunction("mode", {array}, ModeOptions{n, skip_nulls, min_count}) reached from NDFrame::mode (src/ndframe.h:63-66, 255,
 * src/ndframe.cpp:177-197); pdx_groupby_mode is what GroupBy::mode (src/group_by.h:126-127, src/dataframe.cpp:1808-1865) intends: Arrow's mode
 * with default options over every group's rows; pdx_groupby_sizes is the counts half of Series::value_counts (src/dataframe.cpp:1093-1100),
 * beside pdx_groupby_unique_keys.  Semantics = Arrow C++ 25.0.0 (tests/golden/mode_golden.npz):
 *   - the result is the k = min(n, number of distinct values) most frequent valid values as (mode, count) pairs, ordered by count descending,
 *     ties by value ascending.  Nulls take no part.
 *   - floats: -0.0 == 0.0 is one value (their counts add); every NaN of any sign or payload is one value, sorts above +inf in the tie order,
 *     takes part like any other value and is returned as the canonical quiet NaN (0x7ff8000000000000 / 0x7fc00000).  The zero returned from a
 *     column that holds both zeros is the one that comes first in ROW order (pdx_quantile's convention; Arrow returns whichever zero its
 *     unstable sort left first).
 *   - the result is empty (k = 0) when there is no valid value, when skip_nulls == 0 and the column holds a null, or when fewer than
 *     min_count rows are valid (NaN rows count as valid).
 *   - n <= 0: PDX_INVALID "ModeOptions::n must be strictly positive", before anything is launched.
 *   - a: PDX_INT64, PDX_UINT64, PDX_FLOAT64, PDX_INT32, PDX_FLOAT32, PDX_BOOL (false < true).  PDX_TIMESTAMP_NS returns PDX_NOT_IMPLEMENTED
 *     "Function 'mode' has no kernel matching input types (timestamp[ns])".
 * pdx_mode: any offset, validity at any bit offset, null_count -1; at most 2^31-1 rows (PDX_NOT_IMPLEMENTED beyond).  out_modes->dtype ==
 * a->dtype, out_counts->dtype == PDX_INT64, both capacities >= min(n, a->length); anything else is PDX_INVALID before a launch.  On return
 * both lengths are k, null_count 0 (validity may be NULL, it is not written); rows and bytes beyond k are untouched (bool modes: bits
 * beyond k).  Synchronises `stream` like pdx_aggregate (k is host-visible); deterministic (same bits on any stream / run).
 * Two paths behind one first read (valid rows, smallest / largest value): bool and integer columns whose max - min + 1 <= 8192 are counted
 * (a second read into a workgroup-private LDS histogram); everything else is sorted (pdx_argsort / pdx_sort_indices), the runs of equal
 * values are marked and compacted.  pdx_mode_last_plan (diagnostic, this thread's last pdx_mode; tests assert it so that a moved threshold
 * fails a test): "path=count bins=<threshold> width=<max - min + 1>" | "path=sort runs=<distinct values>" | "path=bool" | "path=empty".
 * pdx_groupby_mode: handles from pdx_groupby_create / pdx_resample_create / pdx_downsample_create; values PDX_INT64 / PDX_UINT64 /
 * PDX_FLOAT64 (others: PDX_NOT_IMPLEMENTED naming the dtype); outputs of >= G rows, the values' dtype and PDX_INT64.  n = 1, skip_nulls,
 * min_count 0 per group.  A group without a valid value gets a null mode (validity bit clear, value bytes zero) and count 0;
 * out_modes->validity is required when such a group exists (PDX_INVALID otherwise: known only after the groups have been reduced,
 * so the output buffers have been written and both outputs come back with length 0); null_count is exact.  Neither the bound-column cache
 * nor pdx_groupby_last_plan is touched.
 * pdx_groupby_sizes: the rows of every group in group-id order, the null key's group included (out_sizes: G int64, device).  Served from
 * the sizes the handle holds (a COUNT of a column without nulls leaves them there); a handle that does not hold them yet takes them from
 * its segment boundaries or computes them through that same COUNT (which reads no value column) and keeps them: later calls, and later
 * COUNTs of columns without nulls, copy them. */
int pdx_mode(const pdx_column* a, int64_t n, int skip_nulls, int64_t min_count, pdx_mut_column* out_modes, pdx_mut_column* out_counts, void* stream);
int pdx_mode_last_plan(char* buf, size_t buf_len);
int pdx_groupby_mode(pdx_groupby* gb, const pdx_column* values, pdx_mut_column* out_modes, pdx_mut_column* out_counts, void* stream);
int pdx_groupby_sizes(pdx_groupby* gb, int64_t* out_sizes /* G int64, device */, void* stream);

/* ---------------------------------------------------------------- lookups: is_in / index_in, index, argmin / argmax, dictionary_encode
 * Replace CallFunction("is_in" | "index_in", {array}, SetLookupOptions{value_set, skip_nulls}) (Series::is_in / index_in, src/series.cpp:632-640),
 * CallFunction("index", {array}, IndexOptions{value}) and the index(min()) / index(max()) built on it (NDFrame::index / argmin / argmax,
 * src/ndframe.h:276-282; Series::idxMin / idxMax, src/series.cpp:164-172; DataFrame::idxMin / idxMax, src/dataframe.cpp:496-512) and
 * DictionaryEncode (Series::dictionary_encode, src/series.cpp:341).  Semantics = Arrow C++ 25.0.0, bit for bit (tests/golden/lookup_golden.npz).
 * Common to all: a: PDX_INT64, PDX_UINT64, PDX_TIMESTAMP_NS, PDX_FLOAT64, PDX_INT32, PDX_FLOAT32; PDX_BOOL returns PDX_NOT_IMPLEMENTED naming the
 * dtype.  Any offset, validity at any bit offset, null_count -1, a column without validity is all valid, int64 lengths; an empty input gives
 * PDX_OK and length 0; rows, bytes and bits of an output beyond the result length are untouched; value bytes under a null row are zero;
 * deterministic.  Every refusal happens before anything is launched.
 *
 * pdx_is_in / pdx_index_in: values match by BIT PATTERN (Arrow's memo table): 0.0 and -0.0 differ, NaNs of another sign or payload differ.
 *   value_set: the dtype of `a` (PDX_INVALID otherwise: Arrow would cast the set, the facades do where pdx_cast is exact), at most 2^31-1
 *   entries, duplicates and nulls allowed.  pdx_is_in: out PDX_BOOL, never null (validity not touched, null_count 0).  pdx_index_in: out
 *   PDX_INT32 = the position of the value's FIRST occurrence in value_set, null where there is none (out->validity is required for a non-empty
 *   input; null_count exact: it is read back, the call's only host wait -- pdx_is_in is asynchronous).  A null row: with skip_nulls == 0 it
 *   matches the set's first null (true / its position) when the set holds one; otherwise false / null.  An empty set gives all false / null.
 *   The set is deduplicated into an open-addressing table at load factor <= 0.5; sets of up to 2048 entries are probed from a copy in every
 *   workgroup's LDS (PDX_LOOKUP_LDS_MAX=<entries> lowers that bound), larger ones where they were built.  pdx_lookup_last_plan (diagnostic,
 *   this thread's last pdx_is_in / pdx_index_in; tests assert it): "plan=lds|global|empty set_size=<entries> slots=<table slots>".
 * pdx_index: *out_row (host) = the first valid row with a[row] == value under IEEE == (0.0 finds -0.0), -1 when there is none; a null or NaN
 *   value (value == NULL included) gives -1 and is not an error.  value->dtype must equal a's (PDX_INVALID), 4-byte values as pdx_scalar
 *   documents; a value that a 4-byte column cannot hold (an integer outside int32, a double that is no float32) gives -1.  One pass that
 *   stops behind the first match; synchronises `stream`.
 * pdx_arg_extreme: out_rows[c] (host, ncols) = index(min(cols[c])) (is_max == 0) / index(max(cols[c])) in ONE read of every column: the row of
 *   the smallest / largest valid value, the first such row on ties (0.0 == -0.0 tie); NaN never wins over a number; -1 when the column is
 *   empty, all null, or its valid values are all NaN (Arrow's min is NaN then, which index never finds).  1 .. 65535 columns, which may
 *   differ in dtype and length; one launch for all of them plus a small final kernel; synchronises `stream`.
 * pdx_dictionary_encode: out_dict (a's dtype, capacity >= a->length, no nulls; its length is set on return) = the distinct bit patterns of
 *   the valid rows in first-occurrence order; out_codes (PDX_INT32, >= a->length rows) = each row's position in it, null for a null row
 *   (null_encoding = mask: a null takes no dictionary slot; out_codes->validity is required when `a` can hold a null).  Built on the
 *   group-by handle over the 8-byte bit image (a 4-byte column is zero-extended first), whose limit it inherits: at most 2^31-1 rows
 *   (PDX_NOT_IMPLEMENTED beyond).  Synchronises `stream`. */
int pdx_is_in(const pdx_column* a, const pdx_column* value_set, int skip_nulls, pdx_mut_column* out, void* stream);
int pdx_index_in(const pdx_column* a, const pdx_column* value_set, int skip_nulls, pdx_mut_column* out, void* stream);
int pdx_lookup_last_plan(char* buf, size_t buf_len);
int pdx_index(const pdx_column* a, const pdx_scalar* value /* NULL: the null scalar */, int64_t* out_row /* host */, void* stream);
int pdx_arg_extreme(int is_max, const pdx_column* cols, int ncols, int64_t* out_rows /* host, ncols */, void* stream);
int pdx_dictionary_encode(const pdx_column* a, pdx_mut_column* out_codes, pdx_mut_column* out_dict, void* stream);

/* ---------------------------------------------------------------- join: hash equi-join of two frames on one key column
 * The reference's README lists "merging and joining" and implements neither (its column-wise pd::concat aligns on UNIQUE labels only), so
 * there is no call site to cite: the facades' DataFrame::merge / join are built on these calls.  The result size depends on the data, so the
 * join lives in a handle: pdx_join_create matches the keys and knows the row count, pdx_join_indices writes the result as two PDX_INT64
 * columns of TAKE INDICES into the left and the right frame, made to be fed to pdx_take (whose null index gives a null row).
 *   keys    : one column per side, PDX_INT64, PDX_UINT64, PDX_TIMESTAMP_NS or PDX_INT32, the same dtype on both sides (PDX_INVALID
 *             otherwise: cast one side first).  PDX_FLOAT64, PDX_FLOAT32 and PDX_BOOL return PDX_NOT_IMPLEMENTED naming the dtype (no rule
 *             for float equality is decided here).  Any offset, validity at any bit offset, null_count -1, a column without validity is
 *             all valid.  At most 2^31-1 rows per side (the group-by handle's limit; PDX_NOT_IMPLEMENTED beyond); the OUTPUT row count is
 *             an int64 and may exceed 2^31.  An empty side is not an error.  Every refusal happens before anything is launched.
 *   match   : keys match by value.  A NULL KEY MATCHES NOTHING, not even another null: the rule of Arrow's hash join (Acero, with its
 *             default JoinKeyCmp::EQ) and of SQL.  pandas' merge differs: it matches null keys with each other.
 *   how     : pdx_join_how.  The row order is fully defined:
 *             INNER  rows ordered by left row; the matches of one left row by ascending right row.
 *             LEFT   the same, and a left row without a match (a null key included) appears once, with a NULL right index.
 *             OUTER  LEFT, followed by the right rows that no left row matched (null-key rows among them) in right row order, each with
 *                    a NULL left index.
 *             SEMI   the left rows with at least one match, ANTI those without (null keys included), each once, in left order; there is
 *                    no right output.
 *             (A RIGHT join is a LEFT join with the sides swapped; the facades do that.)
 *   outputs : pdx_join_indices: out_left / out_right are PDX_INT64 of capacity >= pdx_join_rows; a smaller capacity, another dtype or a
 *             missing buffer returns PDX_INVALID before anything is written.  out_right->validity is required unless how is INNER,
 *             out_left->validity for OUTER (PDX_INVALID otherwise, whether or not a null occurs); where a validity buffer is given and no
 *             null can occur its bits are set.  For SEMI / ANTI out_right must be NULL (PDX_INVALID otherwise: there is nothing to
 *             write).  On return both lengths are the row count and null_count is exact; value bytes under a null index are zero; rows,
 *             bytes and validity bits beyond the result length are untouched.  Deterministic: the same bytes on any stream and run.
 *             pdx_join_indices may be called more than once on a handle.
 *   how it runs: the right side is grouped by the group-by handle (distinct keys in first-occurrence order, pdx_groupby_groupings' rows of
 *             every key in row order; an int32 key is zero-extended to 8 bytes first); the distinct keys go into the lookups'
 *             open-addressing table (load factor <= 0.5), probed from a copy in LDS up to 2048 distinct keys (PDX_LOOKUP_LDS_MAX lowers
 *             the bound) and in global memory beyond; one pass over the left keys writes every row's match list and output count; an
 *             exclusive scan gives every left row its first output row.  pdx_join_create reads the totals back once (its only host wait
 *             beside those of the group-by calls) and, for SEMI / ANTI and the OUTER tail, compacts the selected rows.
 *             pdx_join_indices is asynchronous on `stream`: its kernel is output-parallel -- a workgroup owns 2048 consecutive output
 *             rows and finds the left rows that cover them by a search of the offsets -- so one hot key is written by as many workgroups
 *             as its matches fill, and left rows without output cost nothing.  The handle holds 16 bytes per left row and 8 per right row.
 *   pdx_join_last_plan (diagnostic; tests assert it): "plan=lds|global|empty build_rows=<right rows> distinct=<groups of the right key, the
 *             null key counting as one> out_rows=<pdx_join_rows>"; empty: the right side has no rows. */
typedef enum pdx_join_how { PDX_JOIN_INNER = 0, PDX_JOIN_LEFT = 1, PDX_JOIN_OUTER = 2, PDX_JOIN_SEMI = 3, PDX_JOIN_ANTI = 4 } pdx_join_how;
typedef struct pdx_join pdx_join;
int pdx_join_create(const pdx_column* left_key, const pdx_column* right_key, int how, void* stream, pdx_join** out);
int pdx_join_rows(const pdx_join* j, int64_t* out_rows /* host */);
int pdx_join_indices(pdx_join* j, pdx_mut_column* out_left, pdx_mut_column* out_right /* NULL for SEMI / ANTI */, void* stream);
int pdx_join_last_plan(const pdx_join* j, char* buf, size_t buf_len);
int pdx_join_destroy(pdx_join* j);

/* ---------------------------------------------------------------- exact multi-GPU fp64 sum (partial-tree exchange)
 * The reference's per-group sum is Arrow's pairwise tree over the group's rows in GLOBAL row order; with row-range shards a
 * rank holds the global ranks [P, P+c) of a group.  Instead of shipping its rows to the group's owner, a rank ships
 *   - the raw values of the (at most two) 16-value leaves it shares with its neighbours ("fragments"), and
 *   - one node per maximal ALIGNED power-of-two block of the leaves that lie completely inside its range,
 * as records (key = global_gid * 64 + code; code 0 = one row of a leaf begun on a lower rank, 1..28 = a tree node of level code - 1,
 * 32 + k = the first k rows of a leaf as their sequential sum).  The owner replays the records of a
 * group in (rank, emission) order through Arrow's binary counter: bit-identical to the single-process result, with
 * O(32 + 2 log c) instead of c values per group and rank.
 *
 * pdx_groupby_group_values : stable sort of a non-null float64 column by group; the handle caches the grouped values.
 * pdx_grouped_counts       : rows per group (G int64, group-id order).
 * pdx_grouped_partial_plan : number of records given prefix[g] = rows of group g held by lower ranks (G int64, group-id order);
 *                            order (optional, G int64) = local group ids in record EMISSION order -- pass the ids sorted by global
 *                            group id and the records come out already partitioned by owner rank (no routing pass).
 * pdx_grouped_partial_fill : writes the records; gid_map[g] = global group id of local group g.
 * pdx_replay_partials      : owner side: records for global ids [gid_lo, gid_lo + n_own) in (source rank, emission) order ->
 *                            out_sum[gid - gid_lo].  Every owned id must have at least one record. */
typedef struct pdx_grouped pdx_grouped;
int pdx_groupby_group_values(pdx_groupby* gb, const pdx_column* values, void* stream, pdx_grouped** out);
int pdx_grouped_destroy(pdx_grouped* g);
int pdx_grouped_counts(pdx_grouped* g, int64_t* out_counts, void* stream);
int pdx_grouped_partial_plan(pdx_grouped* g, const int64_t* prefix, const int64_t* order, int64_t* out_total, void* stream);
int pdx_grouped_partial_fill(pdx_grouped* g, const int64_t* gid_map, int64_t* rec_key /* may be null: values only */, double* rec_val, void* stream);
/* cuts[d], d = 0..world (device): where the records of owner d's groups -- global ids [G * d / world, G * (d + 1) / world) -- begin in this
 * rank's record stream (emitted in global-id order: pass `order` to the plan).  With the rows every rank holds of every group known to all
 * ranks, the codes of the records follow from (rows on lower ranks, own rows): only the values need to travel. */
int pdx_grouped_record_cuts(pdx_grouped* g, const int64_t* gid_map, int64_t num_global_groups, int world, int64_t* cuts, void* stream);
int pdx_replay_partials(const int64_t* rec_key, const double* rec_val, int64_t m, int64_t gid_lo, int64_t n_own, double* out_sum, void* stream);

/* ---------------------------------------------------------------- resample
 * Replaces pd::resample<> / makeGroupInfo / generate_bins_dt64 / GroupInfo::downsample + the Resampler's GroupBy on
 * the per-row labels (src/resample.h:19-43,91-122; src/resample.cpp:11-83,85-178,202-295; src/core.cpp:308-331;
 * src/group_by.h:255-299).  ts: sorted PDX_TIMESTAMP_NS without nulls.  The handle behaves like a pdx_groupby whose
 * unique keys are the labels of the NON-EMPTY bins (empty bins vanish, as in the reference).
 * Errors (PDX_INVALID): "Values falls before first bin", "Values falls after last bin",
 * "upSampling is not implemented.", unsorted input.  Row-range shards of one axis: see PDX_ORIGIN_SHARD.
 * Lifetime: the handle keeps the POINTER to ts' values (pdx_resample_row_labels reads them again): the caller's timestamp
 * buffer must stay alive and unchanged until pdx_groupby_destroy. */
int pdx_resample_create(const pdx_column* ts, int64_t freq_ns, int closed_right, int label_right, int origin_type,
                        int64_t origin_custom_ns, int64_t offset_ns, void* stream, pdx_groupby** out);
/* The grid alone (host arithmetic, no GPU): first bin edge and number of bins of an axis with extremes tmin / tmax -- adjustDatesAnchored
 * + date_range (src/resample.cpp:85-178, src/core.cpp:308-331), with the reference's errors.  pdx_resample_create uses it; so does
 * the sharded resample, where every rank must bin on the WHOLE axis' grid. */
int pdx_resample_grid(int64_t tmin, int64_t tmax, int64_t freq_ns, int closed_right, int origin_type, int64_t origin_custom_ns, int64_t offset_ns,
                      int64_t* first_edge, int64_t* num_bins);
/* per-row labels (GroupInfo::downsample): device pointer to num_rows int64 */
int pdx_resample_row_labels(pdx_groupby* gb, int64_t* out_labels, void* stream);

/* DataFrame::downsample's grouping in one call (reference src/dataframe.cpp:1265-1290: arrow::compute::CeilTemporal /
 * FloorTemporal(m_index, RoundTemporalOptions(multiple, unit, week_starts_monday, false, calendar_based_origin)), for the
 * M / W / Y / Q and *E rules Subtract(one day), then Resampler(GroupBy) keyed on the rounded index).  The handle behaves like
 * pdx_groupby_create(pdx_round_temporal(ts) + label_shift_ns): unique keys = the distinct rounded labels (+ shift) in
 * first-occurrence order, null timestamps form one null group.  ceil_mode / unit / multiple / week_starts_monday /
 * calendar_based_origin as in pdx_round_temporal; label_shift_ns is added to every label (e.g. -86400e9).
 * When ts has no nulls and its rounded labels never descend (a sorted axis) the groups are found as runs of equal labels in
 * ONE pass over ts -- the rounded column is never materialised or hashed; any other input takes pdx_round_temporal +
 * pdx_groupby_create internally.  Same results either way.  The handle keeps no pointer into ts. */
int pdx_downsample_create(const pdx_column* ts, int64_t multiple, int unit, int ceil_mode, int week_starts_monday,
                          int calendar_based_origin, int64_t label_shift_ns, void* stream, pdx_groupby** out);

/* ---------------------------------------------------------------- temporal rounding: DataFrame::downsample
 * Replaces arrow::compute::FloorTemporal / CeilTemporal(m_index, RoundTemporalOptions(freq_value, getCalendarUnit(freq_unit[0]),
 * weekStartsMonday, ceil_is_strictly_greater = false, calendar_based_origin = startEpoch)) at src/dataframe.cpp:1271-1276
 * (unit letters: src/core.cpp:135-172).  ts: PDX_TIMESTAMP_NS (no time zone); out: PDX_TIMESTAMP_NS of the same length, null where
 * ts is null.  ceil_mode != 0: CeilTemporal (closed_label_right), else FloorTemporal.  Semantics follow Arrow C++ 25.0.0:
 * floors go toward -inf; calendar_based_origin counts the multiples from the floor to the next larger unit (day: the 1st of the
 * month, week: the first week of the year) instead of from the epoch; month / quarter ceil is always floor + multiple.
 * The reference then subtracts one day for M / W / Q rules (src/dataframe.cpp:1277-1285: pdx_binary(PDX_SUB) on the int64 view)
 * and keys a Resampler's GroupBy on the result (pdx_groupby_create; the labels need not be sorted). */
typedef enum pdx_calendar_unit {
  PDX_UNIT_NANOSECOND = 0, PDX_UNIT_MICROSECOND = 1, PDX_UNIT_MILLISECOND = 2, PDX_UNIT_SECOND = 3, PDX_UNIT_MINUTE = 4,
  PDX_UNIT_HOUR = 5, PDX_UNIT_DAY = 6, PDX_UNIT_WEEK = 7, PDX_UNIT_MONTH = 8, PDX_UNIT_QUARTER = 9,
  PDX_UNIT_YEAR = 10 /* pdx_temporal_between only; rounding to years returns PDX_NOT_IMPLEMENTED */
} pdx_calendar_unit;
/* ceil_mode (the rounding mode): PDX_ROUND_FLOOR / PDX_ROUND_CEIL as above (every value other than 0 and 2 is a ceil, as it always
 * was); PDX_ROUND_NEAREST is Arrow's round_temporal
 * (DateTimeLike::round, src/series.cpp:672-685): of the floor f and the ceil c of t under the same options it returns c when
 * t - f >= c - t, else f -- a tie goes up; month / quarter compare the distances in nanoseconds to the first instants of the two
 * months (pinned by tests/golden/temporal_golden.npz).  ceil_is_strictly_greater is always false (the facades refuse true). */
typedef enum pdx_round_mode { PDX_ROUND_FLOOR = 0, PDX_ROUND_CEIL = 1, PDX_ROUND_NEAREST = 2 } pdx_round_mode;
int pdx_round_temporal(int ceil_mode, const pdx_column* ts, int64_t multiple, int unit, int week_starts_monday, int calendar_based_origin,
                       pdx_mut_column* out, void* stream);

/* ---------------------------------------------------------------- the dt accessor: calendar components and *_between
 * Replaces the Arrow temporal kernels behind Series::dt() (DateTimeLike, src/datetimelike.h; src/series.cpp:1387-1487,
 * src/dataframe.cpp:904-913).  Input is always PDX_TIMESTAMP_NS without a time zone (anything else: PDX_INVALID); all divisions floor
 * toward -inf (-1 ns is 1969-12-31 23:59:59.999999999); results are bit-identical to Arrow C++ 25 (tests/golden/temporal_golden.npz).
 *
 * pdx_temporal_components: ONE read of ts produces nc columns, 1 <= nc <= 8 (PDX_INVALID otherwise): 8 B read + 8 x nc B written
 * per row.  components[c] is a pdx_temporal_component, outs[c] the caller's buffer for it, of at least ts->length rows and of the
 * component's dtype (PDX_INVALID on a mismatch):
 *   PDX_INT64  : YEAR, MONTH (1-12), DAY (1-31), DAY_OF_WEEK (0 = Monday .. 6 = Sunday: Arrow's default DayOfWeekOptions, which
 *                is what the reference passes), DAY_OF_YEAR (1-366), HOUR, MINUTE, SECOND, MILLISECOND / MICROSECOND / NANOSECOND
 *                (0-999 each), QUARTER (1-4), ISO_WEEK, ISO_YEAR, ISO_DAY_OF_WEEK (1 = Monday .. 7), US_WEEK, US_YEAR (weeks from
 *                Sunday, week 1 holds 4 January), WEEK (week_opts)
 *   PDX_BOOL   : IS_LEAP_YEAR (bit-packed, stored in whole 64-row words: the values buffer needs 8-byte alignment and
 *                (length + 7) / 8 bytes)
 *   PDX_FLOAT64: SUBSECOND = (nanoseconds since the last whole second) / 1e9, one IEEE division
 * week_opts is arrow::compute::WeekOptions for WEEK (NULL: {1, 0, 0} = the ISO week); ISO_WEEK is {1, 0, 0}, US_WEEK {0, 0, 0}.
 * year_month_day() is {YEAR, MONTH, DAY} and iso_calendar() {ISO_YEAR, ISO_WEEK, ISO_DAY_OF_WEEK} in one call.  Nulls propagate:
 * every output with a validity buffer receives the input's validity (an input with nulls needs one on every output); length 0 is
 * PDX_OK.
 *
 * pdx_temporal_between: the number of `unit` boundaries crossed from a to b, floor(b, unit) - floor(a, unit) counted in units ->
 * PDX_INT64, null where either side is null.  unit: any pdx_calendar_unit but MONTH (Arrow has no months_between): YEAR and QUARTER
 * difference the calendar fields, WEEK counts Mondays (Arrow's default, which the reference uses).  Unequal lengths: PDX_INVALID
 * "Array arguments must all be the same length".  A difference that overflows int64 (only NANOSECOND between instants more than
 * 292 years apart can) wraps: outside the contract.
 *
 * Out of scope, refused by the facades with PDX_NOT_IMPLEMENTED naming the method: is_dst and anything that needs a time zone;
 * strftime / strptime; day_time_interval_between, month_interval_between, month_day_nano_interval_between (no interval dtypes). */
typedef enum pdx_temporal_component {
  PDX_TC_YEAR = 0, PDX_TC_MONTH = 1, PDX_TC_DAY = 2, PDX_TC_DAY_OF_WEEK = 3, PDX_TC_DAY_OF_YEAR = 4, PDX_TC_HOUR = 5, PDX_TC_MINUTE = 6,
  PDX_TC_SECOND = 7, PDX_TC_MILLISECOND = 8, PDX_TC_MICROSECOND = 9, PDX_TC_NANOSECOND = 10, PDX_TC_QUARTER = 11, PDX_TC_ISO_WEEK = 12,
  PDX_TC_ISO_YEAR = 13, PDX_TC_ISO_DAY_OF_WEEK = 14, PDX_TC_US_WEEK = 15, PDX_TC_US_YEAR = 16, PDX_TC_WEEK = 17,
  PDX_TC_IS_LEAP_YEAR = 18, PDX_TC_SUBSECOND = 19
} pdx_temporal_component;
typedef struct pdx_week_options {
  int32_t week_starts_monday;
  int32_t count_from_zero;
  int32_t first_week_is_fully_in_year;
} pdx_week_options;
int pdx_temporal_components(const pdx_column* ts, const int* components, int nc, const pdx_week_options* week_opts, pdx_mut_column* outs,
                            void* stream);
int pdx_temporal_between(int unit, const pdx_column* a, const pdx_column* b, pdx_mut_column* out, void* stream);

/* ---------------------------------------------------------------- index alignment (the callers' slow path)
 * Binary operators on Series with UNEQUAL indexes go through Series::broadcast (src/series.cpp:212-227):
 * Concatenate(index_a, index_b) -> Unique -> array_sort_indices(ascending) -> Take, then Series::reindex of both operands
 * (src/series.cpp:1255-1309: std::unordered_map label -> LAST position, absent labels -> null).
 * pdx_index_union: the distinct labels of a and b (same dtype: int64 / uint64 / timestamp[ns], no nulls), sorted ascending
 *   (sort != 0: Series::broadcast) or in first-occurrence order (sort == 0: Series::union_, src/series.cpp:782-798, used by the
 *   column-wise concat, src/concat.cpp:78-88, 192-244).  out: same dtype, capacity a.length + b.length; out->length is set.
 * pdx_index_intersection: Series::intersection (src/series.cpp:763-780): the labels of a that occur in b, one per distinct
 *   label, ordered by their (last) position in a.  out: capacity a.length.
 * pdx_reindex_indices: for every label of new_index its LAST position in old_index as int64 take indices with a validity
 *   bitmap (absent label -> null index); feed it to pdx_take, whose null indices produce null rows (== AppendNull). */
int pdx_index_union(const pdx_column* a, const pdx_column* b, int sort, pdx_mut_column* out, void* stream);
int pdx_index_intersection(const pdx_column* a, const pdx_column* b, pdx_mut_column* out, void* stream);
int pdx_reindex_indices(const pdx_column* old_index, const pdx_column* new_index, pdx_mut_column* out_idx, void* stream);

/* ---------------------------------------------------------------- sort (sort / argsort / n_largest / n_smallest)
 * Series::argsort (src/series.cpp:864-868) and Series::sort (978-992: Take of values and index by the same indices; n_largest /
 * n_smallest, 1211-1229, are sort + Slice) call CallFunction("array_sort_indices", ArraySortOptions{order}).  Semantics pinned
 * against Arrow 25.0.0: STABLE in both orders (equal values keep their row order; -0.0 == 0.0), NaN behind every number and
 * nulls behind the NaNs in BOTH orders.  col: int64 / uint64 / float64 / timestamp[ns], <= 2^31-1 rows; out_indices: PDX_UINT64,
 * capacity col.length (the take indices; feed them to pdx_take). */
int pdx_argsort(const pdx_column* col, int ascending, pdx_mut_column* out_indices, void* stream);

/* DataFrame::argsort (src/dataframe.cpp:1073-1091): CallFunction("sort_indices", SortOptions{one SortKey per field}) -- a STABLE
 * lexicographic sort by several columns.  Semantics pinned against Arrow 25.0.0 (default null placement): per key first the class,
 * numbers < NaN < null in BOTH orders (descending reverses only the numbers), then the value (-0.0 == 0.0: such a tie goes on to the
 * next key); rows that tie on every key keep their row order.
 *   keys: 1 .. PDX_SORT_MAX_KEYS columns of equal length (<= 2^31-1 rows), int64 / uint64 / float64 / timestamp[ns] / int32 / float32
 *   (bool: PDX_NOT_IMPLEMENTED), each with its own offset and validity; descending: nkeys flags, NULL = all ascending;
 *   out_indices: PDX_UINT64, capacity >= the row count (the take indices; feed them to pdx_take).
 * The keys are sorted as range-compressed composite keys: per key a value field of bit_length(max - min) bits and, only when the
 * column has a NaN or null row, a 2-bit class field above it; the fields of all keys, last key least significant, are packed without
 * splitting a field into rounds of at most 64 bits, each round one stable radix sort.  info (optional) reports what ran: rounds = the
 * composite sorts (0 when every field has width 0: the result is 0 .. n-1), key_bits = the sum of all field widths, passes = the 8-bit
 * radix passes issued. */
#define PDX_SORT_MAX_KEYS 16
typedef struct pdx_sort_info {
  int32_t rounds;
  int32_t key_bits;
  int32_t passes;
  int32_t reserved;
} pdx_sort_info;
int pdx_sort_indices(const pdx_column* keys, int nkeys, const int* descending, pdx_mut_column* out_indices, pdx_sort_info* info, void* stream);

/* ---------------------------------------------------------------- top-k and partition (Series::n_largest / n_smallest / nth_element)
 * pdx_select_k: the first min(k, col.length) entries of what pdx_argsort(col, ascending) writes, bit for bit, without sorting the column
 * (the reference's n_largest / n_smallest, src/series.cpp:1211-1229, are sort + Slice).  So: STABLE in both orders (equal values keep
 * their row order; -0.0 == 0.0), NaN rows behind every number and null rows behind the NaNs in BOTH orders; a k beyond the count of
 * numbers continues with the first NaN rows in row order, then the first null rows in row order.
 *   col: int64 / uint64 / float64 / timestamp[ns] / int32 / float32 (bool: PDX_NOT_IMPLEMENTED), <= 2^31-1 rows, offset and validity
 *   honoured; k < 0: PDX_INVALID; out_indices: PDX_UINT64 without validity, capacity >= min(k, length); its length is set to that value
 *   and nothing beyond it is written.
 * Plans (pdx_select_k_last_plan, diagnostic, this thread's last pdx_select_k: "plan=select|sort|empty k=... rows=... levels=..."):
 *   empty   k == 0 or an empty column: nothing is launched.
 *   select  the radix select of pdx_quantile finds the key T at the k-th place among the numbers (levels = histogram levels it took);
 *           one counting read, a scan and one writing read collect the rows that beat T and the first k - (their count) rows equal to
 *           T in row order (+ the first NaN / null rows when k exceeds the numbers); only those k (key, row) pairs are sorted.
 *   sort    k >= length, or k above the crossover fraction of the rows (a measured constant): one single-key
 *           pdx_sort_indices, the first k indices copied out.
 *   PDX_SELECT_K_PLAN=select|sort (environment, read per call) forces a plan wherever it is legal (select needs 0 < k < length).
 *
 * pdx_partition_nth: Series::nth_element (src/series.cpp:973-976, CallFunction("partition_nth_indices", PartitionNthOptions{pivot})).
 * DEVIATION, on purpose: Arrow's output is whatever std::nth_element left behind (its null rows are not even in row order), so this call
 * is NOT bit-identical to Arrow; it is defined by its own contract.  With m the count of numbers and p = min(pivot, m):
 *   - out_indices is a permutation of 0 .. length-1;
 *   - every number in places [0, p) is <= every number in places [p, m);
 *   - if pivot < m, the row at place pivot holds the value pdx_argsort(col, 1) puts at place pivot;
 *   - the NaN rows follow in places [m, m + nan), then the null rows;
 *   - the layout is deterministic: with T the key at rank min(pivot, m - 1) of the numbers (pivot >= m: the largest key), the rows with
 *     key < T in row order, the rows with key == T in row order, the rows with key > T in row order, the NaN rows in row order, the
 *     null rows in row order.
 * It runs the same select, one counting read and one scatter read, and sorts nothing.  pivot == length is legal (as in Arrow);
 * pivot < 0 or pivot > length: PDX_INVALID (Arrow happens to accept a negative pivot; that is not mirrored).  Same dtypes and limits as
 * pdx_select_k; out_indices: PDX_UINT64 without validity, capacity >= length. */
int pdx_select_k(const pdx_column* col, int64_t k, int ascending, pdx_mut_column* out_indices, void* stream);
int pdx_partition_nth(const pdx_column* col, int64_t pivot, pdx_mut_column* out_indices, void* stream);
int pdx_select_k_last_plan(char* buf, size_t buf_len);

/* ---------------------------------------------------------------- concat (rows)
 * Replaces arrow::ConcatenateTables + CombineChunksToBatch at src/concat.cpp:152-154 for same-dtype parts
 * (the all-gatherv merge of sharded results).  out->length must be >= sum of part lengths. */
int pdx_concat(const pdx_column* parts, int nparts, pdx_mut_column* out, void* stream);

/* ---------------------------------------------------------------- Arrow IPC streams <-> device columns
 * Replaces, for the column types of this path, DataFrame::readBinary (src/dataframe.cpp:754-791: ipc::RecordBatchStreamReader::Open
 * + ToRecordBatches, exactly ONE record batch) and DataFrame::toBinary (src/dataframe.cpp:726-752: ipc::MakeStreamWriter +
 * WriteRecordBatch(batch, custom metadata)).  A record batch body is the Arrow layout the kernels read, so reading is a parse of
 * the two flatbuffer messages on the host plus ONE host->device copy of the body; the columns are pointers into it.
 *   pdx_ipc_open     parse a stream held in HOST memory (no GPU needed); the blob must stay alive until pdx_ipc_load returns.
 *                    Column types: bool, (u)int8..64, float32/64, timestamp (any unit, time zone ignored), date64; narrow
 *                    numerics are widened to int64 / uint64 / float64 and timestamps scaled to nanoseconds on the device.
 *                    Anything else (strings, nested, dictionaries, compressed bodies): PDX_NOT_IMPLEMENTED naming the field.
 *   pdx_ipc_load     upload (one copy + the widening kernels); synchronises `stream`.
 *   pdx_ipc_column   the i-th column (device pointers owned by the frame until pdx_ipc_destroy; before pdx_ipc_load only dtype,
 *                    length and null_count are filled in).
 *   pdx_ipc_write    serialise equally long columns as one schema + one record batch (+ custom metadata key/value pairs:
 *                    metadata_kv holds 2 x nmeta strings) + end-of-stream.  columns_on_host != 0: the pdx_column pointers are
 *                    host memory.  *out_blob is malloc'ed by the library: release it with pdx_ipc_free_blob.
 * The index column convention (readBinary's `index` argument: pull the named column out, int64 -> timestamp[ns]) lives in the
 * facades. */
typedef struct pdx_ipc_frame pdx_ipc_frame;
int pdx_ipc_open(const void* blob, size_t size, pdx_ipc_frame** out);
int pdx_ipc_destroy(pdx_ipc_frame* frame);
int pdx_ipc_num_columns(const pdx_ipc_frame* frame);
int64_t pdx_ipc_num_rows(const pdx_ipc_frame* frame);
const char* pdx_ipc_column_name(const pdx_ipc_frame* frame, int i);
int pdx_ipc_num_metadata(const pdx_ipc_frame* frame);
const char* pdx_ipc_metadata_key(const pdx_ipc_frame* frame, int i);
const char* pdx_ipc_metadata_value(const pdx_ipc_frame* frame, int i);
int pdx_ipc_load(pdx_ipc_frame* frame, void* stream);
int pdx_ipc_column(const pdx_ipc_frame* frame, int i, pdx_column* out);
int pdx_ipc_write(const pdx_column* cols, const char* const* names, int ncols, const char* const* metadata_kv, int nmeta, int columns_on_host,
                  void* stream, void** out_blob, size_t* out_size);
int pdx_ipc_free_blob(void* blob);

/* ---------------------------------------------------------------- row-range shards across the GPUs of one node
 * One process per GPU; every rank holds a row range of the frame, ranks in row order.  The reference has no distributed code: the
 * contract is the SINGLE-process result of df.group_by(key).sum / mean / count (src/group_by.h:85-139, src/pd_core_macros.h:5-147)
 * and of pd::concat (src/concat.cpp:116-190), bit for bit.  librccl is opened at run time and called directly (ncclAllGather,
 * grouped ncclSend / ncclRecv over xGMI): no python, no torch in the loop -- a C++ host shards through this same header.
 *   pdx_dist_unique_id   rank 0: 128 bytes (an ncclUniqueId) to hand to the other ranks by whatever channel the host has.
 *   pdx_dist_init        ncclCommInitRank on the calling thread's current device (after pdx_init(device)).
 *   pdx_dist_init_custom the same orchestration over the caller's own transport: two primitives on DEVICE buffers, ordered on the
 *                        given stream -- all_gather (every rank contributes `bytes` bytes, received in rank order) and
 *                        all_to_all_v (byte ranges send_off/send_bytes[peer] of `send` go to peer, recv_off/recv_bytes[peer] of `recv`
 *                        come from peer).  Return 0 for success.  (tests: three processes sharing one GPU, where RCCL refuses
 *                        duplicate devices.)
 *   pdx_dist_groupby_sum_mean_count   keys / values: this rank's shard (values: float64 without nulls); row_offset: index of the
 *                        shard's first row in the whole frame.  Partial-tree exchange: the global first-occurrence dictionary from
 *                        an all-gather(v) of the local uniques, the per-group row counts all-gathered, then per group and rank only the
 *                        boundary-leaf fragments + aligned subtree nodes travel (ONE all-to-all(v)) and the owners replay them through
 *                        Arrow's binary counter.  Every rank ends with the FULL result (G groups in first-occurrence order).
 *   pdx_dist_groupby_fetch   copies of the result columns (any pointer may be NULL; capacity >= num_groups rows).
 *   pdx_dist_concat      all-gather(v) of one column's shards in rank order (values + validity).
 * PDX_DIST_FORCE_COLLECTIVES=1 keeps every collective on the wire at world size 1 (tests on a one-GPU box). */
typedef struct pdx_dist_transport {
  void* ctx;
  int (*all_gather)(void* ctx, const void* send, void* recv, size_t bytes, void* stream);
  int (*all_to_all_v)(void* ctx, const void* send, const size_t* send_off, const size_t* send_bytes, void* recv, const size_t* recv_off,
                      const size_t* recv_bytes, void* stream);
} pdx_dist_transport;
typedef struct pdx_dist pdx_dist;
typedef struct pdx_dist_groupby pdx_dist_groupby;
int pdx_dist_unique_id(void* out_id128);
int pdx_dist_init(const void* id128, int world, int rank, pdx_dist** out);
int pdx_dist_init_custom(const pdx_dist_transport* transport, int world, int rank, pdx_dist** out);
int pdx_dist_destroy(pdx_dist* d);
int pdx_dist_world(const pdx_dist* d);
int pdx_dist_rank(const pdx_dist* d);
int pdx_dist_groupby_sum_mean_count(pdx_dist* d, const pdx_column* keys, const pdx_column* values, int64_t row_offset, void* stream,
                                    pdx_dist_groupby** out);
int64_t pdx_dist_groupby_num_groups(const pdx_dist_groupby* g);
int64_t pdx_dist_groupby_num_records(const pdx_dist_groupby* g);
int pdx_dist_groupby_fetch(const pdx_dist_groupby* g, pdx_mut_column* keys, int64_t* first_rows, double* sums, double* means, int64_t* counts,
                           void* stream);
int pdx_dist_groupby_destroy(pdx_dist_groupby* g);
int pdx_dist_concat(pdx_dist* d, const pdx_column* part, pdx_mut_column* out, void* stream);
/* The order-free kinds over row-range shards -- df.group_by(key).{min, max, count}(col) and the sum of an int64 column
 * (src/group_by.h:85-139, GROUPBY_AGG / GROUPBY_NUMERIC_AGG src/pd_core_macros.h:5-147): every rank reduces its shard, the results go into
 * dense per-group partial arrays indexed by GLOBAL group id, ONE all-gather and a fold in rank order finish (SURVEY 8e 3a's
 * reduce-by-key; int64 sums wrap, min keeps the first of ties, max the first -- the last when the group holds a null on any rank).
 * Values may carry nulls.  kinds: PDX_AGG_MIN / PDX_AGG_MAX / PDX_AGG_COUNT, PDX_AGG_SUM for int64 values; float64 sums / means are order
 * dependent and stay with pdx_dist_groupby_sum_mean_count.  One corner is not Arrow's: a maximum that is a tie of +0.0 and -0.0 ACROSS
 * ranks in a group that has a null on one rank and its last zeros on a rank whose share has none takes that share's first zero.
 * Collective like the other pdx_dist_* calls: a rank whose shard fails its local checks makes EVERY rank return an error before any
 * data exchange.  Fetch: keys / first_rows may be NULL; outs[k] = the k-th requested kind, dtypes as pdx_groupby_agg. */
typedef struct pdx_dist_agg pdx_dist_agg;
int pdx_dist_groupby_order_free(pdx_dist* d, const pdx_column* keys, const pdx_column* values, const int* kinds, int nk, int64_t row_offset, void* stream,
                                pdx_dist_agg** out);
int64_t pdx_dist_agg_num_groups(const pdx_dist_agg* g);
int pdx_dist_agg_fetch(const pdx_dist_agg* g, pdx_mut_column* keys, int64_t* first_rows, pdx_mut_column* outs, void* stream);
int pdx_dist_agg_destroy(pdx_dist_agg* g);
/* pd::resample(df, rule).{kinds}(col) over a sorted axis sharded by row ranges (src/resample.h:91-122, src/group_by.h:255-299): the
 * leading rows of a shard whose bin opened on an earlier rank move there (one all-to-all(v)), every rank bins on the whole axis'
 * grid (pdx_resample_grid of the all-gathered extremes), results are all-gathered in rank order == label order.  kinds:
 * PDX_AGG_SUM .. PDX_AGG_LAST.  Every rank ends with the full result; the reference's whole-axis errors are raised on every rank. */
typedef struct pdx_dist_resampled pdx_dist_resampled;
int pdx_dist_resample(pdx_dist* d, const pdx_column* ts, const pdx_column* values, const int* kinds, int nk, int64_t freq_ns, int closed_right,
                      int label_right, int origin_type, int64_t origin_custom_ns, int64_t offset_ns, void* stream, pdx_dist_resampled** out);
int64_t pdx_dist_resampled_num_bins(const pdx_dist_resampled* g);
int pdx_dist_resampled_fetch(const pdx_dist_resampled* g, pdx_mut_column* labels, pdx_mut_column* outs, void* stream);
int pdx_dist_resampled_destroy(pdx_dist_resampled* g);
/* The headline query on ONE GPU for inputs beyond the per-call limit of pdx_groupby_create (2^31 - 1 rows: the reference's own
 * Grouper::MakeGroupings breaks there): the rows are cut into chunks of chunk_rows (0 = the largest the limit allows; tests
 * pass small values), every chunk plays one rank of the exchange above on a host thread of its own, and the partial-tree records merge
 * the chunks' sums bit-identically to ONE pairwise tree over the whole column.  Result handle as pdx_dist_groupby_sum_mean_count. */
int pdx_groupby_sum_mean_count_chunked(const pdx_column* keys, const pdx_column* values, int64_t chunk_rows, void* stream, pdx_dist_groupby** out);
/* The same for the order-free kinds (PDX_AGG_MIN / MAX / COUNT, PDX_AGG_SUM of int64 values; values may carry nulls): chunks play the ranks of
 * pdx_dist_groupby_order_free, dense per-group partials folded in chunk order.  Result handle as pdx_dist_groupby_order_free (pdx_dist_agg_fetch). */
int pdx_groupby_order_free_chunked(const pdx_column* keys, const pdx_column* values, const int* kinds, int nk, int64_t chunk_rows, void* stream, pdx_dist_agg** out);

/* ---------------------------------------------------------------- Parquet files -> device columns
 * Replaces, for the column types of this path, DataFrame::readParquet (src/dataframe.cpp:646-683: parquet::arrow::OpenFile ->
 * FileReader::ReadTable -> TableBatchReader::ToRecordBatches, exactly ONE record batch).  The host parses the metadata only (the
 * Thrift-compact footer in pdx_parquet_open, the page headers in pdx_parquet_load); the column chunks go to the device in ONE copy
 * and every page payload is decoded there: Snappy blocks, RLE / bit-packed definition levels -> validity bitmap, PLAIN and
 * dictionary-encoded (PLAIN_DICTIONARY / RLE_DICTIONARY) values -> 8-byte values, data pages v1 and v2.
 *   pdx_parquet_open    parse a file held in HOST memory (no GPU needed); the bytes must stay alive until pdx_parquet_load returns.
 *                       Columns: flat BOOLEAN / INT32 / INT64 / FLOAT / DOUBLE leaves, REQUIRED or OPTIONAL; INT annotations widen to
 *                       int64 / uint64, FLOAT to float64, TIMESTAMP(ms | us | ns) becomes timestamp[ns].  One row group, as the
 *                       reference: more give PDX_INVALID "DataFrame Only supports Parquet Table with single record batch", an empty
 *                       table "Cannot Initialize DataFrame with empty parquet table".  PDX_NOT_IMPLEMENTED, naming the column and the
 *                       feature, for strings / BYTE_ARRAY, nested or repeated columns, INT96, DATE / TIME / DECIMAL annotations,
 *                       codecs other than UNCOMPRESSED / SNAPPY, DELTA_* / BYTE_STREAM_SPLIT encodings, encryption.
 *   pdx_parquet_load    upload + decode; synchronises `stream`.  Malformed pages (bad Snappy blocks, short value sections,
 *                       dictionary indices out of range) are detected on the device and fail the call with PDX_INVALID.
 *   pdx_parquet_column  the i-th column (device pointers owned by the file object until pdx_parquet_destroy; before the load only
 *                       dtype, length and the chunk statistics' null_count, -1 when the writer left it out).
 * The file's key_value_metadata (pandas / ARROW:schema entries) is available as strings. */
typedef struct pdx_parquet_file pdx_parquet_file;
int pdx_parquet_open(const void* blob, size_t size, pdx_parquet_file** out);
int pdx_parquet_destroy(pdx_parquet_file* file);
int pdx_parquet_num_columns(const pdx_parquet_file* file);
int64_t pdx_parquet_num_rows(const pdx_parquet_file* file);
const char* pdx_parquet_column_name(const pdx_parquet_file* file, int i);
int pdx_parquet_num_metadata(const pdx_parquet_file* file);
const char* pdx_parquet_metadata_key(const pdx_parquet_file* file, int i);
const char* pdx_parquet_metadata_value(const pdx_parquet_file* file, int i);
int pdx_parquet_load(pdx_parquet_file* file, void* stream);
int pdx_parquet_column(const pdx_parquet_file* file, int i, pdx_column* out);
/* DataFrame::toParquet (src/dataframe.cpp:685-724: one record batch through parquet::arrow::WriteTable with default properties): the
 * equally long columns as ONE row group of uncompressed v1 data pages with PLAIN values; an OPTIONAL column's definition levels are one
 * bit-packed run per page whose payload IS the Arrow validity bitmap of the page's rows.  Columns without a validity bitmap are
 * REQUIRED; uint64 / timestamp[ns] carry their logical types.  Assembled on the host (columns_on_host != 0: the pdx_column pointers
 * are host memory); *out_blob is malloc'ed by the library: release it with pdx_parquet_free_blob.  Readable by Arrow / pyarrow and by
 * pdx_parquet_open. */
int pdx_parquet_write(const pdx_column* cols, const char* const* names, int ncols, int columns_on_host, void* stream, void** out_blob, size_t* out_size);
int pdx_parquet_free_blob(void* blob);

#ifdef __cplusplus
}
#endif
#endif /* PDX_ABI_H */
