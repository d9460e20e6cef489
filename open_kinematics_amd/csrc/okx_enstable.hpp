// okx_enstable.hpp — what the twelve passes over an ensemble table [G * S][ld] share (okx_ensemble.hip, okx_select.hip,
// okx_screen.hip, okx_covariance.hip, okx_curves.hip, okx_front.hip, okx_sobol.hip, okx_bootstrap.hip, okx_effects.hip, okx_tilt.hip, okx_surface.hip,
// okx_predict.hip in its RESIDUAL mode; okx_sample.hip draws tables and reads
// none, so it stays out).  Host side: the view of the table's seven arguments, the argument checks (each with the calling entry point's name
// for the message; a pass calls them where the order of its own checks wants them), the launch plans' common arithmetic and
// the launch helper.  Device side (kernel units only): the acceptance rule, the view's two walks, the workgroup sum and the
// ordered-slot step of the compaction kernels - comparisons and integers only, no floating-point arithmetic: the units
// differ in their contraction setting, and a helper that adds or multiplies would mean different things in them.
#pragma once

#include <cmath>

#include "../../include/okx.h"
#include "okx_program.hpp"

namespace okx {
namespace enstable {

// The table of a call: row g * steps + s holds the n_columns values of step s of geometry g, ld doubles apart; one status
// byte per row, status_stride bytes apart (status null: every row reads as converged, and the stride is 0).
struct Table {
  const double* values;
  const unsigned char* status;
  long long ld, status_stride, n_geom, steps;
  int n_columns;
};

inline Table table_view(const double* d_values, long long ld, const uint8_t* d_status, long long status_stride, long long n_geom,
                        long long steps, int n_columns) {
  return Table{d_values, d_status, ld, d_status ? status_stride : 0, n_geom, steps, n_columns};
}

// the table fields of a kernel's argument struct (it names them as Table does), and of one that reads values only
template <class Args>
inline void set_table(Args* a, const Table& t) {
  a->values = t.values; a->status = t.status; a->ld = t.ld; a->status_stride = t.status_stride;
  a->n_geom = t.n_geom; a->steps = t.steps; a->n_columns = t.n_columns;
}
template <class Args>
inline void set_rows(Args* a, const Table& t) {
  a->values = t.values; a->ld = t.ld; a->n_geom = t.n_geom; a->steps = t.steps;
}

inline int check_counts(const char* who, long long n_geom, long long steps, int n_columns) {
  if (n_geom < 0 || steps < 0 || n_columns < 0) return fail(OKX_ERR_INVALID, "%s: negative geometry, step or column count", who);
  return OKX_OK;
}

// steps fit an int32 and steps * n_columns the pass's `limit`; `what`: what the message finds too many of
inline int check_entries(const char* who, long long steps, int n_columns, long long limit, const char* what = "entries") {
  if (steps > 0x7fffffffll || steps * n_columns > limit) return fail(OKX_ERR_LIMIT, "%s: too many %s for one call", who, what);
  return OKX_OK;
}

// the table [G * S][ld] (`read`: the call has values to read) and its optional status bytes
inline int check_table(const char* who, bool read, const double* d_values, long long ld, int n_columns, const uint8_t* d_status,
                       long long status_stride) {
  if (read && (!d_values || ld < n_columns)) return fail(OKX_ERR_INVALID, "%s: null table or ld < n_columns", who);
  if (d_status && status_stride < 1) return fail(OKX_ERR_INVALID, "%s: status_stride must be positive", who);
  return OKX_OK;
}

// `sizer`: the entry point that says how much the call needs
inline int check_scratch(const char* who, const char* sizer, size_t need, const void* d_scratch, size_t scratch_bytes) {
  if (!d_scratch || scratch_bytes < need)
    return fail(OKX_ERR_INVALID, "%s: %zu bytes of scratch needed (%s), %zu given", who, need, sizer, scratch_bytes);
  return OKX_OK;
}

// host limits [n][2] = (lo, hi): no NaN, lo <= hi
inline int check_limits(const char* who, const double* limits, long long n) {
  for (long long i = 0; i < n; ++i) {
    const double lo = limits[2 * i], hi = limits[2 * i + 1];
    if (std::isnan(lo) || std::isnan(hi)) return fail(OKX_ERR_INVALID, "%s: limit %lld is NaN (an open side is -inf / +inf)", who, i);
    if (lo > hi) return fail(OKX_ERR_INVALID, "%s: limit %lld has lo > hi (%g > %g)", who, i, lo, hi);
  }
  return OKX_OK;
}

// Slabs of geometries for a pass whose lanes own entries (tiles of `tile`) and walk geometries: enough slabs for
// want_groups workgroups, none shorter than min_slab geometries, at most `cap` of them - from the sizes alone.
constexpr long long kNoCap = 0x7fffffffffffffffll;
inline void slab_plan(long long n_geom, long long n_entries, int tile, long long want_groups, long long min_slab, long long cap,
                      long long* n_slabs, long long* slab_len) {
  if (n_geom <= 0) { *n_slabs = 0; *slab_len = 1; return; }
  const long long tiles = n_entries > 0 ? (n_entries + tile - 1) / tile : 1;
  const long long want = (want_groups + tiles - 1) / tiles;
  const long long most = (n_geom + min_slab - 1) / min_slab;
  long long slabs = want < most ? want : most;
  if (slabs < 1) slabs = 1;
  if (slabs > cap) slabs = cap;
  *slab_len = (n_geom + slabs - 1) / slabs;
  *n_slabs = (n_geom + *slab_len - 1) / *slab_len;
}

// Geometries per workgroup for a pass whose workgroups own consecutive geometries: n_geom spread over want_groups, rounded
// up to what a workgroup takes per iteration.
inline long long geometries_per_group(long long n_geom, long long want_groups, long long per_iter) {
  long long gpb = (n_geom + want_groups - 1) / want_groups;
  gpb = (gpb + per_iter - 1) / per_iter * per_iter;
  return gpb < per_iter ? per_iter : gpb;
}

// a kernel launch of an entry point: a launch the runtime refuses is the entry point's OKX_ERR_DEVICE
#define OKX_LAUNCH(kernel, grid, block, lds, stream, ...)                \
  do {                                                                   \
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);   \
    HIP_TRY(hipGetLastError());                                          \
  } while (0)

#if defined(__HIPCC__)

// The rule and the status read are MACROS, and the view's accessors are forced inline with reference parameters, because
// the kernels are held to their instruction text (tools/kernel_text_digest.py): a function is inlined after the first
// simplification passes have run over the kernel around an opaque call, and a by-value parameter counts as well defined,
// which the expression written out does not - either moves operand orders and branch threading in the caller.  In these
// forms the six units' kernels compile to the text they had with the expressions in place, except okx_select_count,
// okx_screen_compact and okx_front_compact (profiles/r18/EXPERIMENTS.md).

// The acceptance rule.  A state counts when it is BatchResult.accepted - converged, not residual-exceeded, not failed - and
// its value is one the reference would not report as None: finite.  (ensemble_stats.STATUS_ACCEPT_MASK on the Python side.)
#define OKX_ENS_ACCEPTED(status, v) \
  (((status) & (unsigned)(OKX_INFO_CONVERGED | OKX_INFO_RESIDUAL_EXCEEDED | OKX_INFO_FAILED)) == OKX_INFO_CONVERGED && __builtin_isfinite(v))
// the status byte of row `row` of a table whose rows' bytes lie `stride` apart; a call without a status table reads converged
#define OKX_ENS_STATUS_AT(status, row, stride) ((status) ? (status)[(long long)(row) * (stride)] : 1u)

// the view, from a kernel's argument struct that names the table fields as Table does
#define OKX_ENS_TABLE_OF(a) okx::enstable::Table{(a).values, (a).status, (a).ld, (a).status_stride, (a).n_geom, (a).steps, (a).n_columns}

// Walk 1 (a lane owns entry e = s * n_columns + k and walks geometries): the entry of geometry 0, and how far the next
// geometry's lies - in doubles and in status bytes.
__device__ __forceinline__ const double* entry_values(const Table& t, const long long& e) {
  return t.values + e / t.n_columns * t.ld + e % t.n_columns;
}
__device__ __forceinline__ const unsigned char* entry_status(const Table& t, const long long& e) {
  return t.status ? t.status + e / t.n_columns * t.status_stride : nullptr;
}
__device__ __forceinline__ long long value_step(const Table& t) { return t.steps * t.ld; }
__device__ __forceinline__ long long status_step(const Table& t) { return t.steps * t.status_stride; }

// Walk 2 (the lanes of a group share geometry g): its first row; (s, k) inside it is values[s * ld + k], status[s * status_stride].
__device__ __forceinline__ const double* geometry_values(const Table& t, const long long& g) { return t.values + g * t.steps * t.ld; }
__device__ __forceinline__ const unsigned char* geometry_status(const Table& t, const long long& g) {
  return t.status ? t.status + g * t.steps * t.status_stride : nullptr;
}

// the sum of one value per thread over a workgroup of kWaves wavefronts, in every thread (integers: the order does not matter)
template <int kWaves>
__device__ inline long long block_sum(long long x, long long* lds) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  __syncthreads();  // (lds may still be read from the call before)
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
  __syncthreads();
  long long sum = 0;
  for (int w = 0; w < kWaves; ++w) sum += lds[w];
  return sum;
}

// The ordered-slot step of a compaction: how many threads before this one in the workgroup keep their item - a ballot, the
// prefix inside the wavefront, the wavefronts' counts through wave_n [kWaves] in LDS - and in *all how many keep one in the
// whole workgroup.  No atomic decides a position.
template <int kWaves>
__device__ inline unsigned kept_before(bool keep, unsigned* wave_n, unsigned* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(keep);
  const unsigned mine = (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) wave_n[wave] = (unsigned)__popcll(mask);
  __syncthreads();
  unsigned ahead = 0u, total = 0u;
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) ahead += wave_n[w];
    total += wave_n[w];
  }
  *all = total;
  return ahead + mine;
}

#endif  // __HIPCC__

}  // namespace enstable
}  // namespace okx
