// Main effects from given data (okx_ensemble_bin, okx_ensemble_effects, include/okx.h): how an output depends on ONE factor
// beyond a straight line - the conditional moments of every (step, column) entry of an evaluated ensemble over equal-probability
// bins of every factor (Plischke 2010).  Per (factor j, bin b, entry) COUNT, sum d and sum d^2, d = value - shift, over the
// geometries that fall into bin b of factor j and count at the entry (okx_enstable.hpp's rule and the optional mask bytes).
//
// Two passes.  The BIN pass is integers and comparisons only: okx_effects_bytes writes the bin byte of every (geometry, factor) -
// the number of edges <= x, 255 for a NaN -, okx_effects_lists turns each factor's byte column into the list of its binned
// geometries, bin by bin and ascending inside a bin, with the bins' starts: a workgroup per (factor, bin) counts the bytes below
// its own (its start), then walks the column 256 geometries a round and places the round's members by a ballot and prefix
// counts (enstable::kept_before).  No atomic decides a slot: the list is the same bits every run.
//
// The EFFECTS pass streams the table; what has to be right is traffic and registers.  A workgroup - one wavefront - owns (a tile
// of 64 entries, factor j, bin b); as in okx_sobol.hip a lane owns one entry e = s * K + k and walks the bin's list in order:
// every wave-instruction reads 64 consecutive doubles of one row (ld == K), the list, the mask and the offsets are uniform over
// the wavefront, and the three sums live in registers - no slabs, no partials, no LDS, no scratch buffer.  The walk is unrolled by
// kRows so that eight rows' loads are in flight before the first is added (one load, one wait, one add per row would leave the
// pass waiting on memory for the length of the list).  The table is read once per factor.
//
// ROUNDING.  Contraction is off for the unit: d = value - shift is rounded, then d * d, then each is added to its sum.  Every cell
// (factor, bin, field, entry) is ONE chain of additions in ascending geometry order - the order ensemble_stats.effects_host uses -
// begun at 0 or, accumulating, at what d_acc holds: bit-identical from run to run and from device to device, equal to the host
// on integer tables, and chunks accumulated in ascending order carry the bits of the whole; accumulators merged by addition
// (ranks) differ from the whole by the addition order only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/okx.h"
#include "okx_enstable.hpp"
#include "okx_program.hpp"

#pragma clang fp contract(off)

namespace okx {
namespace eff {

constexpr int kTile = 64;     // entries per workgroup of the effects pass: one per lane, one wavefront
constexpr int kRows = 8;      // rows of a list whose loads are in flight together
constexpr int kWaves = 4;     // wavefronts of a workgroup of the list pass
constexpr int kBlock = 64 * kWaves;
constexpr int kFields = OKX_EFFECTS_FIELDS;

// ---- the bin pass ----

// one thread per (geometry, factor): the number of the factor's edges <= x, comparisons only; NaN: OKX_ENS_EFFECTS_NO_BIN
__global__ __launch_bounds__(kBlock) void okx_effects_bytes(const double* factors, long long ldf, const double* edges, long long n_geom, int n_factors,
                                                            int n_bins, unsigned char* bins) {
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_geom * n_factors) return;
  const long long g = t / n_factors;
  const int j = (int)(t % n_factors);
  const double x = factors[g * ldf + j];
  const double* edge = edges + (long long)j * (n_bins - 1);
  unsigned at = 0u;
  for (int i = 0; i < n_bins - 1; ++i) at += edge[i] <= x ? 1u : 0u;
  bins[t] = x != x ? (unsigned char)OKX_ENS_EFFECTS_NO_BIN : (unsigned char)at;
}

// one workgroup per (factor j, bin b): offsets[j][b] (the last bin also offsets[j][n_bins] and the -1 of the unused tail) and the
// bin's stretch of order[j]
__global__ __launch_bounds__(kBlock) void okx_effects_lists(const unsigned char* bins, long long n_geom, int n_factors, int n_bins, int* order,
                                                            long long* offsets) {
  __shared__ long long sums[kWaves];
  __shared__ unsigned wave_n[kWaves];
  const int j = blockIdx.x, b = blockIdx.y;
  const unsigned char* column = bins + j;
  long long below = 0, here = 0;
  for (long long g = threadIdx.x; g < n_geom; g += kBlock) {
    const int byte = column[g * n_factors];
    below += byte < b ? 1 : 0;
    here += byte == b ? 1 : 0;
  }
  const long long start = enstable::block_sum<kWaves>(below, sums);
  const long long mine = enstable::block_sum<kWaves>(here, sums);
  int* list = order + (long long)j * n_geom;
  long long* off = offsets + (long long)j * (n_bins + 1);
  if (threadIdx.x == 0) {
    off[b] = start;
    if (b == n_bins - 1) off[n_bins] = start + mine;
  }
  long long at = start;
  for (long long g0 = 0; g0 < n_geom; g0 += kBlock) {  // (every thread of the workgroup takes every round: kept_before has barriers)
    const long long g = g0 + threadIdx.x;
    const bool keep = g < n_geom && column[g * n_factors] == b;
    unsigned all;
    const unsigned slot = enstable::kept_before<kWaves>(keep, wave_n, &all);
    if (keep) list[at + slot] = (int)g;  // at + slot < start + mine <= n_geom
    at += all;
  }
  if (b == n_bins - 1)
    for (long long p = start + mine + threadIdx.x; p < n_geom; p += kBlock) list[p] = -1;
}

// ---- the effects pass ----

struct Args {
  const double* values;
  const unsigned char* status;
  const unsigned char* mask;  // [n_geom] or null
  const double* shift;
  const int* order;           // [n_factors][n_geom]
  const long long* offsets;   // [n_factors][n_bins + 1]
  double* acc;                // [n_factors][n_bins][kFields][n_entries]
  long long ld, status_stride;
  long long n_geom, steps;
  long long n_entries;
  int n_columns, n_bins, accumulate;
};

// kStatus / kMask: the call has status bytes / mask bytes.  They are template arguments so that the walk has no branch around a
// load: with the null tests inside the loop every byte load was waited for at once, and the rows' loads with it.
template <bool kStatus, bool kMask>
__global__ __launch_bounds__(kTile) void okx_effects_walk(Args a) {
  const int lane = threadIdx.x;
  const long long e = (long long)blockIdx.x * kTile + lane;
  const bool live = e < a.n_entries;
  const long long er = live ? e : 0;  // a lane past the table walks entry 0 and stores nothing
  const long long j = blockIdx.y, b = blockIdx.z;
  const long long* off = a.offsets + j * (a.n_bins + 1) + b;
  long long lo = off[0], hi = off[1];  // (uniform over the wavefront; a list is never trusted beyond the table)
  lo = lo < 0 ? 0 : lo;
  hi = hi > a.n_geom ? a.n_geom : hi;
  const int* list = a.order + j * a.n_geom;
  const enstable::Table t = OKX_ENS_TABLE_OF(a);
  const double* vp = enstable::entry_values(t, er);
  const unsigned char* sp = kStatus ? a.status + er / a.n_columns * a.status_stride : nullptr;
  const long long v_step = enstable::value_step(t), s_step = enstable::status_step(t);
  const double sh = a.shift[er];
  double* out = a.acc + ((j * a.n_bins + b) * kFields) * a.n_entries + er;
  double count = 0.0, sum = 0.0, sq = 0.0;
  if (a.accumulate) {  // the chains go on from what the cell holds
    count = out[OKX_EFFECTS_COUNT * a.n_entries]; sum = out[OKX_EFFECTS_SUM * a.n_entries]; sq = out[OKX_EFFECTS_SUMSQ * a.n_entries];
  }
  long long p = lo;
  for (; p + kRows <= hi; p += kRows) {
    long long g[kRows];
    bool inside[kRows];
    double v[kRows];
    unsigned st[kRows], mk[kRows];
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      const long long at = list[p + i];
      inside[i] = at >= 0 && at < a.n_geom;
      g[i] = inside[i] ? at : 0;
    }
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      v[i] = vp[g[i] * v_step];
      st[i] = kStatus ? sp[g[i] * s_step] : 1u;
      mk[i] = kMask ? a.mask[g[i]] : 0u;
    }
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      const unsigned word = st[i] | ((mk[i] & 1u) << 2);  // a masked geometry reads as failed: one test, and no load is left behind a branch
      const bool ok = inside[i] & OKX_ENS_ACCEPTED(word, v[i]);
      const double d = v[i] - sh;
      count += ok ? 1.0 : 0.0;
      sum += ok ? d : 0.0;       // (x + 0.0 is x for every x a chain can hold: it starts at +0.0 and never becomes -0.0)
      sq += ok ? d * d : 0.0;
    }
  }
  for (; p < hi; ++p) {
    const long long at = list[p];
    const bool inside = at >= 0 && at < a.n_geom;
    const long long g = inside ? at : 0;
    const double v = vp[g * v_step];
    const unsigned st = kStatus ? sp[g * s_step] : 1u;
    const unsigned mk = kMask ? a.mask[g] : 0u;
    const unsigned word = st | ((mk & 1u) << 2);
    const bool ok = inside & OKX_ENS_ACCEPTED(word, v);
    const double d = v - sh;
    count += ok ? 1.0 : 0.0;
    sum += ok ? d : 0.0;
    sq += ok ? d * d : 0.0;
  }
  if (!live) return;
  out[OKX_EFFECTS_COUNT * a.n_entries] = count; out[OKX_EFFECTS_SUM * a.n_entries] = sum; out[OKX_EFFECTS_SUMSQ * a.n_entries] = sq;
}

template <bool kStatus, bool kMask>
inline hipError_t launch_walk(const Args& a, int n_factors, hipStream_t st) {
  const unsigned tiles = (unsigned)((a.n_entries + kTile - 1) / kTile);
  hipLaunchKernelGGL((okx_effects_walk<kStatus, kMask>), dim3(tiles, (unsigned)n_factors, (unsigned)a.n_bins), dim3(kTile), 0, st, a);
  return hipGetLastError();
}

inline int check_sizes(const char* who, long long n_geom, int n_factors, int n_bins) {
  if (n_factors < 1 || n_factors > OKX_ENS_EFFECTS_MAX_FACTORS)
    return fail(OKX_ERR_INVALID, "%s: %d factors, 1 to %d allowed", who, n_factors, (int)OKX_ENS_EFFECTS_MAX_FACTORS);
  if (n_bins < 1 || n_bins > OKX_ENS_EFFECTS_MAX_BINS)
    return fail(OKX_ERR_INVALID, "%s: %d bins, 1 to %d allowed", who, n_bins, (int)OKX_ENS_EFFECTS_MAX_BINS);
  if (n_geom > 0x7fffffffll) return fail(OKX_ERR_LIMIT, "%s: too many geometries for one call", who);  // (order is int32)
  return OKX_OK;
}

}  // namespace eff
}  // namespace okx

using okx::fail;
namespace et = okx::enstable;

extern "C" {

int32_t okx_ensemble_bin(int64_t n_geometries, int32_t n_factors, const double* d_factors, int64_t ldf, const double* d_edges, int32_t n_bins,
                         uint8_t* d_bins, int32_t* d_order, int64_t* d_offsets, void* stream) {
  namespace ef = okx::eff;
  const char* who = "okx_ensemble_bin";
  if (int rc = et::check_counts(who, n_geometries, 0, 0)) return rc;
  if (int rc = ef::check_sizes(who, n_geometries, n_factors, n_bins)) return rc;
  if (!d_offsets) return fail(OKX_ERR_INVALID, "%s: null offsets table", who);
  if (n_geometries > 0 && (!d_factors || ldf < n_factors)) return fail(OKX_ERR_INVALID, "%s: null factor table or ldf < n_factors", who);
  if (n_geometries > 0 && (!d_bins || !d_order)) return fail(OKX_ERR_INVALID, "%s: null bin or order table", who);
  if (n_geometries > 0 && n_bins > 1 && !d_edges) return fail(OKX_ERR_INVALID, "%s: null edge table", who);
  const hipStream_t st = (hipStream_t)stream;
  const long long threads = (long long)n_geometries * n_factors;
  if (threads > 0)
    OKX_LAUNCH(ef::okx_effects_bytes, dim3((unsigned)((threads + ef::kBlock - 1) / ef::kBlock)), dim3(ef::kBlock), 0, st, d_factors, (long long)ldf, d_edges,
               (long long)n_geometries, n_factors, n_bins, d_bins);
  OKX_LAUNCH(ef::okx_effects_lists, dim3((unsigned)n_factors, (unsigned)n_bins), dim3(ef::kBlock), 0, st, d_bins, (long long)n_geometries, n_factors, n_bins,
             d_order, reinterpret_cast<long long*>(d_offsets));
  return OKX_OK;
}

int32_t okx_ensemble_effects(int64_t n_geometries, int64_t steps, int32_t n_columns, const double* d_values, int64_t ld, const uint8_t* d_status,
                             int64_t status_stride, const uint8_t* d_mask, int32_t n_factors, int32_t n_bins, const int32_t* d_order,
                             const int64_t* d_offsets, const double* d_shift, int32_t accumulate, double* d_acc, void* stream) {
  namespace ef = okx::eff;
  const char* who = "okx_ensemble_effects";
  if (int rc = et::check_counts(who, n_geometries, steps, n_columns)) return rc;
  if (int rc = ef::check_sizes(who, n_geometries, n_factors, n_bins)) return rc;
  if (int rc = et::check_entries(who, steps, n_columns, (1ll << 38) / ((long long)ef::kFields * n_factors * n_bins))) return rc;
  const long long n_entries = (long long)steps * n_columns;
  if (n_entries > 0 && (!d_acc || !d_shift)) return fail(OKX_ERR_INVALID, "%s: null accumulator or shift table", who);
  if (!d_offsets || (n_geometries > 0 && !d_order)) return fail(OKX_ERR_INVALID, "%s: null order or offsets table (okx_ensemble_bin makes them)", who);
  if (int rc = et::check_table(who, n_entries > 0 && n_geometries > 0, d_values, ld, n_columns, d_status, status_stride)) return rc;
  if (n_entries == 0) return OKX_OK;
  ef::Args a{};
  et::set_table(&a, et::table_view(d_values, ld, d_status, status_stride, n_geometries, steps, n_columns));
  a.mask = d_mask; a.shift = d_shift; a.order = d_order; a.offsets = reinterpret_cast<const long long*>(d_offsets); a.acc = d_acc;
  a.n_entries = n_entries; a.n_bins = n_bins; a.accumulate = accumulate ? 1 : 0;
  const hipStream_t st = (hipStream_t)stream;
  if (d_status)
    HIP_TRY(d_mask ? (ef::launch_walk<true, true>(a, n_factors, st)) : (ef::launch_walk<true, false>(a, n_factors, st)));
  else
    HIP_TRY(d_mask ? (ef::launch_walk<false, true>(a, n_factors, st)) : (ef::launch_walk<false, false>(a, n_factors, st)));
  return OKX_OK;
}

}  // extern "C"
