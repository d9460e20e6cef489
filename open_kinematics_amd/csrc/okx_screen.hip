// Ensemble screening (okx_ensemble_screen*, include/okx.h): the JOINT spec-limit verdict of every geometry of a table of
// metric columns [G * S][ld] - flags, the worst scaled margin and the entry that holds it - with the ensemble's tally, the
// blame counts per (entry, side) and the ascending list of the geometries that pass.
//
// The transpose of okx_ensemble.hip / okx_select.hip: there a lane owns an ENTRY and walks geometries; here the reduction
// runs over the S * K entries of ONE geometry, which are contiguous when ld == K.
//
// Verdict pass (okx_screen_verdict): a group of L lanes (L = the power of two >= S * K, at most 64) strides over the
// entries of one geometry - a wavefront reads 64 consecutive doubles - and 64 / L geometries share a wavefront when the
// table is narrow.  (s, k) of a lane's entry advance by additions (no division in the loop), so strided rows (ld > K) and a
// strided status byte cost nothing extra.  Limits and scale are re-read per geometry: S * K * 24 bytes that stay in L2.
// The group then reduces (margin, entry) to the minimum with the lowest entry on ties and ORs the flags by xor-shuffles;
// its first lane writes the geometry's verdict and, into d_scratch, its blame key (entry, side; -1: none).  A workgroup owns
// gpb consecutive geometries (a function of the sizes alone), counts its passed / outside / unresolved geometries by
// ballots and leaves the three totals in d_scratch.  The pass touches neither d_blame nor d_pass_count otherwise, so it
// also does what must come before the second pass: it zeroes d_blame (accumulate = 0) and keeps the survivor count found
// so far - two launches in all.
// Compaction pass (okx_screen_compact): every workgroup sums the passed totals of the workgroups before it, then walks its
// own geometries in ascending order with ballot + prefix counts: a survivor's slot is base + what passed before it - no
// atomic decides a position.  The blame keys of the same geometries gather in LDS (uint32 [S K][2]) and leave with one
// 64-bit integer atomic per non-zero counter, or - when the counters do not fit - per wavefront, one atomic per distinct
// key.  The last workgroup sums all totals into d_tally and d_pass_count, each written by that one thread.
//
// Every floating-point operation is rounded on its own, in the order of ensemble_stats.screen_host: x = v - lo, y = hi - v,
// each divided by the scale, m = y < x ? y : x.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/okx.h"
#include "okx_enstable.hpp"
#include "okx_program.hpp"

#pragma clang fp contract(off)

namespace okx {
namespace scr {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr long long kWantGroups = 1024;       // workgroups aimed at (four per CU of a 256-CU part, from the sizes alone)
constexpr long long kLdsBlameBytes = 32 * 1024;  // the blame counters of a workgroup live in LDS up to this size
constexpr long long kMaxEntries = 1ll << 30;  // (entry * 2 + side) is an int32
constexpr int kNoEntry = 0x7fffffff;

typedef unsigned long long u64;

struct Plan {
  int lanes;         // per geometry: power of two, 1 .. 64
  long long gpb;     // geometries per workgroup
  long long groups;  // workgroups
  int lds_blame;     // the blame counters fit LDS
};

inline Plan plan_for(long long n_geom, long long n_entries) {
  Plan p;
  p.lanes = 1;
  while (p.lanes < 64 && p.lanes < n_entries) p.lanes <<= 1;
  const long long per_iter = (long long)kWaves * (64 / p.lanes);
  p.gpb = enstable::geometries_per_group(n_geom, kWantGroups, per_iter);
  p.groups = n_geom > 0 ? (n_geom + p.gpb - 1) / p.gpb : 0;
  p.lds_blame = n_entries * 2 * 4 <= kLdsBlameBytes ? 1 : 0;
  return p;
}

// d_scratch: int64 the survivor count before this call | int64 per workgroup (passed, outside, unresolved) | int32 per
// geometry the blame key
inline size_t scratch_words(long long groups) { return 1 + 3 * (size_t)groups; }
inline size_t scratch_bytes(long long groups, long long n_geom) { return 8 * scratch_words(groups) + 4 * (size_t)(n_geom > 0 ? n_geom : 0); }

struct VerdictArgs {
  const double* values;
  const unsigned char* status;
  const double* limits;  // [E][2]
  const double* scale;   // [E] or null
  unsigned char* flags;
  double* margin;
  int* entry;
  int* blame_key;        // [n_geom]: entry * 2 + side of an OUTSIDE geometry, -1 otherwise
  u64* blame;            // [E][2]: zeroed here unless accumulate
  long long* totals;     // [groups][3]
  const long long* pass_count;
  long long* base;       // the survivor count before this call
  long long ld, status_stride, n_geom, steps, gpb, groups;
  int n_entries, n_columns, lanes, accumulate;
};

__global__ __launch_bounds__(kThreads) void okx_screen_verdict(VerdictArgs a) {
  __shared__ unsigned scr_lds[4];  // passed, outside, unresolved
  const int E = a.n_entries, L = a.lanes, pack = 64 / L;
  if (threadIdx.x < 4) scr_lds[threadIdx.x] = 0u;
  __syncthreads();
  // what the compaction pass needs done before it starts (nothing in THIS pass reads or adds into these)
  if (!a.accumulate)
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < 2ll * E; i += (long long)gridDim.x * kThreads) a.blame[i] = 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.base = a.accumulate ? *a.pass_count : 0ll;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = lane & (L - 1), sub = lane / L;
  const int K = a.n_columns > 0 ? a.n_columns : 1;
  const int s0 = t / K, k0 = t % K, ds = L / K, dk = L % K;  // entry e = t, t + L, ...: (s, k) by additions
  const long long g0 = (long long)blockIdx.x * a.gpb;
  const long long g1 = g0 + a.gpb < a.n_geom ? g0 + a.gpb : a.n_geom;
  const enstable::Table tab = OKX_ENS_TABLE_OF(a);
  unsigned n_pass = 0u, n_out = 0u, n_unres = 0u;  // wave-uniform
  for (long long gb = g0 + (long long)wave * pack; gb < g1; gb += (long long)kWaves * pack) {
    const long long g = gb + sub;
    const bool live = g < g1;
    double m = __builtin_inf();
    int key = kNoEntry;  // entry * 2 + (value below lo)
    unsigned fl = 0u;
    if (live) {
      const double* vp = enstable::geometry_values(tab, g);
      const unsigned char* sp = enstable::geometry_status(tab, g);
      int s = s0, k = k0;
#pragma unroll 4
      for (int e = t; e < E; e += L) {
        const double lo = a.limits[2 * (long long)e], hi = a.limits[2 * (long long)e + 1];
        const double v = vp[(long long)s * a.ld + k];
        const unsigned st = OKX_ENS_STATUS_AT(sp, s, a.status_stride);
        const double sc = a.scale ? a.scale[e] : 1.0;
        s += ds; k += dk;
        if (k >= K) { k -= K; ++s; }
        if (!(__builtin_isfinite(lo) || __builtin_isfinite(hi))) continue;  // not looked at
        if (!OKX_ENS_ACCEPTED(st, v)) { fl |= OKX_SCREEN_UNRESOLVED; continue; }
        const bool below = v < lo;
        if (below || v > hi) fl |= OKX_SCREEN_OUTSIDE;
        double x = v - lo, y = hi - v;
        if (a.scale) { x = x / sc; y = y / sc; }
        const double mm = y < x ? y : x;
        if (mm < m || key == kNoEntry) { m = mm; key = e * 2 + (below ? 1 : 0); }  // ascending e: a tie keeps the lower entry
      }
    }
    for (int off = L >> 1; off > 0; off >>= 1) {
      const double om = __shfl_xor(m, off);
      const int okey = __shfl_xor(key, off);
      fl |= (unsigned)__shfl_xor((int)fl, off);
      if (om < m || (om == m && okey < key)) { m = om; key = okey; }
    }
    const bool lead = live && t == 0;
    const bool outside = (fl & OKX_SCREEN_OUTSIDE) != 0u;
    if (lead) {
      a.flags[g] = (unsigned char)fl;
      a.margin[g] = m;
      a.entry[g] = key == kNoEntry ? -1 : key >> 1;
      // side 0: below lo, side 1: above hi
      a.blame_key[g] = outside && key != kNoEntry ? (key >> 1) * 2 + ((key & 1) ? 0 : 1) : -1;
    }
    n_pass += (unsigned)__popcll(__ballot(lead && fl == 0u));
    n_out += (unsigned)__popcll(__ballot(lead && outside));
    n_unres += (unsigned)__popcll(__ballot(lead && (fl & OKX_SCREEN_UNRESOLVED) != 0u));
  }
  if (lane == 0) {
    if (n_pass != 0u) atomicAdd(&scr_lds[0], n_pass);
    if (n_out != 0u) atomicAdd(&scr_lds[1], n_out);
    if (n_unres != 0u) atomicAdd(&scr_lds[2], n_unres);
  }
  __syncthreads();
  if (threadIdx.x < 3 && blockIdx.x < a.groups) a.totals[3 * (long long)blockIdx.x + threadIdx.x] = (long long)scr_lds[threadIdx.x];
}

struct CompactArgs {
  const unsigned char* flags;
  const int* blame_key;     // [n_geom]
  u64* blame;               // [E][2]
  const long long* totals;  // [groups][3]
  const long long* base;
  long long* tally;         // [4]
  long long* pass_index;    // [capacity] or null
  long long* pass_count;
  long long n_geom, gpb, groups, capacity, geometry_offset;
  int accumulate, n_entries, lds_blame;
};

__global__ __launch_bounds__(kThreads) void okx_screen_compact(CompactArgs a) {
  __shared__ long long sums[kWaves];
  __shared__ unsigned wave_n[kWaves];
  extern __shared__ unsigned blame_lds[];  // [E][2] (lds_blame)
  const int n_blame = a.lds_blame ? 2 * a.n_entries : 0;
  for (int i = threadIdx.x; i < n_blame; i += kThreads) blame_lds[i] = 0u;  // (block_sum's barriers come before the first add)
  const long long b = blockIdx.x;
  const bool last = b + 1 >= a.groups;  // (groups == 0: the one workgroup launched)
  long long before = 0;
  for (long long i = threadIdx.x; i < b && i < a.groups; i += kThreads) before += a.totals[3 * i];
  before = enstable::block_sum<kWaves>(before, sums);
  const long long base = *a.base;
  const long long g0 = b * a.gpb;
  const long long g1 = g0 + a.gpb < a.n_geom ? g0 + a.gpb : a.n_geom;
  const int lane = threadIdx.x & 63;
  long long at = base + before;  // the slot of the next survivor of this workgroup
  for (long long gc = g0; gc < g1; gc += kThreads) {
    const long long g = gc + threadIdx.x;
    const bool pass = g < g1 && a.flags[g] == 0;
    int blamed = g < g1 ? a.blame_key[g] : -1;
    if (a.lds_blame) {
      if (blamed >= 0) atomicAdd(&blame_lds[blamed], 1u);
    } else {
      // one atomic per distinct key of the wavefront (the loop's condition is a ballot: every lane takes every turn)
      for (u64 left = __ballot(blamed >= 0); left != 0ull; left = __ballot(blamed >= 0)) {
        const int first = __ffsll((long long)left) - 1;
        const int k0 = __shfl(blamed, first);
        const u64 same = __ballot(blamed == k0);
        if (lane == first) atomicAdd(&a.blame[k0], (u64)__popcll(same));
        if (blamed == k0) blamed = -1;
      }
    }
    unsigned all;
    const long long slot = at + enstable::kept_before<kWaves>(pass, wave_n, &all);
    if (pass && a.pass_index && slot >= 0 && slot < a.capacity) a.pass_index[slot] = a.geometry_offset + g;
    at += all;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_blame; i += kThreads) {
    const unsigned c = blame_lds[i];
    if (c != 0u) atomicAdd(&a.blame[i], (u64)c);
  }
  if (last) {
    long long n_out = 0, n_unres = 0;
    for (long long i = threadIdx.x; i < a.groups; i += kThreads) { n_out += a.totals[3 * i + 1]; n_unres += a.totals[3 * i + 2]; }
    n_out = enstable::block_sum<kWaves>(n_out, sums);
    n_unres = enstable::block_sum<kWaves>(n_unres, sums);
    if (threadIdx.x == 0) {
      const long long passed = at - base;  // what passed before this workgroup and in it
      const long long add[4] = {a.n_geom, passed, n_out, n_unres};
      for (int i = 0; i < 4; ++i) a.tally[i] = (a.accumulate ? a.tally[i] : 0ll) + add[i];
      *a.pass_count = at;
    }
  }
}

inline int check_sizes(const char* who, long long n_geom, long long steps, int n_columns) {
  if (int rc = enstable::check_counts(who, n_geom, steps, n_columns)) return rc;
  return enstable::check_entries(who, steps, n_columns, kMaxEntries);
}

}  // namespace scr
}  // namespace okx

using okx::fail;
namespace et = okx::enstable;

extern "C" {

size_t okx_ensemble_screen_scratch_bytes(int64_t n_geometries, int64_t steps, int32_t n_columns) {
  namespace sc = okx::scr;
  if (n_geometries < 0 || steps < 0 || n_columns < 0) return 0;
  return sc::scratch_bytes(sc::plan_for(n_geometries, (long long)steps * n_columns).groups, n_geometries);
}

int32_t okx_ensemble_screen_check(const double* limits, const double* scale, int64_t n_entries) {
  if (n_entries < 0 || (n_entries > 0 && !limits)) return fail(OKX_ERR_INVALID, "okx_ensemble_screen: null limits");
  if (int rc = et::check_limits("okx_ensemble_screen", limits, n_entries)) return rc;
  if (scale)
    for (int64_t i = 0; i < n_entries; ++i)
      if (!(std::isfinite(scale[i]) && scale[i] > 0.0))
        return fail(OKX_ERR_INVALID, "okx_ensemble_screen: scale %lld is %g, not finite and > 0", (long long)i, scale[i]);
  return OKX_OK;
}

int32_t okx_ensemble_screen(int64_t n_geometries, int64_t steps, int32_t n_columns, const double* d_values, int64_t ld, const uint8_t* d_status,
                            int64_t status_stride, const double* d_limits, const double* d_scale, int64_t geometry_offset, int32_t accumulate,
                            uint8_t* d_flags, double* d_margin, int32_t* d_entry, int64_t* d_tally, int64_t* d_blame, int64_t* d_pass_index,
                            int64_t capacity, int64_t* d_pass_count, void* d_scratch, size_t scratch_bytes, void* stream) {
  namespace sc = okx::scr;
  if (int rc = sc::check_sizes("okx_ensemble_screen", n_geometries, steps, n_columns)) return rc;
  const long long n_entries = (long long)steps * n_columns;
  if (!d_tally || !d_pass_count || (n_entries > 0 && !d_blame)) return fail(OKX_ERR_INVALID, "okx_ensemble_screen: null tally, blame or survivor count");
  if (n_geometries > 0 && (!d_flags || !d_margin || !d_entry)) return fail(OKX_ERR_INVALID, "okx_ensemble_screen: null flags, margin or entry table");
  if (n_entries > 0 && !d_limits) return fail(OKX_ERR_INVALID, "okx_ensemble_screen: null limits");
  if (int rc = et::check_table("okx_ensemble_screen", n_geometries > 0 && n_entries > 0, d_values, ld, n_columns, d_status, status_stride)) return rc;
  if (capacity < 0) return fail(OKX_ERR_INVALID, "okx_ensemble_screen: negative capacity");
  const size_t need = okx_ensemble_screen_scratch_bytes(n_geometries, steps, n_columns);
  if (int rc = et::check_scratch("okx_ensemble_screen", "okx_ensemble_screen_scratch_bytes", need, d_scratch, scratch_bytes)) return rc;
  const sc::Plan plan = sc::plan_for(n_geometries, n_entries);
  if (plan.groups > 0x7fffffffll) return fail(OKX_ERR_LIMIT, "okx_ensemble_screen: too many geometries for one call");
  long long* base = static_cast<long long*>(d_scratch);
  long long* totals = base + 1;
  int* blame_key = reinterpret_cast<int*>(totals + 3 * plan.groups);
  const unsigned grid = (unsigned)(plan.groups > 0 ? plan.groups : 1);  // (no geometry: the one workgroup zeroes and keeps the count)
  {
    sc::VerdictArgs a{};
    et::set_table(&a, et::table_view(d_values, ld, d_status, status_stride, n_geometries, steps, n_columns));
    a.limits = d_limits; a.scale = d_scale;
    a.flags = d_flags; a.margin = d_margin; a.entry = d_entry;
    a.blame_key = blame_key; a.blame = reinterpret_cast<sc::u64*>(d_blame); a.totals = totals;
    a.pass_count = reinterpret_cast<const long long*>(d_pass_count); a.base = base;
    a.gpb = plan.gpb; a.groups = plan.groups; a.n_entries = (int)n_entries; a.lanes = plan.lanes; a.accumulate = accumulate != 0;
    OKX_LAUNCH(sc::okx_screen_verdict, dim3(grid), dim3(sc::kThreads), 0, (hipStream_t)stream, a);
  }
  sc::CompactArgs c{};
  c.flags = d_flags; c.blame_key = blame_key; c.blame = reinterpret_cast<sc::u64*>(d_blame); c.totals = totals; c.base = base;
  c.tally = reinterpret_cast<long long*>(d_tally); c.pass_index = reinterpret_cast<long long*>(d_pass_index);
  c.pass_count = reinterpret_cast<long long*>(d_pass_count);
  c.n_geom = n_geometries; c.gpb = plan.gpb; c.groups = plan.groups; c.capacity = d_pass_index ? capacity : 0;
  c.geometry_offset = geometry_offset; c.accumulate = accumulate != 0; c.n_entries = (int)n_entries; c.lds_blame = plan.lds_blame;
  OKX_LAUNCH(sc::okx_screen_compact, dim3(grid), dim3(sc::kThreads), plan.lds_blame ? 8 * (size_t)n_entries : 0, (hipStream_t)stream, c);
  return OKX_OK;
}

}  // extern "C"
