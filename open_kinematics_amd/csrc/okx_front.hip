// Ensemble Pareto front (okx_ensemble_front*, include/okx.h): which geometries of a table of metric columns [G * S][ld] no
// other geometry beats on every one of M <= 8 objectives at once - per geometry the number of candidates that dominate it,
// per ensemble the tally and the ascending list of the front members with the raw table values of their objectives.
//
// All comparisons, no floating-point sum and no floating-point atomic: the result is exact and bit-identical however the
// geometries were chunked, and fronts merge by front(A u B) = front(front(A) u front(B)).
//
// Three launches, all sized by plan_for(n_geometries, n_objectives) alone (it never looks at the device):
// Gather pass (okx_front_gather): one lane per geometry reads its M selected entries, decides whether it is a CANDIDATE
// (mask byte 0, every selected entry counts by the acceptance rule of okx_enstable.hpp) and writes its objective vector - v, -v or
// |v - target|, the subtraction rounded once - into d_scratch, double [rows][MP]: rows = G rounded up to a tile of kTile,
// MP = M rounded up to even (M = 1: 1) so that a row of an even M is 16-byte aligned.  The vector of a geometry that is no
// candidate, and of the padding rows, is all NaN: a NaN compares false both ways, so such a row neither dominates nor is
// counted, and the all-pairs pass needs no candidate byte.  (An objective of a candidate is never NaN: v and target are
// finite; |v - target| may overflow to +inf, which orders as it should.)  The pass also initialises d_dominated: 0 for a
// candidate, -1 otherwise.
// All-pairs pass (okx_front_pairs<M>): a lane owns one b with its vector in registers (the template makes every index a
// constant); a workgroup of 256 lanes walks tiles of kTile a-vectors that it copies to LDS laid out [a][MP].  Every lane of
// a wavefront reads the same a - identical addresses broadcast, no bank conflict - and two objectives come with one 16-byte
// read.  a dominates b when a[m] <= b[m] for all m and not a[m] >= b[m] for all m (IEEE compares: -0.0 == +0.0, equal
// vectors do not dominate each other).  The a range is split over blockIdx.y so that 4096 geometries still fill the card
// (grid 16 x 64); every split adds its int32 count into d_dominated[b] with one integer atomic per lane - integer sums carry
// the same bits in any order.
// Compaction pass (okx_front_compact): a workgroup owns gpb consecutive geometries, counts the front members before them
// (d_dominated == 0) and walks its own in ascending order with ballot + prefix counts (enstable::kept_before): a
// member's slot is what lies before it - no atomic decides a position.  It writes the id and the raw table values of the
// member's objectives; the last workgroup writes the tally (seen, candidates, front members).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/okx.h"
#include "okx_enstable.hpp"
#include "okx_program.hpp"

#pragma clang fp contract(off)

namespace okx {
namespace frt {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 64;                 // a-vectors per LDS tile
constexpr int kMaxM = OKX_ENS_FRONT_MAX_OBJECTIVES;
constexpr long long kWantGroups = 1024;   // workgroups the all-pairs pass aims at (four per CU of a 256-CU part, from the sizes alone)
constexpr long long kCompactRows = 1024;  // geometries per workgroup of the compaction pass

constexpr int padded(int m) { return m == 1 ? 1 : (m + 1) & ~1; }

struct Plan {
  long long rows;      // G rounded up to a multiple of kTile: the rows of the objective table in scratch
  long long tiles;     // rows / kTile
  long long b_blocks;  // workgroups along b
  long long splits;    // workgroups along a (blockIdx.y)
  long long tiles_per_split;
  long long groups;    // workgroups of the compaction pass
};

inline Plan plan_for(long long n_geom, int n_obj) {
  (void)n_obj;  // (the tile holds kTile vectors whatever M is; M only sets the row length)
  Plan p{};
  if (n_geom <= 0) return p;
  p.tiles = (n_geom + kTile - 1) / kTile;
  p.rows = p.tiles * kTile;
  p.b_blocks = (n_geom + kThreads - 1) / kThreads;
  long long want = (kWantGroups + p.b_blocks - 1) / p.b_blocks;
  if (want > p.tiles) want = p.tiles;
  p.tiles_per_split = (p.tiles + want - 1) / want;
  p.splits = (p.tiles + p.tiles_per_split - 1) / p.tiles_per_split;
  p.groups = (n_geom + kCompactRows - 1) / kCompactRows;
  return p;
}

// the selected entries as kernel arguments: (step, column) of entry s * n_columns + k, sense and target
struct Objectives {
  int step[kMaxM], column[kMaxM], sense[kMaxM];
  double target[kMaxM];
  int n;
};

struct GatherArgs {
  const double* values;
  const unsigned char* status;
  const unsigned char* mask;
  double* obj;     // [rows][mp]
  int* dominated;  // [n_geom]
  long long ld, status_stride, mask_stride, n_geom, steps, rows;
  int mp;
  Objectives o;
};

__global__ __launch_bounds__(kThreads) void okx_front_gather(GatherArgs a) {
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= a.rows) return;
  double o[kMaxM];
  bool ok = g < a.n_geom && (!a.mask || a.mask[g * a.mask_stride] == 0);
#pragma unroll
  for (int m = 0; m < kMaxM; ++m) {
    o[m] = 0.0;
    if (ok && m < a.o.n) {
      const long long row = g * a.steps + a.o.step[m];
      const double v = a.values[row * a.ld + a.o.column[m]];
      if (!OKX_ENS_ACCEPTED(OKX_ENS_STATUS_AT(a.status, row, a.status_stride), v)) ok = false;
      const int sense = a.o.sense[m];
      o[m] = sense == OKX_FRONT_MAX ? -v : sense == OKX_FRONT_TARGET ? __builtin_fabs(v - a.o.target[m]) : v;
    }
  }
  double* out = a.obj + g * a.mp;
#pragma unroll
  for (int m = 0; m < kMaxM; ++m)
    if (m < a.mp) out[m] = ok ? o[m] : __builtin_nan("");
  if (g < a.n_geom) a.dominated[g] = ok ? 0 : -1;
}

template <int M>
__global__ __launch_bounds__(kThreads) void okx_front_pairs(const double* __restrict__ obj, int* __restrict__ dominated, long long n_geom,
                                                             long long tiles, long long tiles_per_split) {
  constexpr int MP = padded(M);
  __shared__ __attribute__((aligned(16))) double tile[kTile * MP];
  const long long b = (long long)blockIdx.x * kThreads + threadIdx.x;
  double ob[M];
#pragma unroll
  for (int m = 0; m < M; ++m) ob[m] = b < n_geom ? obj[b * MP + m] : __builtin_nan("");
  const long long t0 = (long long)blockIdx.y * tiles_per_split;
  const long long t1 = t0 + tiles_per_split < tiles ? t0 + tiles_per_split : tiles;
  int count = 0;
  for (long long t = t0; t < t1; ++t) {
    __syncthreads();  // (the tile before may still be read)
    for (int i = threadIdx.x; i < kTile * MP; i += kThreads) tile[i] = obj[t * (kTile * MP) + i];  // rows < plan.rows: always there
    __syncthreads();
#pragma unroll 8
    for (int a = 0; a < kTile; ++a) {
      bool le = true, ge = true;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const double x = tile[a * MP + m];
        le = le & (x <= ob[m]);
        ge = ge & (x >= ob[m]);
      }
      count += (le & !ge) ? 1 : 0;
    }
  }
  // (a lane whose b is no candidate holds NaN: nothing was counted)
  if (count != 0) atomicAdd(&dominated[b], count);
}

struct CompactArgs {
  const int* dominated;
  const double* values;
  const long long* index;  // or null
  long long* tally;        // [3]
  long long* front_index;  // [cap_index] or null
  double* front_values;    // [cap_values][n] or null
  long long ld, n_geom, steps, groups, cap_index, cap_values, geometry_offset;
  Objectives o;
};

__global__ __launch_bounds__(kThreads) void okx_front_compact(CompactArgs a) {
  __shared__ long long sums[kWaves];
  __shared__ unsigned wave_n[kWaves];
  const long long blk = blockIdx.x;
  const bool last = blk + 1 >= a.groups;  // (groups == 0: the one workgroup launched)
  const long long g0 = blk * kCompactRows;
  const long long g1 = g0 + kCompactRows < a.n_geom ? g0 + kCompactRows : a.n_geom;
  long long before = 0, candidates = 0;
  for (long long i = threadIdx.x; i < g0 && i < a.n_geom; i += kThreads) {
    const int d = a.dominated[i];
    before += d == 0 ? 1 : 0;
    candidates += d >= 0 ? 1 : 0;
  }
  before = enstable::block_sum<kWaves>(before, sums);
  long long at = before;  // the slot of the next front member of this workgroup
  for (long long gc = g0; gc < g1; gc += kThreads) {
    const long long g = gc + threadIdx.x;
    const int d = g < g1 ? a.dominated[g] : -1;
    const bool member = d == 0;
    candidates += d >= 0 ? 1 : 0;
    unsigned all;
    const long long slot = at + enstable::kept_before<kWaves>(member, wave_n, &all);
    if (member) {
      if (a.front_index && slot < a.cap_index) a.front_index[slot] = a.index ? a.index[g] : a.geometry_offset + g;
      if (a.front_values && slot < a.cap_values) {
        double* out = a.front_values + slot * a.o.n;
#pragma unroll
        for (int m = 0; m < kMaxM; ++m)
          if (m < a.o.n) out[m] = a.values[(g * a.steps + a.o.step[m]) * a.ld + a.o.column[m]];  // the raw table bits
      }
    }
    at += all;
  }
  if (last) {
    candidates = enstable::block_sum<kWaves>(candidates, sums);
    if (threadIdx.x == 0) {
      a.tally[0] = a.n_geom;
      a.tally[1] = candidates;
      a.tally[2] = at;  // the members before this workgroup and in it
    }
  }
}

template <int M>
int launch_pairs(const Plan& p, const double* obj, int* dominated, long long n_geom, hipStream_t stream) {
  OKX_LAUNCH(okx_front_pairs<M>, dim3((unsigned)p.b_blocks, (unsigned)p.splits), dim3(kThreads), 0, stream, obj, dominated, n_geom, p.tiles,
             p.tiles_per_split);
  return OKX_OK;
}

// what okx_ensemble_front_check reports; `o` (or null) takes the entries apart for the kernels
inline int check_objectives(const char* who, long long n_geom, long long steps, int n_columns, const int32_t* entries, const int32_t* sense,
                            const double* target, int n_obj, Objectives* o) {
  if (int rc = enstable::check_counts(who, n_geom, steps, n_columns)) return rc;
  if (n_geom > OKX_ENS_FRONT_MAX_GEOMETRIES)
    return fail(OKX_ERR_INVALID, "%s: %lld geometries, at most %d in one call (chunk and merge)", who, n_geom, (int)OKX_ENS_FRONT_MAX_GEOMETRIES);
  if (n_obj < 1 || n_obj > kMaxM) return fail(OKX_ERR_INVALID, "%s: %d objectives, 1 to %d allowed", who, n_obj, kMaxM);
  if (!entries || !sense) return fail(OKX_ERR_INVALID, "%s: null entries or sense", who);
  const long long n_table = steps * (long long)n_columns;
  for (int m = 0; m < n_obj; ++m) {
    if (entries[m] < 0 || entries[m] >= n_table)
      return fail(OKX_ERR_INVALID, "%s: entry %d is %d, outside [0, %lld)", who, m, (int)entries[m], n_table);
    for (int j = 0; j < m; ++j)
      if (entries[j] == entries[m]) return fail(OKX_ERR_INVALID, "%s: entry %d repeats entry %d (index %d)", who, m, j, (int)entries[m]);
    if (sense[m] < OKX_FRONT_MIN || sense[m] > OKX_FRONT_TARGET)
      return fail(OKX_ERR_INVALID, "%s: sense %d is %d, not 0 (min), 1 (max) or 2 (target)", who, m, (int)sense[m]);
    if (sense[m] == OKX_FRONT_TARGET) {
      if (!target) return fail(OKX_ERR_INVALID, "%s: objective %d aims at a target and no targets are given", who, m);
      if (!std::isfinite(target[m])) return fail(OKX_ERR_INVALID, "%s: target %d is %g, not finite", who, m, target[m]);
    }
    if (o) {
      o->step[m] = (int)(entries[m] / n_columns);
      o->column[m] = (int)(entries[m] % n_columns);
      o->sense[m] = sense[m];
      o->target[m] = sense[m] == OKX_FRONT_TARGET ? target[m] : 0.0;
    }
  }
  if (o) o->n = n_obj;
  return OKX_OK;
}

}  // namespace frt
}  // namespace okx

using okx::fail;
namespace et = okx::enstable;

extern "C" {

size_t okx_ensemble_front_scratch_bytes(int64_t n_geometries, int32_t n_objectives) {
  namespace fr = okx::frt;
  if (n_geometries < 0 || n_objectives < 1 || n_objectives > fr::kMaxM) return 0;
  return 8 * (size_t)fr::plan_for(n_geometries, n_objectives).rows * (size_t)fr::padded(n_objectives);
}

int32_t okx_ensemble_front_check(int64_t n_geometries, int64_t steps, int32_t n_columns, const int32_t* entries, const int32_t* sense,
                                 const double* target, int32_t n_objectives) {
  return okx::frt::check_objectives("okx_ensemble_front", n_geometries, steps, n_columns, entries, sense, target, n_objectives, nullptr);
}

int32_t okx_ensemble_front(int64_t n_geometries, int64_t steps, int32_t n_columns, const double* d_values, int64_t ld, const uint8_t* d_status,
                           int64_t status_stride, const int32_t* entries, const int32_t* sense, const double* target, int32_t n_objectives,
                           const uint8_t* d_mask, int64_t mask_stride, const int64_t* d_index, int64_t geometry_offset, int32_t* d_dominated,
                           int64_t* d_tally, int64_t* d_front_index, double* d_front_values, int64_t capacity, void* d_scratch,
                           size_t scratch_bytes, void* stream) {
  namespace fr = okx::frt;
  const char* who = "okx_ensemble_front";
  fr::Objectives o{};
  if (int rc = fr::check_objectives(who, n_geometries, steps, n_columns, entries, sense, target, n_objectives, &o)) return rc;
  if (!d_tally) return fail(OKX_ERR_INVALID, "%s: null tally", who);
  if (n_geometries > 0 && !d_dominated) return fail(OKX_ERR_INVALID, "%s: null dominated table", who);
  if (int rc = et::check_table(who, n_geometries > 0, d_values, ld, n_columns, d_status, status_stride)) return rc;
  if (d_mask && mask_stride < 1) return fail(OKX_ERR_INVALID, "%s: mask_stride must be positive", who);
  if (capacity < 0) return fail(OKX_ERR_INVALID, "%s: negative capacity", who);
  const size_t need = okx_ensemble_front_scratch_bytes(n_geometries, n_objectives);
  if (need > 0)
    if (int rc = et::check_scratch(who, "okx_ensemble_front_scratch_bytes", need, d_scratch, scratch_bytes)) return rc;
  const fr::Plan plan = fr::plan_for(n_geometries, n_objectives);
  hipStream_t st = (hipStream_t)stream;
  double* obj = static_cast<double*>(d_scratch);
  const et::Table table = et::table_view(d_values, ld, d_status, status_stride, n_geometries, steps, n_columns);
  if (n_geometries > 0) {
    fr::GatherArgs g{};
    et::set_rows(&g, table);  // (the objectives carry their own step and column)
    g.status = table.status; g.status_stride = table.status_stride; g.mask = d_mask; g.mask_stride = d_mask ? mask_stride : 0;
    g.obj = obj; g.dominated = d_dominated; g.rows = plan.rows; g.mp = fr::padded(n_objectives); g.o = o;
    OKX_LAUNCH(fr::okx_front_gather, dim3((unsigned)((plan.rows + fr::kThreads - 1) / fr::kThreads)), dim3(fr::kThreads), 0, st, g);
    static constexpr decltype(&fr::launch_pairs<1>) kPairs[fr::kMaxM] = {  // (check_objectives: 1 <= n_objectives <= kMaxM)
        fr::launch_pairs<1>, fr::launch_pairs<2>, fr::launch_pairs<3>, fr::launch_pairs<4>,
        fr::launch_pairs<5>, fr::launch_pairs<6>, fr::launch_pairs<7>, fr::launch_pairs<8>};
    if (int rc = kPairs[n_objectives - 1](plan, obj, d_dominated, n_geometries, st)) return rc;
  }
  fr::CompactArgs c{};
  et::set_rows(&c, table);
  c.dominated = d_dominated; c.index = reinterpret_cast<const long long*>(d_index);
  c.tally = reinterpret_cast<long long*>(d_tally); c.front_index = reinterpret_cast<long long*>(d_front_index); c.front_values = d_front_values;
  c.groups = plan.groups; c.cap_index = d_front_index ? capacity : 0; c.cap_values = d_front_values ? capacity : 0;
  c.geometry_offset = geometry_offset; c.o = o;
  OKX_LAUNCH(fr::okx_front_compact, dim3((unsigned)(plan.groups > 0 ? plan.groups : 1)), dim3(fr::kThreads), 0, st, c);
  return OKX_OK;
}

}  // extern "C"
