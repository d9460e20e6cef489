// Sobol' accumulators (okx_ensemble_sobol, include/okx.h): over the FAMILIES of an evaluated pick-freeze ensemble - a table
// of metric columns [N * M * S][ld], family i's M = D + 2 geometries contiguous (member 0 = A, 1 = B, 2 + j = A with group
// j from B) - per (step, column) entry the counts, sum dA, sum dB, sum dA^2, sum dB^2 and per group j
//   P_j = sum dB (dj - dA),  Q_j = sum (dA - dj)^2,  R_j = sum (dB - dj)^2,   d = value - shift,
// over the families whose every member counts at that entry (okx_enstable.hpp's rule and the optional mask bytes).
//
// The pass streams the table once; what has to be right is traffic and registers.  As in okx_ensemble.hip a lane owns one
// entry e = s * K + k and walks families: every wave-instruction reads 64 consecutive doubles of one row (ld == K), and the
// sums live in registers.  3 D sums per lane do not fit (6 D VGPRs), so the groups are TILED: a workgroup - one wavefront -
// owns (tile of 64 entries, slab of families, tile of GT groups) and keeps 3 GT sums; GT is 4, 8, 12 or 16 (96 VGPRs of
// sums at most, no scratch memory: `make resource-usage`), the smallest multiple of 4 that spreads D evenly over
// ceil(D / 16) tiles - a function of D alone, and each P_j, Q_j, R_j is one lane's own chain of additions anyway, so no
// bit depends on the tiling.  Per family a lane loads A, B and its tile's GT members (slots past the last group read A
// again - a cache hit, and nobody stores their sums), and, when D > 16, tests the members of the other tiles for the
// counting rule; D <= 16 reads the table exactly once, D = 30 twice.  Tile 0 also carries the six common fields.
// Stage 1 (okx_sobol_partial) leaves one partial per (slab, field, entry) in scratch, families ascending; stage 2
// (okx_sobol_merge) adds the slabs in ascending order, after what d_acc holds when the call accumulates.  The slab plan
// never looks at the device, there is no floating-point atomic, and contraction is off for the unit (every difference and
// product rounded on its own, as ensemble_stats.sobol_host forms them): the bits repeat from run to run and from device to
// device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/okx.h"
#include "okx_enstable.hpp"
#include "okx_program.hpp"

#pragma clang fp contract(off)

namespace okx {
namespace sob {

constexpr int kTile = 64;                // entries per workgroup: one per lane, one wavefront
constexpr int kFields = OKX_SOBOL_FIELDS;
constexpr int kMaxTile = 16;             // groups a lane keeps sums for, at most
constexpr long long kMinSlab = 32;       // families: a slab's partial costs 3 / slab_len of the table it stands for, written and read
constexpr long long kWantGroups = 2048;  // stage-1 wavefronts aimed at (two per SIMD of a 256-CU part, from the problem size alone)

inline int group_tiles(int n_groups) { return (n_groups + kMaxTile - 1) / kMaxTile; }
// groups per tile: D spread evenly over its tiles, rounded up to a multiple of 4
inline int tile_groups(int n_groups) {
  const int tiles = group_tiles(n_groups);
  return ((n_groups + tiles - 1) / tiles + 3) / 4 * 4;
}

inline void slab_plan(long long n_families, long long n_entries, int n_groups, long long* n_slabs, long long* slab_len) {
  const long long want = (kWantGroups + group_tiles(n_groups) - 1) / group_tiles(n_groups);
  enstable::slab_plan(n_families, n_entries, kTile, want, kMinSlab, 65535, n_slabs, slab_len);
}

struct Args {
  const double* values;
  const unsigned char* status;
  const unsigned char* mask;  // [n_geom] or null
  const double* shift;
  double* partial;            // [n_slabs][kFields + 3 D][n_entries]
  long long ld, status_stride;
  long long n_geom, steps;    // n_geom = n_families * members
  long long n_families, n_entries, slab_len;
  int n_columns, n_groups, members;
};

template <int GT>
__global__ __launch_bounds__(kTile) void okx_sobol_partial(Args a) {
  const int lane = threadIdx.x;
  const long long e = (long long)blockIdx.x * kTile + lane;
  const bool live = e < a.n_entries;
  const long long er = live ? e : 0;  // a lane past the table walks entry 0 and stores nothing
  const long long slab = blockIdx.y;
  const int j0 = (int)blockIdx.z * GT;                                   // the tile's first group
  const int nj = a.n_groups - j0 < GT ? a.n_groups - j0 : GT;            // and how many it has (>= 1)
  const long long f0 = slab * a.slab_len;
  const long long f1 = f0 + a.slab_len < a.n_families ? f0 + a.slab_len : a.n_families;
  const enstable::Table t = OKX_ENS_TABLE_OF(a);
  const double* vp = enstable::entry_values(t, er);
  const unsigned char* sp = enstable::entry_status(t, er);
  const long long v_step = enstable::value_step(t), s_step = enstable::status_step(t);
  const double sh = a.shift[er];
  double count = 0.0, dropped = 0.0, sum_a = 0.0, sum_b = 0.0, sq_a = 0.0, sq_b = 0.0;
  double p[GT], q[GT], r[GT];
#pragma unroll
  for (int j = 0; j < GT; ++j) p[j] = q[j] = r[j] = 0.0;
  for (long long f = f0; f < f1; ++f) {
    const long long g = f * a.members;  // member 0; member m is geometry g + m < n_geom
    const double va = vp[g * v_step], vb = vp[(g + 1) * v_step];
    bool ok = OKX_ENS_ACCEPTED(OKX_ENS_STATUS_AT(sp, g, s_step), va) && OKX_ENS_ACCEPTED(OKX_ENS_STATUS_AT(sp, g + 1, s_step), vb);
    double vj[GT];
#pragma unroll
    for (int j = 0; j < GT; ++j) {
      const long long m = g + (j < nj ? 2 + j0 + j : 0);  // (uniform over the wavefront)
      vj[j] = vp[m * v_step];
      ok = ok && OKX_ENS_ACCEPTED(OKX_ENS_STATUS_AT(sp, m, s_step), vj[j]);
    }
    // the members of the other tiles: the counting rule alone
    for (int m = 2; m < a.members; ++m) {
      if (m == 2 + j0) { m += nj - 1; continue; }
      const double v = vp[(g + m) * v_step];
      ok = ok && OKX_ENS_ACCEPTED(OKX_ENS_STATUS_AT(sp, g + m, s_step), v);
    }
    if (a.mask) {  // (bytes uniform over the wavefront)
      unsigned bad = 0u;
      for (int m = 0; m < a.members; ++m) bad |= a.mask[g + m];
      ok = ok && (bad & 1u) == 0u;
    }
    count += ok ? 1.0 : 0.0;
    dropped += ok ? 0.0 : 1.0;
    if (!ok) continue;
    const double da = va - sh, db = vb - sh;
    sum_a += da;
    sum_b += db;
    sq_a += da * da;
    sq_b += db * db;
#pragma unroll
    for (int j = 0; j < GT; ++j) {
      const double dj = vj[j] - sh;
      const double ua = da - dj, ub = db - dj;
      p[j] += db * (dj - da);
      q[j] += ua * ua;
      r[j] += ub * ub;
    }
  }
  if (!live) return;
  const long long rows = kFields + 3ll * a.n_groups;
  double* out = a.partial + slab * rows * a.n_entries + e;
  if (blockIdx.z == 0) {
    out[OKX_SOBOL_COUNT * a.n_entries] = count; out[OKX_SOBOL_DROPPED * a.n_entries] = dropped;
    out[OKX_SOBOL_SUM_A * a.n_entries] = sum_a; out[OKX_SOBOL_SUM_B * a.n_entries] = sum_b;
    out[OKX_SOBOL_SUMSQ_A * a.n_entries] = sq_a; out[OKX_SOBOL_SUMSQ_B * a.n_entries] = sq_b;
  }
#pragma unroll
  for (int j = 0; j < GT; ++j)
    if (j < nj) {
      double* o = out + (kFields + 3ll * (j0 + j)) * a.n_entries;
      o[0] = p[j]; o[a.n_entries] = q[j]; o[2 * a.n_entries] = r[j];
    }
}

// One thread per (field, entry): the slabs in ascending order, after d_acc's own content when the call accumulates.
__global__ __launch_bounds__(256) void okx_sobol_merge(const double* partial, long long n_slabs, long long n_entries, int rows, int accumulate,
                                                       double* acc) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_entries * rows) return;
  const int field = (int)(t / n_entries);
  const long long e = t % n_entries;
  double* out = acc + e * rows + field;
  const double* in = partial + (long long)field * n_entries + e;
  const long long step = (long long)rows * n_entries;
  double x = accumulate ? *out : 0.0;
  // eight slabs' loads in flight, added in the same ascending order (one load, one wait, one add per slab left the pass
  // waiting on memory 128 times over at C5's shape)
  long long k = 0;
  for (; k + 8 <= n_slabs; k += 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = in[(k + i) * step];
#pragma unroll
    for (int i = 0; i < 8; ++i) x += v[i];
  }
  for (; k < n_slabs; ++k) x += in[k * step];
  *out = x;
}

template <int GT>
inline hipError_t launch_partial(const Args& a, long long n_slabs, hipStream_t st) {
  const unsigned tiles = (unsigned)((a.n_entries + kTile - 1) / kTile);
  hipLaunchKernelGGL(okx_sobol_partial<GT>, dim3(tiles, (unsigned)n_slabs, (unsigned)group_tiles(a.n_groups)), dim3(kTile), 0, st, a);
  return hipGetLastError();
}

inline int check_sizes(const char* who, long long n_families, int n_groups, long long steps, int n_columns) {
  if (int rc = enstable::check_counts(who, n_families, steps, n_columns)) return rc;
  if (n_groups < 1 || n_groups > OKX_ENS_SOBOL_MAX_GROUPS)
    return fail(OKX_ERR_INVALID, "%s: %d groups, 1 to %d allowed", who, n_groups, (int)OKX_ENS_SOBOL_MAX_GROUPS);
  if (n_families > (1ll << 53) / (n_groups + 2)) return fail(OKX_ERR_LIMIT, "%s: geometry indices beyond 2^53", who);
  return enstable::check_entries(who, steps, n_columns, (1ll << 38) / (kFields + 3 * n_groups));
}

}  // namespace sob
}  // namespace okx

using okx::fail;
namespace et = okx::enstable;

extern "C" {

size_t okx_ensemble_sobol_scratch_bytes(int64_t n_families, int32_t n_groups, int64_t steps, int32_t n_columns) {
  namespace sb = okx::sob;
  if (n_families <= 0 || steps < 0 || n_columns < 0 || n_groups < 1 || n_groups > OKX_ENS_SOBOL_MAX_GROUPS) return 0;
  const long long n_entries = (long long)steps * n_columns;
  long long n_slabs, slab_len;
  sb::slab_plan(n_families, n_entries, n_groups, &n_slabs, &slab_len);
  return sizeof(double) * (size_t)n_slabs * (size_t)(sb::kFields + 3 * n_groups) * (size_t)n_entries;
}

int32_t okx_ensemble_sobol(int64_t n_families, int32_t n_groups, int64_t steps, int32_t n_columns, const double* d_values, int64_t ld,
                           const uint8_t* d_status, int64_t status_stride, const uint8_t* d_mask, const double* d_shift, int32_t accumulate,
                           double* d_acc, void* d_scratch, size_t scratch_bytes, void* stream) {
  namespace sb = okx::sob;
  const char* who = "okx_ensemble_sobol";
  if (int rc = sb::check_sizes(who, n_families, n_groups, steps, n_columns)) return rc;
  const long long n_entries = (long long)steps * n_columns;
  if (n_entries > 0 && (!d_acc || !d_shift)) return fail(OKX_ERR_INVALID, "%s: null accumulator or shift table", who);
  if (int rc = et::check_table(who, n_entries > 0 && n_families > 0, d_values, ld, n_columns, d_status, status_stride)) return rc;
  const size_t need = okx_ensemble_sobol_scratch_bytes(n_families, n_groups, steps, n_columns);
  if (need > 0)
    if (int rc = et::check_scratch(who, "okx_ensemble_sobol_scratch_bytes", need, d_scratch, scratch_bytes)) return rc;
  if (n_entries == 0) return OKX_OK;
  long long n_slabs, slab_len;
  sb::slab_plan(n_families, n_entries, n_groups, &n_slabs, &slab_len);
  const hipStream_t st = (hipStream_t)stream;
  const int rows = sb::kFields + 3 * n_groups;
  double* partial = static_cast<double*>(d_scratch);
  if (n_slabs > 0) {
    const long long members = n_groups + 2;
    sb::Args a{};
    et::set_table(&a, et::table_view(d_values, ld, d_status, status_stride, n_families * members, steps, n_columns));
    a.mask = d_mask; a.shift = d_shift; a.partial = partial;
    a.n_families = n_families; a.n_entries = n_entries; a.slab_len = slab_len; a.n_groups = n_groups; a.members = (int)members;
    // the sums of a lane stay in registers: tiles of 4, 8, 12 or 16 groups, more than 16 as further workgroups
    switch (sb::tile_groups(n_groups)) {
      case 4: HIP_TRY(sb::launch_partial<4>(a, n_slabs, st)); break;
      case 8: HIP_TRY(sb::launch_partial<8>(a, n_slabs, st)); break;
      case 12: HIP_TRY(sb::launch_partial<12>(a, n_slabs, st)); break;
      default: HIP_TRY(sb::launch_partial<16>(a, n_slabs, st)); break;
    }
  }
  const long long threads = n_entries * rows;
  OKX_LAUNCH(sb::okx_sobol_merge, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, partial, n_slabs, n_entries, rows, accumulate ? 1 : 0,
             d_acc);
  return OKX_OK;
}

}  // extern "C"
