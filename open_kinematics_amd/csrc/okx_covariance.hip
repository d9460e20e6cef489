// Ensemble covariance (okx_ensemble_covariance*, include/okx.h): over the geometries of a table of metric columns
// [G * S][ld], the Gram matrix sum d_n d_m and the sums sum d_n of N selected (step, column) entries, d = value - shift,
// over the COMPLETE cases - the geometries whose every selected entry counts by the acceptance rule (okx_enstable.hpp).
//
// The first ensemble pass with real arithmetic: a symmetric rank-G update, N^2 G flop for the lower triangle, where
// okx_ensemble.hip / okx_select.hip / okx_screen.hip stream.  Three launches:
//
// Used pass (okx_cov_used): a workgroup builds the offset table of the selected entries in LDS from d_entries (s * ld + k
// and s, one division per entry and workgroup), then one wavefront per geometry strides its lanes over the entries - 64
// consecutive doubles where the entries are consecutive -, tests value and status byte and votes.  The used byte goes to
// d_scratch (and to d_used); a workgroup owns gpb consecutive geometries and leaves its used count in d_scratch.
// Partial Gram (okx_cov_gram): one workgroup per (tile pair I >= J of the lower triangle in 64-entry tiles, slab of
// geometries).  It stages panels [32 geometries][64 entries] of masked, shifted d in LDS - the row of a dropped geometry
// and the columns beyond N are zero, so they add nothing - while the next panel's loads are in flight, and its four
// wavefronts each own a 32 x 32 quarter of the tile as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64: lane l feeds
// A[l & 15][k = l >> 4] = d[geometry k][entry of I] and B[k = l >> 4][l & 15] = d[geometry k][entry of J], one
// ds_read_b64 each from rows 80 doubles apart (16 lanes per row, rows r and r + 1 on different bank halves), and holds
// C[row = (l >> 4) + 4 reg][col = l & 15].  A diagonal pair stages one panel, skips the quarter above the diagonal and
// sums its panel's columns (ascending geometries) for d_sum.  Partials go to d_scratch as [pair][slab][64][64].
// Merge (okx_cov_merge): per element n >= m, after what d_gram holds when accumulating, the slabs in ascending order; the
// one total is written to both triangles, so gram[n][m] and gram[m][n] are the same bits.  The same for d_sum; one thread
// adds the used counts of the workgroups into d_counts.
//
// No floating-point atomic, no atomic on global memory at all: the slab plan and with it every addition order is a function
// of (G, S, K, N) alone (plan_for never looks at the device).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../include/okx.h"
#include "okx_enstable.hpp"
#include "okx_gramtile.hpp"
#include "okx_program.hpp"
#include "okx_quad.hpp"

#pragma clang fp contract(off)

namespace okx {
namespace cov {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 64;                 // entries per tile side
constexpr int kBlock = 32;                // geometries per staged panel
constexpr int kRow = 80;                  // doubles between panel rows: 64 + 16, rows r and r + 1 on different bank halves
constexpr long long kMinSlab = 128;       // geometries per slab at least (a multiple of kBlock)
constexpr long long kWantGroups = 1024;   // workgroups aimed at (four per CU of a 256-CU part, from the sizes alone)
constexpr long long kMaxTable = 1ll << 30;  // steps * n_columns

typedef double d4 __attribute__((ext_vector_type(4)));

struct Plan {
  int tiles;            // ceil(N / 64)
  long long pairs;      // tiles (tiles + 1) / 2
  long long slab_len;   // geometries per slab, a multiple of kBlock
  long long slabs;
  long long gpb;        // used pass: geometries per workgroup
  long long ugroups;    // used pass: workgroups
};

inline Plan plan_for(long long n_geom, long long n) {
  Plan p;
  p.tiles = (int)((n + kTile - 1) / kTile);
  p.pairs = (long long)p.tiles * (p.tiles + 1) / 2;
  p.slab_len = gramtile::slab_length(n_geom, p.pairs, kWantGroups, kBlock, kMinSlab);
  p.slabs = n_geom > 0 ? (n_geom + p.slab_len - 1) / p.slab_len : 0;
  p.gpb = enstable::geometries_per_group(n_geom, kWantGroups, kWaves);
  p.ugroups = n_geom > 0 ? (n_geom + p.gpb - 1) / p.gpb : 0;
  return p;
}

// d_scratch: uint8 used [G rounded up to 8] | int64 used count per workgroup of the used pass | double sums [tile][slab][64]
// | double partial Gram tiles [pair][slab][64][64]
struct Layout {
  size_t used, totals, sums, tiles, bytes;
};

inline Layout layout_for(const Plan& p, long long n_geom) {
  Layout l;
  l.used = 0;
  l.totals = ((size_t)(n_geom > 0 ? n_geom : 0) + 7) / 8 * 8;
  l.sums = l.totals + 8 * (size_t)p.ugroups;
  l.tiles = l.sums + 8 * (size_t)p.tiles * (size_t)p.slabs * kTile;
  l.bytes = l.tiles + 8 * (size_t)p.pairs * (size_t)p.slabs * kTile * kTile;
  return l;
}

struct UsedArgs {
  const double* values;
  const unsigned char* status;
  const int* entries;        // [n] or null
  unsigned char* used;       // d_scratch: [n_geom]
  unsigned char* used_out;   // d_used or null
  long long* totals;         // [ugroups]
  long long ld, status_stride, n_geom, steps, gpb;
  int n, n_columns, n_table;
};

__global__ __launch_bounds__(kThreads) void okx_cov_used(UsedArgs a) {
  __shared__ long long off[OKX_ENS_COV_MAX_ENTRIES];  // s * ld + k of a selected entry; -1: no such entry (nothing counts)
  __shared__ int stp[OKX_ENS_COV_MAX_ENTRIES];        // its step
  __shared__ unsigned n_used;
  const int K = a.n_columns > 0 ? a.n_columns : 1;
  for (int n = threadIdx.x; n < a.n; n += kThreads) {
    const int e = a.entries ? a.entries[n] : n;
    const bool valid = e >= 0 && e < a.n_table;
    const int s = valid ? e / K : 0;
    off[n] = valid ? (long long)s * a.ld + (e - s * K) : -1ll;
    stp[n] = s;
  }
  if (threadIdx.x == 0) n_used = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long g0 = (long long)blockIdx.x * a.gpb;
  const long long g1 = g0 + a.gpb < a.n_geom ? g0 + a.gpb : a.n_geom;
  const enstable::Table tab = OKX_ENS_TABLE_OF(a);
  unsigned count = 0u;  // wave-uniform
  for (long long g = g0 + wave; g < g1; g += kWaves) {
    const double* vp = enstable::geometry_values(tab, g);
    const unsigned char* sp = enstable::geometry_status(tab, g);
    bool ok = true;
    for (int n = lane; n < a.n; n += 64) {
      const long long o = off[n];
      if (o < 0) { ok = false; continue; }
      const double v = vp[o];
      const unsigned st = OKX_ENS_STATUS_AT(sp, stp[n], a.status_stride);
      ok = ok && OKX_ENS_ACCEPTED(st, v);
    }
    const bool all = __ballot(!ok) == 0ull;
    if (lane == 0) {
      a.used[g] = all ? 1 : 0;
      if (a.used_out) a.used_out[g] = all ? 1 : 0;
    }
    count += all ? 1u : 0u;
  }
  if (lane == 0 && count != 0u) atomicAdd(&n_used, count);  // (LDS, integers)
  __syncthreads();
  if (threadIdx.x == 0) a.totals[blockIdx.x] = (long long)n_used;
}

using gramtile::pair_of;  // pair p of the lower triangle, row by row: (0,0) (1,0) (1,1) (2,0) ...

struct GramArgs {
  const double* values;
  const int* entries;          // [n] or null
  const double* shift;         // [n_table]
  const unsigned char* used;   // [n_geom]
  double* part;                // [pairs][slabs][64][64]
  double* sums;                // [tiles][slabs][64]
  long long ld, n_geom, steps, slab_len, slabs;
  int n, n_columns, n_table;
};

// kMfma = false: the register-tiled v_fma_f64 form of the same pass, kept to be measured against (OKX_DEV=cov_valu,
// tools/ensemble_covariance_rate.py): thread (ty, tx) = (t >> 4, t & 15) owns the 4 x 4 block at (4 ty, 4 tx) of the tile and adds
// one geometry after the other - the same panels, partials and merge; its bits differ from the matrix form's by rounding.
template <bool kMfma>
__global__ __launch_bounds__(kThreads) void okx_cov_gram(GramArgs a) {
  __shared__ double pan[2][kBlock][kRow];
  __shared__ long long off[2][kTile];
  __shared__ double shf[2][kTile];
  int ti, tj;
  pair_of(blockIdx.x, &ti, &tj);
  const bool diag = ti == tj;
  const long long slab = blockIdx.y;
  if (threadIdx.x < 2 * kTile) {
    const int which = threadIdx.x >> 6, c = threadIdx.x & 63;
    const int K = a.n_columns > 0 ? a.n_columns : 1;
    const int n = (which ? tj : ti) * kTile + c;
    long long o = -1ll;
    double sh = 0.0;
    if (n < a.n) {
      const int e = a.entries ? a.entries[n] : n;
      if (e >= 0 && e < a.n_table) {
        const int s = e / K;
        o = (long long)s * a.ld + (e - s * K);
        sh = a.shift[e];
      }
    }
    off[which][c] = o;
    shf[which][c] = sh;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane, r0 = wave;  // staging: this thread's column and its rows r0, r0 + 4, ...
  const long long o_i = off[0][col], o_j = off[1][col];
  const double sh_i = shf[0][col], sh_j = shf[1][col];
  const long long row_stride = a.steps * a.ld;
  const long long g_begin = slab * a.slab_len;
  const long long g_end = g_begin + a.slab_len < a.n_geom ? g_begin + a.slab_len : a.n_geom;
  constexpr int kMine = kBlock / kWaves;
  double ri[kMine], rj[kMine];
  auto load = [&](long long gb) {
#pragma unroll
    for (int i = 0; i < kMine; ++i) {
      const long long g = gb + r0 + kWaves * i;
      const bool u = g < g_end && a.used[g] != 0;  // (a used geometry: every selected entry of it exists and is finite)
      const double* vp = a.values + g * row_stride;
      ri[i] = u && o_i >= 0 ? vp[o_i] - sh_i : 0.0;
      if (!diag) rj[i] = u && o_j >= 0 ? vp[o_j] - sh_j : 0.0;
    }
  };
  const int wr = wave >> 1, wc = wave & 1;  // the wavefront's quarter of the tile
  const bool idle = kMfma && diag && wc > wr;  // above the diagonal: never read
  const int li = lane & 15, lk = lane >> 4;
  const double (*pj)[kRow] = diag ? pan[0] : pan[1];
  d4 c00 = {0.0, 0.0, 0.0, 0.0}, c01 = c00, c10 = c00, c11 = c00;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  double acc[4][4] = {};
  double sum = 0.0;
  load(g_begin);
  for (long long gb = g_begin; gb < g_end; gb += kBlock) {
#pragma unroll
    for (int i = 0; i < kMine; ++i) {
      pan[0][r0 + kWaves * i][col] = ri[i];
      if (!diag) pan[1][r0 + kWaves * i][col] = rj[i];
    }
    __syncthreads();
    if (gb + kBlock < g_end) load(gb + kBlock);  // in flight under the products
    if (!kMfma) {
#pragma unroll 4
      for (int r = 0; r < kBlock; ++r) {
        double av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { av[i] = pan[0][r][4 * ty + i]; bv[i] = pj[r][4 * tx + i]; }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fma(av[i], bv[j], acc[i][j]);
      }
    } else if (!idle) {
#pragma unroll
      for (int kk = 0; kk < kBlock; kk += 4) {
        const double a0 = pan[0][kk + lk][wr * 32 + li], a1 = pan[0][kk + lk][wr * 32 + 16 + li];
        const double b0 = pj[kk + lk][wc * 32 + li], b1 = pj[kk + lk][wc * 32 + 16 + li];
        c00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, c00, 0, 0, 0);
        c01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, c01, 0, 0, 0);
        c10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, c10, 0, 0, 0);
        c11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, c11, 0, 0, 0);
      }
    }
    if (diag && wave == 1) {  // (the idle wavefront of a diagonal pair) the panel's column sums, ascending geometries
#pragma unroll 8
      for (int r = 0; r < kBlock; ++r) sum += pan[0][r][lane];
    }
    __syncthreads();
  }
  double* out = a.part + ((long long)blockIdx.x * a.slabs + slab) * (kTile * kTile);
  if (!kMfma) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) out[(4 * ty + i) * kTile + 4 * tx + j] = acc[i][j];
  } else if (!idle) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = wr * 32 + lk + 4 * reg, cl = wc * 32 + li;  // C[row = (l >> 4) + 4 reg][col = l & 15]
      out[row * kTile + cl] = c00[reg];
      out[row * kTile + cl + 16] = c01[reg];
      out[(row + 16) * kTile + cl] = c10[reg];
      out[(row + 16) * kTile + cl + 16] = c11[reg];
    }
  }
  if (diag && wave == 1) a.sums[((long long)ti * a.slabs + slab) * kTile + lane] = sum;
}

struct MergeArgs {
  const double* part;
  const double* sums;
  const long long* totals;  // [ugroups]
  double* gram;             // [n][n]
  double* sum;              // [n]
  long long* counts;        // [2]
  long long slabs, ugroups, n_geom;
  int n, accumulate;
};

__global__ __launch_bounds__(kThreads) void okx_cov_merge(MergeArgs a) {
  __shared__ long long wave_sum[kWaves];
  int ti, tj;
  pair_of(blockIdx.x, &ti, &tj);
  const double* part = a.part + (long long)blockIdx.x * a.slabs * (kTile * kTile);
  {  // one element per thread: blockIdx.y cuts the tile into kTile * kTile / kThreads runs of rows
    const int idx = (int)blockIdx.y * kThreads + threadIdx.x;
    const int n = ti * kTile + (idx >> 6), m = tj * kTile + (idx & 63);
    if (n < a.n && m <= n) {
      double t = a.accumulate ? a.gram[(long long)n * a.n + m] : 0.0;
      for (long long s = 0; s < a.slabs; ++s) t += part[s * (kTile * kTile) + idx];
      a.gram[(long long)n * a.n + m] = t;
      a.gram[(long long)m * a.n + n] = t;
    }
  }
  if (blockIdx.y != 0) return;
  if (ti == tj && threadIdx.x < kTile) {
    const int n = ti * kTile + threadIdx.x;
    if (n < a.n) {
      double t = a.accumulate ? a.sum[n] : 0.0;
      for (long long s = 0; s < a.slabs; ++s) t += a.sums[((long long)ti * a.slabs + s) * kTile + threadIdx.x];
      a.sum[n] = t;
    }
  }
  if (blockIdx.x == 0) {  // (its own workgroup sum: only thread 0 wants it, so one barrier and no broadcast - enstable::block_sum has two)
    long long used = 0;
    for (long long i = threadIdx.x; i < a.ugroups; i += kThreads) used += a.totals[i];
    for (int o = 32; o > 0; o >>= 1) used += __shfl_xor(used, o);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = used;
    __syncthreads();
    if (threadIdx.x == 0) {
      used = 0;
      for (int w = 0; w < kWaves; ++w) used += wave_sum[w];
      a.counts[0] = (a.accumulate ? a.counts[0] : 0ll) + used;
      a.counts[1] = (a.accumulate ? a.counts[1] : 0ll) + (a.n_geom - used);
    }
  }
}

inline int check_sizes(const char* who, long long n_geom, long long steps, int n_columns, long long n) {
  if (int rc = enstable::check_counts(who, n_geom, steps, n_columns)) return rc;
  if (int rc = enstable::check_entries(who, steps, n_columns, kMaxTable, "entries in the table")) return rc;
  if (n < 1 || n > OKX_ENS_COV_MAX_ENTRIES)
    return fail(OKX_ERR_INVALID, "%s: %lld entries selected, 1 to %d allowed", who, n, (int)OKX_ENS_COV_MAX_ENTRIES);
  return OKX_OK;
}

}  // namespace cov
}  // namespace okx

using okx::fail;
namespace et = okx::enstable;

extern "C" {

size_t okx_ensemble_covariance_scratch_bytes(int64_t n_geometries, int64_t steps, int32_t n_columns, int32_t n_entries) {
  namespace cv = okx::cov;
  if (n_geometries < 0 || steps < 0 || n_columns < 0 || n_entries < 1 || n_entries > OKX_ENS_COV_MAX_ENTRIES) return 0;
  const size_t bytes = cv::layout_for(cv::plan_for(n_geometries, n_entries), n_geometries).bytes;
  return bytes < 8 ? 8 : bytes;
}

int32_t okx_ensemble_covariance_check(const int32_t* entries, int32_t n_entries, int64_t n_table_entries) {
  return okx::gramtile::check_entry_list("okx_ensemble_covariance", entries, n_entries, n_table_entries, OKX_ENS_COV_MAX_ENTRIES);
}

int32_t okx_ensemble_covariance(int64_t n_geometries, int64_t steps, int32_t n_columns, const double* d_values, int64_t ld, const uint8_t* d_status,
                                int64_t status_stride, const int32_t* d_entries, int32_t n_entries, const double* d_shift, int32_t accumulate,
                                double* d_gram, double* d_sum, int64_t* d_counts, uint8_t* d_used, void* d_scratch, size_t scratch_bytes,
                                void* stream) {
  namespace cv = okx::cov;
  const char* who = "okx_ensemble_covariance";
  if (int rc = cv::check_sizes(who, n_geometries, steps, n_columns, n_entries)) return rc;
  const long long n_table = (long long)steps * n_columns;
  if (!d_entries && n_entries != n_table)
    return fail(OKX_ERR_INVALID, "%s: without an entry list all %lld entries are selected, not %lld", who, n_table, (long long)n_entries);
  if (n_entries > n_table) return fail(OKX_ERR_INVALID, "%s: %lld distinct entries of a table of %lld", who, (long long)n_entries, n_table);
  if (!d_gram || !d_sum || !d_counts || !d_shift) return fail(OKX_ERR_INVALID, "%s: null gram, sum, counts or shift", who);
  if (int rc = et::check_table(who, n_geometries > 0, d_values, ld, n_columns, d_status, status_stride)) return rc;
  const cv::Plan plan = cv::plan_for(n_geometries, n_entries);
  const cv::Layout lay = cv::layout_for(plan, n_geometries);
  const size_t need = okx_ensemble_covariance_scratch_bytes(n_geometries, steps, n_columns, n_entries);
  if (int rc = et::check_scratch(who, "okx_ensemble_covariance_scratch_bytes", need, d_scratch, scratch_bytes)) return rc;
  if (plan.ugroups > 0x7fffffffll) return fail(OKX_ERR_LIMIT, "%s: too many geometries for one call", who);
  unsigned char* base = static_cast<unsigned char*>(d_scratch);
  unsigned char* used = base + lay.used;
  long long* totals = reinterpret_cast<long long*>(base + lay.totals);
  double* sums = reinterpret_cast<double*>(base + lay.sums);
  double* part = reinterpret_cast<double*>(base + lay.tiles);
  if (n_geometries > 0) {
    const et::Table table = et::table_view(d_values, ld, d_status, status_stride, n_geometries, steps, n_columns);
    cv::UsedArgs u{};
    et::set_table(&u, table);
    u.entries = d_entries; u.used = used; u.used_out = d_used; u.totals = totals;
    u.gpb = plan.gpb; u.n = n_entries; u.n_table = (int)n_table;
    OKX_LAUNCH(cv::okx_cov_used, dim3((unsigned)plan.ugroups), dim3(cv::kThreads), 0, (hipStream_t)stream, u);
    cv::GramArgs g{};
    et::set_rows(&g, table);  // (the used bytes stand for the status table)
    g.entries = d_entries; g.shift = d_shift; g.used = used; g.part = part; g.sums = sums;
    g.slab_len = plan.slab_len; g.slabs = plan.slabs; g.n = n_entries; g.n_columns = n_columns; g.n_table = (int)n_table;
    const bool valu = std::getenv("OKX_DEV") != nullptr && okx::dev_switch("cov_valu");  // (one look at the environment per launch)
    const dim3 grid((unsigned)plan.pairs, (unsigned)plan.slabs);
    if (valu) OKX_LAUNCH(cv::okx_cov_gram<false>, grid, dim3(cv::kThreads), 0, (hipStream_t)stream, g);
    else OKX_LAUNCH(cv::okx_cov_gram<true>, grid, dim3(cv::kThreads), 0, (hipStream_t)stream, g);
  }
  cv::MergeArgs m{};
  m.part = part; m.sums = sums; m.totals = totals; m.gram = d_gram; m.sum = d_sum; m.counts = reinterpret_cast<long long*>(d_counts);
  m.slabs = plan.slabs; m.ugroups = plan.ugroups; m.n_geom = n_geometries; m.n = n_entries; m.accumulate = accumulate != 0;
  OKX_LAUNCH(cv::okx_cov_merge, dim3((unsigned)plan.pairs, cv::kTile * cv::kTile / cv::kThreads), dim3(cv::kThreads), 0, (hipStream_t)stream, m);
  return OKX_OK;
}

}  // extern "C"
