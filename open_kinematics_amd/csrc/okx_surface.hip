// Polynomial response surface of an ensemble (okx_ensemble_basis*, okx_ensemble_surface*, include/okx.h): the normal equations of a
// regression of N selected (step, column) entries of a table of metric columns [G * S][ld] on T basis terms of per-geometry factors.
//
// Basis pass (okx_surf_basis): a thread per (geometry, term), term fastest.  A workgroup owns 256 consecutive terms of ONE geometry: its
// threads first look at the row's n_factors factors together (one barrier) - a factor that is not finite makes the row invalid, its terms
// 0 -, then every thread forms u = (x - centre) * scale of its term's one or two factors, psi by the factor's kind and the term's degree
// and the product.  Every operation is rounded on its own (contraction is off for the unit): the bits of ensemble_stats.basis_host.
//
// Surface pass, okx_cov_gram's shape (okx_covariance.hip) over TWO operands, Phi [G][ld_phi] and D = value - shift of the entries:
// Used pass (okx_surf_used): okx_cov_used's vote - a wavefront per geometry strides its lanes over the selected entries - with the mask
// byte (bit 0) and the valid byte of the basis pass on top.
// Partial tiles (okx_surf_tile): one workgroup per (item, slab of geometries).  The items are the tile pairs I >= J of the lower triangle
// of Phi^T Phi in 64-term tiles, then the full rectangle Phi^T D in (64 terms) x (64 entries) tiles.  Panels [32 geometries][64] of both
// operands are staged in LDS - the row of a dropped geometry and the columns beyond T / N are zero - while the next panel's loads are in
// flight; the four wavefronts own 32 x 32 quarters of the tile as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64 with the operand layout
// okx_cov_gram documents (rows 80 doubles apart).  A diagonal pair stages one panel and skips the quarter above the diagonal.  A rectangle
// item of the FIRST term tile also sums d d of its D panel's columns (one wavefront, ascending geometries, product rounded, then added)
// for d_sumsq.  Partials go to d_scratch as [item][slab][64][64].
// Merge (okx_surf_merge): per element, after what the output holds when accumulating, the slabs in ascending order; a Gram total is
// written to both triangles.  One thread adds the used counts of the used pass's workgroups into d_counts.
//
// No floating-point atomic, no atomic on global memory: the slab plan and with it every addition order is a function of (G, T, N) alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/okx.h"
#include "okx_enstable.hpp"
#include "okx_gramtile.hpp"
#include "okx_program.hpp"
#include "okx_surfbasis.hpp"  // psi

#pragma clang fp contract(off)

namespace okx {
namespace surf {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 64;                 // terms / entries per tile side
constexpr int kBlock = 32;                // geometries per staged panel
constexpr int kRow = 80;                  // doubles between panel rows (okx_cov_gram: rows r and r + 1 on different bank halves)
constexpr long long kMinSlab = 128;       // geometries per slab at least (a multiple of kBlock)
constexpr long long kWantGroups = 1024;   // workgroups aimed at (four per CU of a 256-CU part, from the sizes alone)
constexpr long long kMaxTable = 1ll << 30;  // steps * n_columns
constexpr int kMaxFactors = OKX_ENS_SAMPLE_MAX_LATENTS;

typedef double d4 __attribute__((ext_vector_type(4)));

// ---- basis ----

struct BasisArgs {
  const double* factors;   // [n_geom][ld]
  const double* law;       // [n_factors][3]
  const int* terms;        // [n_terms][4]
  double* phi;             // [n_geom][ld_phi]
  unsigned char* valid;    // [n_geom]
  long long ld, ld_phi, n_geom;
  int n_factors, n_terms, term_groups;
};

__global__ __launch_bounds__(kThreads) void okx_surf_basis(BasisArgs a) {
  __shared__ int bad[kWaves];
  const long long g = blockIdx.x / a.term_groups;
  const int t = (int)(blockIdx.x % a.term_groups) * kThreads + threadIdx.x;
  const double* row = a.factors + g * a.ld;
  bool finite = true;
  for (int p = threadIdx.x; p < a.n_factors; p += kThreads) finite = finite && __builtin_isfinite(row[p]);
  const bool wave_bad = __ballot(!finite) != 0ull;
  if ((threadIdx.x & 63) == 0) bad[threadIdx.x >> 6] = wave_bad ? 1 : 0;
  __syncthreads();
  int any = 0;
  for (int w = 0; w < kWaves; ++w) any |= bad[w];
  const bool ok = any == 0;
  if (t == 0) a.valid[g] = ok ? 1 : 0;
  if (t >= a.n_terms) return;
  double v = 0.0;
  if (ok) {
    const int fa = a.terms[4 * t], da = a.terms[4 * t + 1], fb = a.terms[4 * t + 2], db = a.terms[4 * t + 3];
    double pa = 1.0, pb = 1.0;
    if (fa >= 0 && fa < a.n_factors) pa = psi((int)a.law[3 * fa], da, (row[fa] - a.law[3 * fa + 1]) * a.law[3 * fa + 2]);
    if (fb >= 0 && fb < a.n_factors) pb = psi((int)a.law[3 * fb], db, (row[fb] - a.law[3 * fb + 1]) * a.law[3 * fb + 2]);
    v = pa * pb;
  }
  a.phi[g * a.ld_phi + t] = v;
}

// ---- surface ----

struct Plan {
  int tt, tn;           // ceil(T / 64), ceil(N / 64)
  long long pairs;      // tt (tt + 1) / 2: the lower triangle of Phi^T Phi
  long long items;      // pairs + tt tn: then the rectangle Phi^T D, term tile by term tile
  long long slab_len;   // geometries per slab, a multiple of kBlock
  long long slabs;
  long long gpb;        // used pass: geometries per workgroup
  long long ugroups;    // used pass: workgroups
};

inline Plan plan_for(long long n_geom, long long t, long long n) {
  Plan p;
  p.tt = (int)((t + kTile - 1) / kTile);
  p.tn = (int)((n + kTile - 1) / kTile);
  p.pairs = (long long)p.tt * (p.tt + 1) / 2;
  p.items = p.pairs + (long long)p.tt * p.tn;
  p.slab_len = gramtile::slab_length(n_geom, p.items, kWantGroups, kBlock, kMinSlab);
  p.slabs = n_geom > 0 ? (n_geom + p.slab_len - 1) / p.slab_len : 0;
  p.gpb = enstable::geometries_per_group(n_geom, kWantGroups, kWaves);
  p.ugroups = n_geom > 0 ? (n_geom + p.gpb - 1) / p.gpb : 0;
  return p;
}

// d_scratch: uint8 used [G rounded up to 8] | int64 used count per workgroup of the used pass | double sums of squares
// [entry tile][slab][64] | double partial tiles [item][slab][64][64]
struct Layout {
  size_t used, totals, squares, tiles, bytes;
};

inline Layout layout_for(const Plan& p, long long n_geom) {
  Layout l;
  l.used = 0;
  l.totals = ((size_t)(n_geom > 0 ? n_geom : 0) + 7) / 8 * 8;
  l.squares = l.totals + 8 * (size_t)p.ugroups;
  l.tiles = l.squares + 8 * (size_t)p.tn * (size_t)p.slabs * kTile;
  l.bytes = l.tiles + 8 * (size_t)p.items * (size_t)p.slabs * kTile * kTile;
  return l;
}

struct UsedArgs {
  const double* values;
  const unsigned char* status;
  const unsigned char* mask;   // [n_geom] or null
  const unsigned char* valid;  // [n_geom]
  const int* entries;          // [n] or null
  unsigned char* used;         // d_scratch: [n_geom]
  unsigned char* used_out;     // d_used or null
  long long* totals;           // [ugroups]
  long long ld, status_stride, n_geom, steps, gpb;
  int n, n_columns, n_table;
};

__global__ __launch_bounds__(kThreads) void okx_surf_used(UsedArgs a) {
  __shared__ long long off[OKX_ENS_SURFACE_MAX_ENTRIES];  // s * ld + k of a selected entry; -1: no such entry (nothing counts)
  __shared__ int stp[OKX_ENS_SURFACE_MAX_ENTRIES];        // its step
  __shared__ unsigned wave_used[kWaves];
  const int K = a.n_columns > 0 ? a.n_columns : 1;
  for (int n = threadIdx.x; n < a.n; n += kThreads) {
    const int e = a.entries ? a.entries[n] : n;
    const bool valid = e >= 0 && e < a.n_table;
    const int s = valid ? e / K : 0;
    off[n] = valid ? (long long)s * a.ld + (e - s * K) : -1ll;
    stp[n] = s;
  }
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
    const bool open = (a.mask ? (a.mask[g] & 1u) == 0u : true) && a.valid[g] != 0;
    const bool all = __ballot(!ok) == 0ull && open;
    if (lane == 0) {
      a.used[g] = all ? 1 : 0;
      if (a.used_out) a.used_out[g] = all ? 1 : 0;
    }
    count += all ? 1u : 0u;
  }
  if (lane == 0) wave_used[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long total = 0;
    for (int w = 0; w < kWaves; ++w) total += wave_used[w];
    a.totals[blockIdx.x] = total;
  }
}

using gramtile::pair_of;  // pair p of the lower triangle, row by row: (0,0) (1,0) (1,1) (2,0) ...

struct TileArgs {
  const double* values;
  const double* phi;           // [n_geom][ld_phi]
  const int* entries;          // [n] or null
  const double* shift;         // [n_table]
  const unsigned char* used;   // [n_geom]
  double* part;                // [items][slabs][64][64]
  double* squares;             // [tn][slabs][64]
  long long ld, ld_phi, n_geom, steps, slab_len, slabs, pairs;
  int t, n, tn, n_columns, n_table;
};

__global__ __launch_bounds__(kThreads) void okx_surf_tile(TileArgs a) {
  __shared__ double pan[2][kBlock][kRow];
  __shared__ long long off[kTile];
  __shared__ double shf[kTile];
  const bool rect = (long long)blockIdx.x >= a.pairs;  // a tile of Phi^T D; else a tile pair of Phi^T Phi
  int ti, tj;
  if (rect) {
    const long long r = (long long)blockIdx.x - a.pairs;
    ti = (int)(r / a.tn);
    tj = (int)(r % a.tn);
  } else {
    pair_of(blockIdx.x, &ti, &tj);
  }
  const bool diag = !rect && ti == tj;
  const bool squares = rect && ti == 0;
  const long long slab = blockIdx.y;
  if (threadIdx.x < kTile) {  // (the offsets of a rectangle's entries; a pair reads none)
    const int K = a.n_columns > 0 ? a.n_columns : 1;
    const int n = tj * kTile + (int)threadIdx.x;
    long long o = -1ll;
    double sh = 0.0;
    if (rect && n < a.n) {
      const int e = a.entries ? a.entries[n] : n;
      if (e >= 0 && e < a.n_table) {
        const int s = e / K;
        o = (long long)s * a.ld + (e - s * K);
        sh = a.shift[e];
      }
    }
    off[threadIdx.x] = o;
    shf[threadIdx.x] = sh;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane, r0 = wave;  // staging: this thread's column and its rows r0, r0 + 4, ...
  const int term_i = ti * kTile + col, term_j = tj * kTile + col;
  const bool has_i = term_i < a.t, has_j = !rect && term_j < a.t;
  const long long o_j = off[col];
  const double sh_j = shf[col];
  const long long row_stride = a.steps * a.ld;
  const long long g_begin = slab * a.slab_len;
  const long long g_end = g_begin + a.slab_len < a.n_geom ? g_begin + a.slab_len : a.n_geom;
  constexpr int kMine = kBlock / kWaves;
  double ri[kMine], rj[kMine];
  auto load = [&](long long gb) {
#pragma unroll
    for (int i = 0; i < kMine; ++i) {
      const long long g = gb + r0 + kWaves * i;
      const bool u = g < g_end && a.used[g] != 0;  // (a used geometry: every selected entry of it is finite and its FACTORS are; its basis row is staged as it lies in d_phi)
      const double* pp = a.phi + g * a.ld_phi;
      ri[i] = u && has_i ? pp[term_i] : 0.0;
      if (rect) rj[i] = u && o_j >= 0 ? a.values[g * row_stride + o_j] - sh_j : 0.0;
      else if (!diag) rj[i] = u && has_j ? pp[term_j] : 0.0;
    }
  };
  const int wr = wave >> 1, wc = wave & 1;  // the wavefront's quarter of the tile
  const bool idle = diag && wc > wr;        // above the diagonal: never read
  const int li = lane & 15, lk = lane >> 4;
  const double (*pj)[kRow] = diag ? pan[0] : pan[1];
  d4 c00 = {0.0, 0.0, 0.0, 0.0}, c01 = c00, c10 = c00, c11 = c00;
  double sq = 0.0;
  load(g_begin);
  for (long long gb = g_begin; gb < g_end; gb += kBlock) {
#pragma unroll
    for (int i = 0; i < kMine; ++i) {
      pan[0][r0 + kWaves * i][col] = ri[i];
      if (!diag) pan[1][r0 + kWaves * i][col] = rj[i];
    }
    __syncthreads();
    if (gb + kBlock < g_end) load(gb + kBlock);  // in flight under the products
    if (!idle) {
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
    if (squares && wave == 1) {  // the D panel's sums of squares, ascending geometries: the product rounded, then added
#pragma unroll 8
      for (int r = 0; r < kBlock; ++r) {
        const double d = pan[1][r][lane];
        sq += d * d;
      }
    }
    __syncthreads();
  }
  double* out = a.part + ((long long)blockIdx.x * a.slabs + slab) * (kTile * kTile);
  if (!idle) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = wr * 32 + lk + 4 * reg, cl = wc * 32 + li;  // C[row = (l >> 4) + 4 reg][col = l & 15]
      out[row * kTile + cl] = c00[reg];
      out[row * kTile + cl + 16] = c01[reg];
      out[(row + 16) * kTile + cl] = c10[reg];
      out[(row + 16) * kTile + cl + 16] = c11[reg];
    }
  }
  if (squares && wave == 1) a.squares[((long long)tj * a.slabs + slab) * kTile + lane] = sq;
}

struct MergeArgs {
  const double* part;
  const double* squares;
  const long long* totals;  // [ugroups]
  double* gram;             // [t][t]
  double* cross;            // [t][n]
  double* sumsq;            // [n]
  long long* counts;        // [2]
  long long slabs, ugroups, n_geom, pairs;
  int t, n, tn, accumulate;
};

__global__ __launch_bounds__(kThreads) void okx_surf_merge(MergeArgs a) {
  __shared__ long long wave_sum[kWaves];
  const bool rect = (long long)blockIdx.x >= a.pairs;
  int ti, tj;
  if (rect) {
    const long long r = (long long)blockIdx.x - a.pairs;
    ti = (int)(r / a.tn);
    tj = (int)(r % a.tn);
  } else {
    pair_of(blockIdx.x, &ti, &tj);
  }
  const double* part = a.part + (long long)blockIdx.x * a.slabs * (kTile * kTile);
  {  // one element per thread: blockIdx.y cuts the tile into kTile * kTile / kThreads runs of rows
    const int idx = (int)blockIdx.y * kThreads + threadIdx.x;
    const int row = ti * kTile + (idx >> 6), cl = tj * kTile + (idx & 63);
    if (rect) {
      if (row < a.t && cl < a.n) {
        double t = a.accumulate ? a.cross[(long long)row * a.n + cl] : 0.0;
        for (long long s = 0; s < a.slabs; ++s) t += part[s * (kTile * kTile) + idx];
        a.cross[(long long)row * a.n + cl] = t;
      }
    } else if (row < a.t && cl <= row) {
      double t = a.accumulate ? a.gram[(long long)row * a.t + cl] : 0.0;
      for (long long s = 0; s < a.slabs; ++s) t += part[s * (kTile * kTile) + idx];
      a.gram[(long long)row * a.t + cl] = t;
      a.gram[(long long)cl * a.t + row] = t;
    }
  }
  if (blockIdx.y != 0) return;
  if (rect && ti == 0 && threadIdx.x < kTile) {
    const int n = tj * kTile + threadIdx.x;
    if (n < a.n) {
      double t = a.accumulate ? a.sumsq[n] : 0.0;
      for (long long s = 0; s < a.slabs; ++s) t += a.squares[((long long)tj * a.slabs + s) * kTile + threadIdx.x];
      a.sumsq[n] = t;
    }
  }
  if (blockIdx.x == 0) {
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

inline int check_terms(const char* who, long long n_terms) {
  if (n_terms < 1 || n_terms > OKX_ENS_SURFACE_MAX_TERMS)
    return fail(OKX_ERR_INVALID, "%s: %lld terms, 1 to %d allowed", who, n_terms, (int)OKX_ENS_SURFACE_MAX_TERMS);
  return OKX_OK;
}

inline int check_selected(const char* who, long long n) {
  if (n < 1 || n > OKX_ENS_SURFACE_MAX_ENTRIES)
    return fail(OKX_ERR_INVALID, "%s: %lld entries selected, 1 to %d allowed", who, n, (int)OKX_ENS_SURFACE_MAX_ENTRIES);
  return OKX_OK;
}

}  // namespace surf
}  // namespace okx

using okx::fail;
namespace et = okx::enstable;

extern "C" {

int32_t okx_ensemble_basis_check(const double* law, int32_t n_factors, const int32_t* terms, int32_t n_terms) {
  namespace sf = okx::surf;
  const char* who = "okx_ensemble_basis";
  if (int rc = sf::check_terms(who, n_terms)) return rc;
  if (n_factors < 1 || n_factors > sf::kMaxFactors)
    return fail(OKX_ERR_INVALID, "%s: %lld factors, 1 to %d allowed", who, (long long)n_factors, sf::kMaxFactors);
  if (!law || !terms) return fail(OKX_ERR_INVALID, "%s: null law or term table", who);
  for (int32_t p = 0; p < n_factors; ++p) {
    const double kind = law[3 * p], centre = law[3 * p + 1], scale = law[3 * p + 2];
    if (!(kind == OKX_SURFACE_MONOMIAL || kind == OKX_SURFACE_HERMITE || kind == OKX_SURFACE_LEGENDRE))
      return fail(OKX_ERR_INVALID, "%s: factor %lld has kind %g, not 0 (monomial), 1 (Hermite) or 2 (Legendre)", who, (long long)p, kind);
    if (!std::isfinite(centre) || !std::isfinite(scale))
      return fail(OKX_ERR_INVALID, "%s: factor %lld has a centre or scale that is not finite", who, (long long)p);
  }
  if (terms[0] != -1 || terms[1] != 0 || terms[2] != -1 || terms[3] != 0)
    return fail(OKX_ERR_INVALID, "%s: term 0 must be the constant (-1, 0, -1, 0)", who);
  for (int32_t t = 0; t < n_terms; ++t)
    for (int half = 0; half < 2; ++half) {
      const long long f = terms[4 * t + 2 * half], d = terms[4 * t + 2 * half + 1];
      if (f < -1 || f >= n_factors)
        return fail(OKX_ERR_INVALID, "%s: term %lld names factor %lld, outside [-1, %lld)", who, (long long)t, f, (long long)n_factors);
      if (f < 0 ? d != 0 : (d < 1 || d > OKX_ENS_SURFACE_MAX_DEGREE))
        return fail(OKX_ERR_INVALID, "%s: term %lld has degree %lld of factor %lld (0 without a factor, else 1 to %d)", who, (long long)t, d, f,
                    (int)OKX_ENS_SURFACE_MAX_DEGREE);
    }
  return OKX_OK;
}

int32_t okx_ensemble_basis(int64_t n_geometries, const double* d_factors, int64_t ld, int32_t n_factors, const double* d_law, const int32_t* d_terms,
                           int32_t n_terms, double* d_phi, int64_t ld_phi, uint8_t* d_valid, void* stream) {
  namespace sf = okx::surf;
  const char* who = "okx_ensemble_basis";
  if (int rc = et::check_counts(who, n_geometries, 0, 0)) return rc;
  if (int rc = sf::check_terms(who, n_terms)) return rc;
  if (n_factors < 1 || n_factors > sf::kMaxFactors)
    return fail(OKX_ERR_INVALID, "%s: %lld factors, 1 to %d allowed", who, (long long)n_factors, sf::kMaxFactors);
  const int groups = (n_terms + sf::kThreads - 1) / sf::kThreads;
  if (n_geometries > 0x7fffffffll / groups) return fail(OKX_ERR_LIMIT, "%s: too many geometries for one call", who);
  if (n_geometries == 0) return OKX_OK;
  if (!d_factors || ld < n_factors) return fail(OKX_ERR_INVALID, "%s: null factor table or ld < n_factors", who);
  if (!d_law || !d_terms) return fail(OKX_ERR_INVALID, "%s: null law or term table", who);
  if (!d_phi || ld_phi < n_terms || !d_valid) return fail(OKX_ERR_INVALID, "%s: null basis table, null valid bytes or ld_phi < n_terms", who);
  sf::BasisArgs a{};
  a.factors = d_factors; a.law = d_law; a.terms = d_terms; a.phi = d_phi; a.valid = d_valid;
  a.ld = ld; a.ld_phi = ld_phi; a.n_geom = n_geometries; a.n_factors = n_factors; a.n_terms = n_terms; a.term_groups = groups;
  OKX_LAUNCH(sf::okx_surf_basis, dim3((unsigned)(n_geometries * groups)), dim3(sf::kThreads), 0, (hipStream_t)stream, a);
  return OKX_OK;
}

size_t okx_ensemble_surface_scratch_bytes(int64_t n_geometries, int64_t steps, int32_t n_columns, int32_t n_terms, int32_t n_entries) {
  namespace sf = okx::surf;
  if (n_geometries < 0 || steps < 0 || n_columns < 0 || n_entries < 1 || n_entries > OKX_ENS_SURFACE_MAX_ENTRIES || n_terms < 1 ||
      n_terms > OKX_ENS_SURFACE_MAX_TERMS)
    return 0;
  const size_t bytes = sf::layout_for(sf::plan_for(n_geometries, n_terms, n_entries), n_geometries).bytes;
  return bytes < 8 ? 8 : bytes;
}

int32_t okx_ensemble_surface_check(const int32_t* entries, int32_t n_entries, int64_t n_table_entries, int32_t n_terms) {
  namespace sf = okx::surf;
  const char* who = "okx_ensemble_surface";
  if (int rc = sf::check_terms(who, n_terms)) return rc;
  return okx::gramtile::check_entry_list(who, entries, n_entries, n_table_entries, OKX_ENS_SURFACE_MAX_ENTRIES);
}

int32_t okx_ensemble_surface(int64_t n_geometries, int64_t steps, int32_t n_columns, const double* d_values, int64_t ld, const uint8_t* d_status,
                             int64_t status_stride, const uint8_t* d_mask, const double* d_phi, int64_t ld_phi, const uint8_t* d_valid, int32_t n_terms,
                             const int32_t* d_entries, int32_t n_entries, const double* d_shift, int32_t accumulate, double* d_gram, double* d_cross,
                             double* d_sumsq, int64_t* d_counts, uint8_t* d_used, void* d_scratch, size_t scratch_bytes, void* stream) {
  namespace sf = okx::surf;
  const char* who = "okx_ensemble_surface";
  if (int rc = et::check_counts(who, n_geometries, steps, n_columns)) return rc;
  if (int rc = et::check_entries(who, steps, n_columns, sf::kMaxTable, "entries in the table")) return rc;
  if (int rc = sf::check_terms(who, n_terms)) return rc;
  if (int rc = sf::check_selected(who, n_entries)) return rc;
  const long long n_table = (long long)steps * n_columns;
  if (!d_entries && n_entries != n_table)
    return fail(OKX_ERR_INVALID, "%s: without an entry list all %lld entries are selected, not %lld", who, n_table, (long long)n_entries);
  if (n_entries > n_table) return fail(OKX_ERR_INVALID, "%s: %lld distinct entries of a table of %lld", who, (long long)n_entries, n_table);
  if (!d_gram || !d_cross || !d_sumsq || !d_counts || !d_shift) return fail(OKX_ERR_INVALID, "%s: null gram, cross, sumsq, counts or shift", who);
  if (int rc = et::check_table(who, n_geometries > 0, d_values, ld, n_columns, d_status, status_stride)) return rc;
  if (n_geometries > 0 && (!d_phi || ld_phi < n_terms || !d_valid))
    return fail(OKX_ERR_INVALID, "%s: null basis table, null valid bytes or ld_phi < n_terms", who);
  const sf::Plan plan = sf::plan_for(n_geometries, n_terms, n_entries);
  const sf::Layout lay = sf::layout_for(plan, n_geometries);
  const size_t need = okx_ensemble_surface_scratch_bytes(n_geometries, steps, n_columns, n_terms, n_entries);
  if (int rc = et::check_scratch(who, "okx_ensemble_surface_scratch_bytes", need, d_scratch, scratch_bytes)) return rc;
  if (reinterpret_cast<uintptr_t>(d_scratch) % 8) return fail(OKX_ERR_INVALID, "%s: the scratch buffer must be 8-byte aligned", who);
  if (plan.ugroups > 0x7fffffffll) return fail(OKX_ERR_LIMIT, "%s: too many geometries for one call", who);
  unsigned char* base = static_cast<unsigned char*>(d_scratch);
  unsigned char* used = base + lay.used;
  long long* totals = reinterpret_cast<long long*>(base + lay.totals);
  double* squares = reinterpret_cast<double*>(base + lay.squares);
  double* part = reinterpret_cast<double*>(base + lay.tiles);
  if (n_geometries > 0) {
    const et::Table table = et::table_view(d_values, ld, d_status, status_stride, n_geometries, steps, n_columns);
    sf::UsedArgs u{};
    et::set_table(&u, table);
    u.mask = d_mask; u.valid = d_valid; u.entries = d_entries; u.used = used; u.used_out = d_used; u.totals = totals;
    u.gpb = plan.gpb; u.n = n_entries; u.n_table = (int)n_table;
    OKX_LAUNCH(sf::okx_surf_used, dim3((unsigned)plan.ugroups), dim3(sf::kThreads), 0, (hipStream_t)stream, u);
    sf::TileArgs g{};
    et::set_rows(&g, table);  // (the used bytes stand for the status table, the mask and the valid bytes)
    g.phi = d_phi; g.ld_phi = ld_phi; g.entries = d_entries; g.shift = d_shift; g.used = used; g.part = part; g.squares = squares;
    g.slab_len = plan.slab_len; g.slabs = plan.slabs; g.pairs = plan.pairs;
    g.t = n_terms; g.n = n_entries; g.tn = plan.tn; g.n_columns = n_columns; g.n_table = (int)n_table;
    OKX_LAUNCH(sf::okx_surf_tile, dim3((unsigned)plan.items, (unsigned)plan.slabs), dim3(sf::kThreads), 0, (hipStream_t)stream, g);
  }
  sf::MergeArgs m{};
  m.part = part; m.squares = squares; m.totals = totals; m.gram = d_gram; m.cross = d_cross; m.sumsq = d_sumsq;
  m.counts = reinterpret_cast<long long*>(d_counts);
  m.slabs = plan.slabs; m.ugroups = plan.ugroups; m.n_geom = n_geometries; m.pairs = plan.pairs;
  m.t = n_terms; m.n = n_entries; m.tn = plan.tn; m.accumulate = accumulate != 0;
  OKX_LAUNCH(sf::okx_surf_merge, dim3((unsigned)plan.items, sf::kTile * sf::kTile / sf::kThreads), dim3(sf::kThreads), 0, (hipStream_t)stream, m);
  return OKX_OK;
}

}  // extern "C"
