// Evaluation of a polynomial response surface (okx_ensemble_predict*, include/okx.h): out[g][n] = shift[n] + sum_t psi_t(factors[g]) c[t][n]
// for G geometries, T basis terms and N entries - or, in RESIDUAL mode, the table's value of entry n minus that - as ONE launch that never
// writes the basis values Phi [G][T] to memory.
//
// okx_pred_tile is okx_surf_tile's tile (okx_surface.hip) turned by one index: there the geometries are summed over (k) and the tile is
// terms x entries; here the TERMS are summed over and a workgroup owns a tile of 64 geometries x 64 entries.  It walks the terms in panels
// of 32, ascending.  For each panel its threads form the basis values of (32 terms) x (64 geometries) straight into LDS - the psi of
// okx_surfbasis.hpp, contraction off, every operation rounded: the bits of okx_surf_basis - and stage the coefficient panel (32 terms) x
// (64 entries) beside it; the terms beyond T, the columns beyond N and the rows of dropped geometries are zero.  The four wavefronts own
// 32 x 32 quarters of the tile as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64 with the operand layout okx_cov_gram documents (lane l
// feeds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15] from rows 80 doubles apart; C[(l >> 4) + 4 reg][l & 15]): A is now
// [geometry][term], B [term][entry], k the term.  The next panel's values - the coefficient loads, the term and law words, and the factor
// loads where they come from memory - are formed into registers under the products of the current one.
//
// How the factor values reach the threads: a staging thread owns ONE geometry (its lane) and eight wave-uniform terms of a panel, so the
// term words and the law are scalar loads and a basis value needs the thread's own x[fa], x[fb].  Up to kLdsFactors = 40 factors the 64
// factor rows of the workgroup are read once, coalesced, into a transposed tile [factor][65] in (dynamic) LDS beside the panels - 62 KB at
// the most, so two workgroups still share a CU - and x[f] is a conflict-free LDS read.  With more factors (up to 288 rows of 64 would be
// 147 KB) the rows stay where they are and x[f] is a load from memory per term and lane, served by L2: slower, the same bits.  Either way
// the first sweep over the rows also decides whether all n_factors of a row are finite.
//
// The bits.  An output is sum over the panels in ascending order, inside a panel whatever the matrix instruction does with its four
// terms at a time, from an accumulator that starts at 0; then shift + sum in one rounded addition; then (RESIDUAL) value - that in one
// rounded subtraction.  Nothing of this depends on G, on where the row lies in the call or in its block, on a leading dimension, on N or
// on another launch: a geometry's row is a function of its factors, the basis, the coefficients and the shift alone (ROW-PURE).
// No scratch, no atomics, one launch.
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
namespace pred {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 64;          // entries per tile
constexpr int kGeom = 64;          // geometries per tile
constexpr int kPanel = 32;         // terms per staged panel
constexpr int kRow = 80;           // doubles between panel rows (okx_cov_gram: rows r and r + 1 on different bank halves)
constexpr int kLdsFactors = 40;    // factor rows of at most this many factors are staged in LDS
constexpr int kXRow = kGeom + 1;   // doubles between the rows of the transposed factor tile
constexpr int kMaxFactors = OKX_ENS_SAMPLE_MAX_LATENTS;
constexpr long long kMaxTable = 1ll << 30;  // steps * n_columns

typedef double d4 __attribute__((ext_vector_type(4)));

struct TileArgs {
  const double* values;         // RESIDUAL: the table
  const unsigned char* status;
  const double* factors;        // [n_geom][ld_x]
  const double* law;            // [p][3]
  const int* terms;             // [t][4]
  const double* coef;           // [t][ld_c]
  const double* shift;          // [n] or null
  const unsigned char* mask;    // [n_geom] or null
  const int* entries;           // [n] or null
  double* out;                  // [n_geom][ld_out]
  unsigned char* valid;         // [n_geom]
  long long ld, status_stride, n_geom, steps;
  long long ld_x, ld_c, ld_out;
  int n_columns, n_table, p, t, n, tn, residual, x_in_lds;
};

__global__ __launch_bounds__(kThreads) void okx_pred_tile(TileArgs a) {
  extern __shared__ double xs[];  // [p][kXRow] when x_in_lds: factor f of the tile's geometry r at xs[f * kXRow + r]
  __shared__ double pan[2][kPanel][kRow];
  __shared__ long long off[kTile];  // RESIDUAL: s * ld + k of the tile's entry; -1: no such entry
  __shared__ int stp[kTile];        // its step
  __shared__ double shf[kTile];
  __shared__ int bad[kGeom];        // the geometry is beyond the call, masked, or has a factor that is not finite
  const long long gblock = (long long)blockIdx.x / a.tn;
  const int tj = (int)((long long)blockIdx.x % a.tn);
  const long long g0 = gblock * kGeom;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (threadIdx.x < kTile) {
    const int K = a.n_columns > 0 ? a.n_columns : 1;
    const int n = tj * kTile + (int)threadIdx.x;
    long long o = -1ll;
    int s = 0;
    double sh = 0.0;
    if (n < a.n) {
      if (a.shift) sh = a.shift[n];
      if (a.residual) {
        const int e = a.entries ? a.entries[n] : n;
        if (e >= 0 && e < a.n_table) {
          s = e / K;
          o = (long long)s * a.ld + (e - s * K);
        }
      }
    }
    off[threadIdx.x] = o;
    stp[threadIdx.x] = s;
    shf[threadIdx.x] = sh;
    const long long g = g0 + threadIdx.x;
    bad[threadIdx.x] = g >= a.n_geom || (a.mask && (a.mask[g] & 1u) != 0u) ? 1 : 0;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < kGeom * a.p; idx += kThreads) {  // the factor rows, coalesced: finite? and the tile into LDS
    const int r = idx / a.p, f = idx - r * a.p;
    const long long g = g0 + r;
    if (g < a.n_geom) {
      const double x = a.factors[g * a.ld_x + f];
      if (!__builtin_isfinite(x)) bad[r] = 1;  // (every writer stores the same word)
      if (a.x_in_lds) xs[f * kXRow + r] = x;
    }
  }
  __syncthreads();
  // staging: this thread's column - geometry `lane` of the basis panel, entry `lane` of the coefficient panel - and its rows
  // (terms) wave, wave + 4, ...: a row's term is the same in every lane
  const bool ok = bad[lane] == 0;
  const double* xrow = a.factors + (g0 + lane) * a.ld_x;  // (read only where ok: then g0 + lane < n_geom)
  const int n_mine = tj * kTile + lane;
  const bool has_n = n_mine < a.n;
  constexpr int kMine = kPanel / kWaves;
  double ri[kMine], rj[kMine];
  auto factor = [&](int f) { return a.x_in_lds ? xs[f * kXRow + lane] : xrow[f]; };
  auto load = [&](int t0) {
#pragma unroll
    for (int i = 0; i < kMine; ++i) {
      const int t = t0 + wave + kWaves * i;
      double v = 0.0, c = 0.0;
      if (t < a.t) {
        const int fa = a.terms[4 * t], da = a.terms[4 * t + 1], fb = a.terms[4 * t + 2], db = a.terms[4 * t + 3];
        const bool ha = fa >= 0 && fa < a.p, hb = fb >= 0 && fb < a.p;
        if (ok) {
          double pa = 1.0, pb = 1.0;
          if (ha) pa = surf::psi((int)a.law[3 * fa], da, (factor(fa) - a.law[3 * fa + 1]) * a.law[3 * fa + 2]);
          if (hb) pb = surf::psi((int)a.law[3 * fb], db, (factor(fb) - a.law[3 * fb + 1]) * a.law[3 * fb + 2]);
          v = pa * pb;
        }
        if (has_n) c = a.coef[(long long)t * a.ld_c + n_mine];
      }
      ri[i] = v;
      rj[i] = c;
    }
  };
  const int wr = wave >> 1, wc = wave & 1;  // the wavefront's quarter of the tile: geometries wr * 32 .., entries wc * 32 ..
  const int li = lane & 15, lk = lane >> 4;
  d4 c00 = {0.0, 0.0, 0.0, 0.0}, c01 = c00, c10 = c00, c11 = c00;
  load(0);
  for (int t0 = 0; t0 < a.t; t0 += kPanel) {
#pragma unroll
    for (int i = 0; i < kMine; ++i) {
      pan[0][wave + kWaves * i][lane] = ri[i];
      pan[1][wave + kWaves * i][lane] = rj[i];
    }
    __syncthreads();
    if (t0 + kPanel < a.t) load(t0 + kPanel);  // in flight under the products
#pragma unroll
    for (int kk = 0; kk < kPanel; kk += 4) {
      const double a0 = pan[0][kk + lk][wr * 32 + li], a1 = pan[0][kk + lk][wr * 32 + 16 + li];
      const double b0 = pan[1][kk + lk][wc * 32 + li], b1 = pan[1][kk + lk][wc * 32 + 16 + li];
      c00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, c00, 0, 0, 0);
      c01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, c01, 0, 0, 0);
      c10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, c10, 0, 0, 0);
      c11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, c11, 0, 0, 0);
    }
    __syncthreads();
  }
  const enstable::Table tab = OKX_ENS_TABLE_OF(a);
  auto store = [&](int r, int cl, double sum) {  // C[r = geometry of the tile][cl = entry of the tile]
    const long long g = g0 + r;
    const int n = tj * kTile + cl;
    if (g >= a.n_geom || n >= a.n) return;
    double v = shf[cl] + sum;
    if (bad[r]) {
      v = __builtin_nan("");
    } else if (a.residual) {
      const long long o = off[cl];
      bool counts = false;
      double value = 0.0;
      if (o >= 0) {
        value = enstable::geometry_values(tab, g)[o];
        const unsigned char* sp = enstable::geometry_status(tab, g);
        const unsigned st = OKX_ENS_STATUS_AT(sp, stp[cl], a.status_stride);
        counts = OKX_ENS_ACCEPTED(st, value);
      }
      v = counts ? value - v : __builtin_nan("");
    }
    a.out[g * a.ld_out + n] = v;
  };
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = wr * 32 + lk + 4 * reg, cl = wc * 32 + li;  // C[row = (l >> 4) + 4 reg][col = l & 15]
    store(row, cl, c00[reg]);
    store(row, cl + 16, c01[reg]);
    store(row + 16, cl, c10[reg]);
    store(row + 16, cl + 16, c11[reg]);
  }
  if (tj == 0 && threadIdx.x < kGeom && g0 + threadIdx.x < a.n_geom) a.valid[g0 + threadIdx.x] = bad[threadIdx.x] ? 0 : 1;
}

inline int check_sizes(const char* who, long long n_terms, long long n_entries, long long n_factors) {
  if (n_terms < 1 || n_terms > OKX_ENS_SURFACE_MAX_TERMS)
    return fail(OKX_ERR_INVALID, "%s: %lld terms, 1 to %d allowed", who, n_terms, (int)OKX_ENS_SURFACE_MAX_TERMS);
  if (n_entries < 1 || n_entries > OKX_ENS_SURFACE_MAX_ENTRIES)
    return fail(OKX_ERR_INVALID, "%s: %lld entries, 1 to %d allowed", who, n_entries, (int)OKX_ENS_SURFACE_MAX_ENTRIES);
  if (n_factors < 1 || n_factors > kMaxFactors) return fail(OKX_ERR_INVALID, "%s: %lld factors, 1 to %d allowed", who, n_factors, kMaxFactors);
  return OKX_OK;
}

}  // namespace pred
}  // namespace okx

using okx::fail;
namespace et = okx::enstable;

extern "C" {

int32_t okx_ensemble_predict_check(const int32_t* entries, int32_t n_entries, int64_t n_table_entries, int32_t n_terms, int32_t n_factors) {
  const char* who = "okx_ensemble_predict";
  if (int rc = okx::pred::check_sizes(who, n_terms, n_entries, n_factors)) return rc;
  if (n_table_entries < 0) return fail(OKX_ERR_INVALID, "%s: negative table size", who);
  if (n_table_entries == 0 && !entries) return OKX_OK;  // VALUE mode: no table
  return okx::gramtile::check_entry_list(who, entries, n_entries, n_table_entries, OKX_ENS_SURFACE_MAX_ENTRIES);
}

int32_t okx_ensemble_predict(int64_t n_geometries, int32_t mode, const double* d_factors, int64_t ld, int32_t n_factors, const double* d_law,
                             const int32_t* d_terms, int32_t n_terms, const double* d_coefficients, int64_t ld_c, int32_t n_entries,
                             const double* d_shift, const uint8_t* d_mask, int64_t steps, int32_t n_columns, const double* d_values, int64_t ld_values,
                             const uint8_t* d_status, int64_t status_stride, const int32_t* d_entries, double* d_out, int64_t ld_out, uint8_t* d_valid,
                             void* stream) {
  namespace pd = okx::pred;
  const char* who = "okx_ensemble_predict";
  if (mode != OKX_PREDICT_VALUE && mode != OKX_PREDICT_RESIDUAL)
    return fail(OKX_ERR_INVALID, "%s: mode %lld, not OKX_PREDICT_VALUE (0) or OKX_PREDICT_RESIDUAL (1)", who, (long long)mode);
  const bool residual = mode == OKX_PREDICT_RESIDUAL;
  if (n_geometries < 0) return fail(OKX_ERR_INVALID, "%s: negative geometry count", who);
  if (int rc = pd::check_sizes(who, n_terms, n_entries, n_factors)) return rc;
  long long n_table = 0;
  if (residual) {
    if (int rc = et::check_counts(who, n_geometries, steps, n_columns)) return rc;
    if (int rc = et::check_entries(who, steps, n_columns, pd::kMaxTable, "entries in the table")) return rc;
    n_table = (long long)steps * n_columns;
    if (!d_values) return fail(OKX_ERR_INVALID, "%s: OKX_PREDICT_RESIDUAL needs the table (d_values is null)", who);
    if (!d_entries && n_entries != n_table)
      return fail(OKX_ERR_INVALID, "%s: without an entry list all %lld entries are selected, not %lld", who, n_table, (long long)n_entries);
    if (int rc = et::check_table(who, true, d_values, ld_values, n_columns, d_status, status_stride)) return rc;
  }
  const long long tn = (n_entries + pd::kTile - 1) / pd::kTile;
  const long long blocks = (n_geometries + pd::kGeom - 1) / pd::kGeom;
  if (blocks > 0x7fffffffll / tn) return fail(OKX_ERR_LIMIT, "%s: too many geometries for one call", who);
  if (n_geometries == 0) return OKX_OK;
  if (!d_out || !d_valid) return fail(OKX_ERR_INVALID, "%s: null output table or null valid bytes", who);
  if (ld_out < n_entries) return fail(OKX_ERR_INVALID, "%s: ld_out < n_entries", who);
  if (!d_factors || ld < n_factors) return fail(OKX_ERR_INVALID, "%s: null factor table or ld < n_factors", who);
  if (!d_law || !d_terms) return fail(OKX_ERR_INVALID, "%s: null law or term table", who);
  if (!d_coefficients || ld_c < n_entries) return fail(OKX_ERR_INVALID, "%s: null coefficient table or ld_c < n_entries", who);
  pd::TileArgs a{};
  if (residual) {
    const et::Table table = et::table_view(d_values, ld_values, d_status, status_stride, n_geometries, steps, n_columns);
    et::set_table(&a, table);
    a.entries = d_entries;
  }
  a.n_geom = n_geometries;
  a.factors = d_factors; a.law = d_law; a.terms = d_terms; a.coef = d_coefficients; a.shift = d_shift; a.mask = d_mask;
  a.out = d_out; a.valid = d_valid; a.ld_x = ld; a.ld_c = ld_c; a.ld_out = ld_out;
  a.n_table = (int)n_table; a.p = n_factors; a.t = n_terms; a.n = n_entries; a.tn = (int)tn; a.residual = residual ? 1 : 0;
  a.x_in_lds = n_factors <= pd::kLdsFactors ? 1 : 0;
  const size_t lds = a.x_in_lds ? sizeof(double) * (size_t)n_factors * pd::kXRow : 0;
  OKX_LAUNCH(pd::okx_pred_tile, dim3((unsigned)(blocks * tn)), dim3(pd::kThreads), lds, (hipStream_t)stream, a);
  return OKX_OK;
}

}  // extern "C"
