// Ensemble curves (okx_ensemble_curves*, include/okx.h): per GEOMETRY and column of a table of metric columns [G * S][ld],
// the characteristics of the curve the column draws ALONG the sweep - a least-squares polynomial of degree D <= 3 in
// u = (x - origin) / scale over the used steps (value, gradient, curvature at the origin), the rms and the largest residual,
// the extremes and where they occur, the abscissa range covered - as OKX_CURVE_FIELDS doubles [G][K][12] that stay in HBM: a
// column table with one step per geometry for the other ensemble passes.
//
// Like okx_screen.hip the reduction runs inside ONE geometry, whose rows are contiguous when ld == K.  A group of L lanes
// owns a geometry, laid out [step slice][column]: CL = the power of two >= K (at most 64) lanes side by side hold the columns
// of one step, SL slices (a power of two, CL * SL <= 64, no more than the power of two >= S) take the steps sl, sl + SL, ...
// - a wavefront reads consecutive doubles - and 64 / L geometries share a wavefront when the table is small; more than 64
// columns go in blocks of 64.  The plan is a function of (S, K) alone, never of G or of the device: a geometry's outputs
// depend on its own rows only and are bit-identical from run to run, across chunkings, devices and ranks.
//
// First walk: a lane keeps one column, so its sums live in registers - n, sum u^i (i <= 2 D), sum u^i (y - y0) (i <= D) with y0
// the lane's own first used value, and (value, step, abscissa) of the extremes.  u and its powers are computed once per step
// (multiplications by 1 / scale: no division in the loop); the abscissa belongs to the geometry, the lanes of a step share
// it.  The group then agrees on y_ref, the used value of the lowest step, every lane moves its sums there
// (sum u^i (y - y_ref) = sum u^i (y - y0) + (y0 - y_ref) sum u^i) and the slices add up by xor-shuffles in a fixed order (no
// atomics, no LDS): every lane ends with the same bits, and every lane solves.
// Solve: Cholesky of the (D + 1) x (D + 1) normal matrix N_ij = sum u^(i + j) in registers.  THE FIT IS REFUSED when a pivot
// N_jj - sum_k L_jk^2 is not greater than 2^-40 times its diagonal entry N_jj (all-equal abscissae end there), and undefined
// with fewer than D + 1 used steps: fields 0 .. 5 are then NaN.
// Second walk over the same rows (L2: one geometry of 256 steps x 4 columns is 8 KB) for the residuals
// r = (y - y_ref) - p(u): sum r^2 and max |r|, reduced the same way.
//
// Fields 6 .. 11 and the count are comparisons and copies of table bits; nothing in this file is contracted - the fused
// multiply-adds of the sums are written out.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/okx.h"
#include "okx_enstable.hpp"
#include "okx_program.hpp"

#pragma clang fp contract(off)

namespace okx {
namespace crv {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr long long kMaxGroups = 8192;  // workgroups at most (a wavefront strides over the geometries beyond)
constexpr int kNoStep = 0x7fffffff;

struct Plan {
  int col_lanes;  // CL: lanes side by side over the columns, power of two, 1 .. 64
  int slices;     // SL: step slices, power of two, CL * SL <= 64
};

inline Plan plan_for(long long steps, int n_columns) {
  Plan p;
  p.col_lanes = 1;
  while (p.col_lanes < 64 && p.col_lanes < n_columns) p.col_lanes <<= 1;
  p.slices = 1;
  while (p.col_lanes * p.slices < 64 && p.slices < steps) p.slices <<= 1;
  return p;
}

struct Args {
  const double* values;
  const unsigned char* status;
  const double* abscissa;  // [S] or null: column x_column of the table
  double* features;        // [G][K][12]
  int* count;              // [G][K]
  long long ld, status_stride, n_geom, steps;
  double origin, scale, inv_scale, lo, hi;
  int n_columns, x_column, col_lanes, col_shift, slices;
};

// (value, step) of an extreme with the lowest step on ties, and what travels with it
struct Extreme {
  double v, x;
  int s;
};

__device__ inline void take_lower(Extreme& e, double v, int s, double x) {
  if (v < e.v || e.s == kNoStep) { e.v = v; e.s = s; e.x = x; }  // ascending s: a tie keeps the lower step
}
__device__ inline void take_higher(Extreme& e, double v, int s, double x) {
  if (v > e.v || e.s == kNoStep) { e.v = v; e.s = s; e.x = x; }
}
__device__ inline void merge_extreme(Extreme& e, int off, bool lower) {
  const double ov = __shfl_xor(e.v, off), ox = __shfl_xor(e.x, off);
  const int os = __shfl_xor(e.s, off);
  if (os == kNoStep) return;
  const bool better = lower ? ov < e.v : ov > e.v;
  if (e.s == kNoStep || better || (ov == e.v && os < e.s)) { e.v = ov; e.s = os; e.x = ox; }
}

// Cholesky solve of N a = b, N_ij = su[i + j] (su[0] = n), in registers; false: refused
template <int D>
__device__ inline bool solve_normal(const double* su, const double* sy, double* a) {
  double low[D + 1][D + 1];
#pragma unroll
  for (int j = 0; j <= D; ++j) {
    double d = su[2 * j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= low[j][k] * low[j][k];
    if (!(d > 0x1p-40 * su[2 * j])) return false;
    low[j][j] = sqrt(d);
#pragma unroll
    for (int i = j + 1; i <= D; ++i) {
      double s = su[i + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= low[i][k] * low[j][k];
      low[i][j] = s / low[j][j];
    }
  }
  double z[D + 1];
#pragma unroll
  for (int i = 0; i <= D; ++i) {
    double s = sy[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= low[i][k] * z[k];
    z[i] = s / low[i][i];
  }
#pragma unroll
  for (int i = D; i >= 0; --i) {
    double s = z[i];
#pragma unroll
    for (int k = i + 1; k <= D; ++k) s -= low[k][i] * a[k];
    a[i] = s / low[i][i];
  }
  return true;
}

template <int D>
__global__ __launch_bounds__(kThreads) void okx_curves_fit(Args a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int CL = a.col_lanes, SL = a.slices, L = CL * SL, pack = 64 / L;
  const int t = lane & (L - 1), sub = lane / L;
  const int kc = t & (CL - 1), sl = t >> a.col_shift;
  const int K = a.n_columns;
  const long long S = a.steps;
  const double nan = __builtin_nan("");
  for (long long gb = ((long long)blockIdx.x * kWaves + wave) * pack; gb < a.n_geom; gb += (long long)gridDim.x * kWaves * pack) {
    const long long g = gb + sub;
    for (int k0 = 0; k0 < K; k0 += CL) {  // (wave-uniform: every lane takes every shuffle)
      const int k = k0 + kc;
      const bool live = g < a.n_geom && k < K;
      const double* vp = a.values + g * S * a.ld;  // (enstable's walk 2, written out: through the view this kernel's text moves)
      const unsigned char* sp = a.status ? a.status + g * S * a.status_stride : nullptr;
      // ---- first walk: this lane's steps of its column ----
      double su[2 * D + 1], sy[D + 1];
#pragma unroll
      for (int i = 0; i <= 2 * D; ++i) su[i] = 0.0;
#pragma unroll
      for (int i = 0; i <= D; ++i) sy[i] = 0.0;
      int n = 0, first = kNoStep;
      double y0 = 0.0;
      Extreme ymin{0.0, 0.0, kNoStep}, ymax{0.0, 0.0, kNoStep}, xlo{0.0, 0.0, kNoStep}, xhi{0.0, 0.0, kNoStep};
      if (live) {
#pragma unroll 4
        for (long long s = sl; s < S; s += SL) {
          const double* row = vp + s * a.ld;
          const double y = row[k];
          const double x = a.abscissa ? a.abscissa[s] : row[a.x_column];
          const unsigned st = OKX_ENS_STATUS_AT(sp, s, a.status_stride);
          // a used step: the state and the value accepted; the abscissa finite and inside the closed window
          if (!(OKX_ENS_ACCEPTED(st, y) && __builtin_isfinite(x) && x >= a.lo && x <= a.hi)) continue;
          if (n == 0) { y0 = y; first = (int)s; }
          ++n;
          take_lower(ymin, y, (int)s, x);
          take_higher(ymax, y, (int)s, x);
          take_lower(xlo, x, (int)s, x);
          take_higher(xhi, x, (int)s, x);
          const double u = (x - a.origin) * a.inv_scale, d = y - y0;
          sy[0] += d;
          if constexpr (D >= 1) {
            double p[2 * D + 1];
            p[1] = u;
#pragma unroll
            for (int i = 2; i <= 2 * D; ++i) p[i] = p[i / 2] * p[i - i / 2];
#pragma unroll
            for (int i = 1; i <= 2 * D; ++i) su[i] += p[i];
#pragma unroll
            for (int i = 1; i <= D; ++i) sy[i] = __builtin_fma(p[i], d, sy[i]);
          }
        }
      }
      su[0] = (double)n;
      // ---- y_ref: the used value of the lowest step of the group's column; the lane's sums moved there ----
      int lowest = first;
      double yref = y0;
      for (int off = CL; off < L; off <<= 1) {
        const int of = __shfl_xor(lowest, off);
        const double oy = __shfl_xor(yref, off);
        if (of < lowest) { lowest = of; yref = oy; }
      }
      const double shift = n > 0 ? y0 - yref : 0.0;
#pragma unroll
      for (int i = 0; i <= D; ++i) sy[i] = __builtin_fma(shift, su[i], sy[i]);
      // ---- the slices add up: fixed order, the same bits in every lane of the column ----
      for (int off = CL; off < L; off <<= 1) {
#pragma unroll
        for (int i = 0; i <= 2 * D; ++i) su[i] += __shfl_xor(su[i], off);
#pragma unroll
        for (int i = 0; i <= D; ++i) sy[i] += __shfl_xor(sy[i], off);
        n += __shfl_xor(n, off);
        merge_extreme(ymin, off, true);
        merge_extreme(ymax, off, false);
        merge_extreme(xlo, off, true);
        merge_extreme(xhi, off, false);
      }
      // ---- solve (every lane, the same registers) ----
      double c[D + 1];
#pragma unroll
      for (int i = 0; i <= D; ++i) c[i] = 0.0;
      const bool fitted = n >= D + 1 && solve_normal<D>(su, sy, c);
      // ---- second walk: the residuals about the fitted shape ----
      double ss = 0.0, worst = 0.0;
      if (live && fitted) {
#pragma unroll 4
        for (long long s = sl; s < S; s += SL) {
          const double* row = vp + s * a.ld;
          const double y = row[k];
          const double x = a.abscissa ? a.abscissa[s] : row[a.x_column];
          const unsigned st = OKX_ENS_STATUS_AT(sp, s, a.status_stride);
          if (!(OKX_ENS_ACCEPTED(st, y) && __builtin_isfinite(x) && x >= a.lo && x <= a.hi)) continue;
          const double u = (x - a.origin) * a.inv_scale;
          double q = c[D];
#pragma unroll
          for (int i = D - 1; i >= 0; --i) q = __builtin_fma(q, u, c[i]);
          const double r = (y - yref) - q;
          ss = __builtin_fma(r, r, ss);
          const double m = __builtin_fabs(r);
          worst = m > worst ? m : worst;
        }
      }
      for (int off = CL; off < L; off <<= 1) {
        ss += __shfl_xor(ss, off);
        const double ow = __shfl_xor(worst, off);
        worst = ow > worst ? ow : worst;
      }
      if (live && sl == 0) {
        double* f = a.features + (g * K + k) * OKX_CURVE_FIELDS;
        a.count[g * K + k] = n;
        if (n == 0) {
#pragma unroll
          for (int i = 0; i < OKX_CURVE_FIELDS; ++i) f[i] = nan;
        } else {
          double scale_i = 1.0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            double ci = 0.0;
            if (i <= D) ci = i == 0 ? c[0] + yref : c[i <= D ? i : 0] / scale_i;
            f[i] = fitted ? ci : nan;
            scale_i = scale_i * a.scale;
          }
          f[4] = fitted ? sqrt(ss / (double)n) : nan;
          f[5] = fitted ? worst : nan;
          f[6] = ymin.v; f[7] = ymax.v;
          f[8] = ymin.x; f[9] = ymax.x;
          f[10] = xlo.v; f[11] = xhi.v;
        }
      }
    }
  }
}

}  // namespace crv
}  // namespace okx

using okx::fail;
namespace et = okx::enstable;

extern "C" {

int32_t okx_ensemble_curves_check(int64_t steps, int32_t n_columns, int64_t abscissa_len, int32_t x_column, double origin, double scale,
                                  double window_lo, double window_hi, int32_t degree) {
  if (degree < 0 || degree > 3) return fail(OKX_ERR_INVALID, "okx_ensemble_curves: degree %d, 0 to 3 allowed", (int)degree);
  if (!(std::isfinite(scale) && scale > 0.0)) return fail(OKX_ERR_INVALID, "okx_ensemble_curves: scale is %g, not finite and > 0", scale);
  if (std::isnan(origin)) return fail(OKX_ERR_INVALID, "okx_ensemble_curves: origin is NaN");
  if (std::isnan(window_lo) || std::isnan(window_hi)) return fail(OKX_ERR_INVALID, "okx_ensemble_curves: window is NaN (an open side is -inf / +inf)");
  if (window_lo > window_hi) return fail(OKX_ERR_INVALID, "okx_ensemble_curves: window has lo > hi (%g > %g)", window_lo, window_hi);
  if (abscissa_len < 0) {
    if (x_column < 0 || x_column >= n_columns)
      return fail(OKX_ERR_INVALID, "okx_ensemble_curves: abscissa column %d, outside [0, %d)", (int)x_column, (int)n_columns);
  } else if (abscissa_len != steps) {
    return fail(OKX_ERR_INVALID, "okx_ensemble_curves: shared abscissa of %lld values, %lld steps", (long long)abscissa_len, (long long)steps);
  }
  return OKX_OK;
}

int32_t okx_ensemble_curves(int64_t n_geometries, int64_t steps, int32_t n_columns, const double* d_values, int64_t ld, const uint8_t* d_status,
                            int64_t status_stride, const double* d_abscissa, int32_t x_column, double origin, double scale, double window_lo,
                            double window_hi, int32_t degree, double* d_features, int32_t* d_count, void* stream) {
  namespace cv = okx::crv;
  if (int rc = et::check_counts("okx_ensemble_curves", n_geometries, steps, n_columns)) return rc;
  if (steps > 0x7fffffffll - 64) return fail(OKX_ERR_LIMIT, "okx_ensemble_curves: too many steps for one call");
  if (n_geometries == 0) return OKX_OK;  // (nothing to validate against: the call does nothing)
  if (int rc = okx_ensemble_curves_check(steps, n_columns, d_abscissa ? steps : -1, x_column, origin, scale, window_lo, window_hi, degree)) return rc;
  if (n_columns == 0) return OKX_OK;
  if (!d_features || !d_count) return fail(OKX_ERR_INVALID, "okx_ensemble_curves: null feature or count table");
  if (int rc = et::check_table("okx_ensemble_curves", steps > 0, d_values, ld, n_columns, d_status, status_stride)) return rc;
  const cv::Plan plan = cv::plan_for(steps, n_columns);
  const long long pack = 64 / (plan.col_lanes * plan.slices);
  const long long tasks = (n_geometries + pack - 1) / pack;
  long long groups = (tasks + cv::kWaves - 1) / cv::kWaves;
  if (groups > cv::kMaxGroups) groups = cv::kMaxGroups;
  cv::Args a{};
  et::set_table(&a, et::table_view(d_values, ld, d_status, status_stride, n_geometries, steps, n_columns));
  a.abscissa = d_abscissa; a.features = d_features; a.count = d_count;
  a.origin = origin; a.scale = scale; a.inv_scale = 1.0 / scale; a.lo = window_lo; a.hi = window_hi;
  a.x_column = d_abscissa ? 0 : x_column; a.col_lanes = plan.col_lanes; a.slices = plan.slices;
  a.col_shift = 0;
  while ((1 << a.col_shift) < plan.col_lanes) ++a.col_shift;
  const dim3 grid((unsigned)groups), block(cv::kThreads);
  hipStream_t st = (hipStream_t)stream;
  switch (degree) {
    case 0: OKX_LAUNCH(cv::okx_curves_fit<0>, grid, block, 0, st, a); break;
    case 1: OKX_LAUNCH(cv::okx_curves_fit<1>, grid, block, 0, st, a); break;
    case 2: OKX_LAUNCH(cv::okx_curves_fit<2>, grid, block, 0, st, a); break;
    default: OKX_LAUNCH(cv::okx_curves_fit<3>, grid, block, 0, st, a); break;
  }
  return OKX_OK;
}

}  // extern "C"
