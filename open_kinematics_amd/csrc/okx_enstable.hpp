// okx_enstable.hpp — the argument checks the ensemble passes share (okx_ensemble.hip, okx_select.hip, okx_screen.hip,
// okx_covariance.hip), each with the calling entry point's name for the message; a pass calls them where the order of its
// own checks wants them.
#pragma once

#include <cmath>

#include "okx_program.hpp"

namespace okx {
namespace enstable {

inline int check_counts(const char* who, long long n_geom, long long steps, int n_columns) {
  if (n_geom < 0 || steps < 0 || n_columns < 0) return fail(OKX_ERR_INVALID, "%s: negative geometry, step or column count", who);
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

}  // namespace enstable
}  // namespace okx
