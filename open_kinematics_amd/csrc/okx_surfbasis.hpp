// okx_surfbasis.hpp — what the two units that form basis values of a response surface share (okx_surface.hip: okx_surf_basis writes them to
// a table; okx_predict.hip: okx_pred_tile forms them into LDS): psi, so that both give the bits of ensemble_stats.basis_host.  Unlike
// okx_enstable.hpp this header DOES floating-point arithmetic, so it sets the contraction itself: both units have it off for all of their
// text, and the pragma below holds from here to the end of the unit that includes it.
#pragma once

#include "../../include/okx.h"

#pragma clang fp contract(off)

#if defined(__HIPCC__)

namespace okx {
namespace surf {

// psi_degree of u by the factor's kind; every operation rounded (ensemble_stats._surface_psi)
__device__ inline double psi(int kind, int degree, double u) {
  if (degree == 0) return 1.0;
  const double uu = u * u;
  if (kind == OKX_SURFACE_HERMITE) {
    if (degree == 1) return u;
    if (degree == 2) return (uu - 1.0) * 0.7071067811865476;
    return ((uu - 3.0) * u) * 0.408248290463863;
  }
  if (kind == OKX_SURFACE_LEGENDRE) {
    if (degree == 1) return u * 1.7320508075688772;
    if (degree == 2) return (3.0 * uu - 1.0) * 1.118033988749895;
    return ((5.0 * uu - 3.0) * u) * 1.3228756555322954;
  }
  if (degree == 1) return u;
  if (degree == 2) return uu;
  return uu * u;
}

}  // namespace surf
}  // namespace okx

#endif  // __HIPCC__
