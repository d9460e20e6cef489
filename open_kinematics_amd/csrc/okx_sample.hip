// Ensemble sampler (okx_ensemble_sample*, include/okx.h): the hardpoint table [n][P][3] of a perturbed-geometry ensemble drawn
// on device by a COUNTER-BASED generator - geometry g's draw is a pure function of (seed, g, latent index, attempt), so any
// chunk, device or rank writes the same bits for the rows it owns.  The definition is open_kinematics_amd/ensemble_sample.py
// (NumPy); this file equals it bit for bit: integer arithmetic, and fp64 add, multiply, divide and sqrt each rounded on its
// own (contraction is off for the whole unit, divide and sqrt go through the _rn intrinsics, no libm call - the tail's
// logarithm of the inverse normal CDF is written out).
//
// One launch (okx_sample_draw), ONE WAVEFRONT = ONE WORKGROUP PER GEOMETRY:
//  - the redraw loop is per geometry, so it is uniform over the wavefront: no lane waits for another geometry's attempts;
//  - lanes run along the latents (one Philox4x32-10 call and one inverse CDF each), then along the perturbed coordinates
//    (the contraction with `mixing` reads the wavefront's latents from LDS - identical addresses broadcast - so a latent is
//    drawn once, not once per coordinate), then along the flat [P * 3] row: the stores of a row are contiguous 8-byte lanes;
//  - the row, the latents and the deltas of the current attempt live in LDS (3 x 288 doubles + 288 strata words, 8064 bytes);
//    the guards (at most 16, kernel arguments) are evaluated by every lane from LDS, which keeps the verdict uniform without
//    a vote;
//  - under LHS the stratum pi_z(g) - a four-round Feistel network walked into [0, n_total) - is computed once per latent
//    before the first attempt; a redraw only moves the draw inside its stratum.
// A workgroup of one wavefront makes the barriers between the phases cheap.  Device tables are indexed defensively: a
// coordinate index outside the row is skipped, never written.
// okx_sample_draw_families (okx_ensemble_sample_families) is the same mapping for a pick-freeze ensemble: one attempt, and a
// latent's counter names the source row of its family instead of the geometry (further down, with its own comment).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/okx.h"
#include "okx_philox.hpp"
#include "okx_program.hpp"

#pragma clang fp contract(off)

namespace okx {
namespace smp {

constexpr int kThreads = 64;
constexpr int kMaxF = OKX_ENS_SAMPLE_MAX_COORDS;
constexpr int kMaxZ = OKX_ENS_SAMPLE_MAX_LATENTS;
constexpr int kMaxRow = 3 * OKX_MAX_POINTS;
constexpr int kMaxGuards = OKX_ENS_SAMPLE_MAX_GUARDS;

typedef unsigned int u32;
typedef unsigned long long u64;

// AS241 (PPND16) and the logarithm's series, the doubles of ensemble_sample.py written as hexadecimal literals
__constant__ const double kA[8] = {0x1.b18d91e9eef75p+1, 0x1.0a4888b1a436ep+7, 0x1.ece5d2213c0ccp+10, 0x1.ad1d8cd4ee71dp+13,
                                   0x1.66c3e869b752ap+15, 0x1.06c1c55b78f20p+16, 0x1.052d26b2e45e4p+15, 0x1.39a296f7d925ep+11};
__constant__ const double kB[8] = {0x1.0000000000000p+0, 0x1.5281b386e1ab5p+5, 0x1.5797efdc8b3f7p+9, 0x1.512322e75c89fp+12,
                                   0x1.4b772d5d65266p+14, 0x1.3317caa64f4bep+15, 0x1.c0e457cb1ae76p+14, 0x1.46a7eca984b69p+12};
__constant__ const double kC[8] = {0x1.6c665fde9526ap+0, 0x1.2857748cab19bp+2, 0x1.713f71462256ap+2, 0x1.d2ecb1a3d02c4p+1,
                                   0x1.453cc085375b2p+0, 0x1.ef2abb9b85c37p-3, 0x1.744eb6c45ec67p-6, 0x1.9615ac0b7ace9p-11};
__constant__ const double kD[8] = {0x1.0000000000000p+0, 0x1.06cefbb46a449p+1, 0x1.ad278e6526633p+0, 0x1.61292f23385c9p-1,
                                   0x1.2f5123394f040p-3, 0x1.f207a7eab17bfp-7, 0x1.1f18cbfdf2728p-11, 0x1.20d3f686439e4p-30};
__constant__ const double kE[8] = {0x1.aa1b1c13ee526p+2, 0x1.5daea6e875003p+2, 0x1.c8ea6461fa445p+0, 0x1.2fad9315255cfp-2,
                                   0x1.b2b41193b4ee7p-6, 0x1.45c1908425345p-10, 0x1.c6ec6cc59e02ap-16, 0x1.afb74d693bf93p-23};
__constant__ const double kF[8] = {0x1.0000000000000p+0, 0x1.331d34fc7d77fp-1, 0x1.186eb183443fbp-3, 0x1.e76f93215462ap-7,
                                   0x1.9c8bc979dc5d7p-11, 0x1.35c2c496374bfp-16, 0x1.31446f740b9e0p-23, 0x1.269bff1f8c190p-49};
__constant__ const double kLog[11] = {0x1.0000000000000p+0, 0x1.5555555555555p-2, 0x1.999999999999ap-3, 0x1.2492492492492p-3,
                                      0x1.c71c71c71c71cp-4, 0x1.745d1745d1746p-4, 0x1.3b13b13b13b14p-4, 0x1.1111111111111p-4,
                                      0x1.e1e1e1e1e1e1ep-5, 0x1.af286bca1af28p-5, 0x1.8618618618618p-5};
constexpr double kLn2 = 0x1.62e42fefa39efp-1;
constexpr double kSqrtHalf = 0x1.6a09e667f3bcdp-1;
constexpr double kSplit1 = 0x1.b333333333333p-2;  // 0.425
constexpr double kConst1 = 0x1.71eb851eb851fp-3;  // 0.180625
constexpr double kConst2 = 0x1.999999999999ap+0;  // 1.6
constexpr double kSplit2 = 5.0;
constexpr double kUMin = 0x1.0000000000000p-53;
constexpr double kUMax = 0x1.fffffffffffffp-1;

struct Guards {
  okx_sample_guard g[kMaxGuards];
  int n;
};

struct Args {
  const double* nominal;  // [p3]
  const int* coords;      // [f]
  const int* kind;        // [z]
  const double* bound;    // [z][3]: k, Phi(-k), Phi(k) - Phi(-k)
  const double* mixing;   // [f][z] or null
  const double* scale;    // [f] (no mixing)
  double* hardpoints;     // [n][p3]
  double* latents;        // [n][z] or null
  double* delta;          // [n][f] or null
  unsigned char* flags;   // [n] or null
  u64 offset, n_total;
  double n_total_f;
  u32 key0, key1;
  int p3, f, z, lhs, max_attempts, half_bits;
  Guards guards;
};

using rng::philox4x32_10;  // (okx_philox.hpp: the bootstrap draws from it too)

__device__ inline u32 mix32(u32 x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  return x ^ (x >> 16);
}

// pi_z(g): the stratum of geometry g (< n_total) under the four round keys of latent z
__device__ inline u32 stratum(u64 g, u64 n_total, int half_bits, const u32* keys) {
  const u32 mask = (1u << half_bits) - 1u;  // half_bits <= 16
  u64 x = g;
  do {
    u32 left = (u32)(x >> half_bits), right = (u32)x & mask;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const u32 next = left ^ (mix32(right + keys[r]) & mask);
      left = right;
      right = next;
    }
    x = ((u64)left << half_bits) | right;
  } while (x >= n_total);  // (a bijection of [0, 2^b) with g inside [0, n_total): the walk returns there)
  return (u32)x;
}

template <int N>
__device__ inline double horner(const double* k, double r) {
  double acc = k[N - 1];
#pragma unroll
  for (int i = N - 2; i >= 0; --i) acc = acc * r + k[i];
  return acc;
}

// log(x) of a normal positive double: x = m 2^e, m in [sqrt(1/2), sqrt(2)), log x = e ln2 + 2 s P(s^2), s = (m - 1) / (m + 1)
__device__ inline double log_unit(double x) {
  const long long bits = __double_as_longlong(x);
  int e = (int)((bits >> 52) & 0x7FF) - 1022;
  double m = __longlong_as_double((bits & 0x800FFFFFFFFFFFFFll) | 0x3FE0000000000000ll);  // [0.5, 1)
  if (m < kSqrtHalf) {
    m = m * 2.0;
    e -= 1;
  }
  const double s = __ddiv_rn(m - 1.0, m + 1.0);
  return (double)e * kLn2 + (2.0 * s) * horner<11>(kLog, s * s);
}

__device__ inline double ppnd16(double u) {
  const double q = u - 0.5;
  if (__builtin_fabs(q) <= kSplit1) {
    const double r = kConst1 - q * q;
    return __ddiv_rn(q * horner<8>(kA, r), horner<8>(kB, r));
  }
  const double tail = q < 0.0 ? u : 1.0 - u;
  const double r = __dsqrt_rn(-log_unit(tail));
  double v;
  if (r <= kSplit2) {
    const double r1 = r - kConst2;
    v = __ddiv_rn(horner<8>(kC, r1), horner<8>(kD, r1));
  } else {
    const double r2 = r - kSplit2;
    v = __ddiv_rn(horner<8>(kE, r2), horner<8>(kF, r2));
  }
  return q < 0.0 ? -v : v;
}

__device__ inline double clamp(double x, double lo, double hi) {  // min(max(x, lo), hi) as NumPy takes them (no NaN here)
  x = x < lo ? lo : x;
  return x > hi ? hi : x;
}

__device__ inline double norm3(double x, double y, double z) { return __dsqrt_rn((x * x + y * y) + z * z); }

// every guard holds for the row in LDS (the same answer in every lane)
__device__ inline bool guards_hold(const Guards& gs, const double* row) {
  bool ok = true;
  for (int i = 0; i < gs.n; ++i) {
    const okx_sample_guard gd = gs.g[i];
    if (gd.kind == OKX_SAMPLE_GUARD_SIGN) {
      ok = ok && (gd.sign * row[gd.a] > gd.eps);
      continue;
    }
    const double* a = row + 3 * gd.a;
    const double* b = row + 3 * gd.b;
    const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    const double span = norm3(dx, dy, dz);
    if (gd.kind == OKX_SAMPLE_GUARD_DISTINCT) {
      ok = ok && (span > gd.eps);
      continue;
    }
    const double* c = row + 3 * gd.c;
    const double tx = __ddiv_rn(dx, span), ty = __ddiv_rn(dy, span), tz = __ddiv_rn(dz, span);
    const double wx = c[0] - a[0], wy = c[1] - a[1], wz = c[2] - a[2];
    const double off = norm3(wy * tz - wz * ty, wz * tx - wx * tz, wx * ty - wy * tx);
    ok = ok && (span > gd.eps) && (off > gd.eps);
  }
  return ok;
}

__global__ __launch_bounds__(kThreads) void okx_sample_draw(Args a) {
  __shared__ double row[kMaxRow];
  __shared__ double lat[kMaxZ];
  __shared__ double dlt[kMaxF];
  __shared__ u32 strata[kMaxZ];
  const int lane = threadIdx.x;
  const u64 local = blockIdx.x;
  const u64 g = a.offset + local;
  const u32 g_lo = (u32)g, g_hi = (u32)(g >> 32);
  if (a.lhs) {
    for (int z = lane; z < a.z; z += kThreads) {
      u32 keys[4];
      philox4x32_10(0u, 0u, (u32)z, (u32)OKX_SAMPLE_PURPOSE_STRATA << 8, a.key0, a.key1, keys);
      strata[z] = stratum(g, a.n_total, a.half_bits, keys);
    }
  }
  int attempt = 0;
  bool ok = false;
  for (;;) {
    // the latents of this attempt
    for (int z = lane; z < a.z; z += kThreads) {
      u32 w[4];
      philox4x32_10(g_lo, g_hi, (u32)z, (u32)attempt | ((u32)OKX_SAMPLE_PURPOSE_DRAW << 8), a.key0, a.key1, w);
      const u64 k = ((u64)w[0] << 20) | (u64)(w[1] >> 12);
      double u = ((double)k + 0.5) * 0x1.0p-52;
      if (a.lhs) u = clamp(__ddiv_rn((double)strata[z] + u, a.n_total_f), kUMin, kUMax);
      const int kind = a.kind[z];
      double x;
      if (kind == OKX_SAMPLE_UNIFORM) {
        x = 2.0 * u - 1.0;
      } else if (kind == OKX_SAMPLE_TRUNCATED) {
        const double bound = a.bound[3 * z], below = a.bound[3 * z + 1], width = a.bound[3 * z + 2];
        x = clamp(ppnd16(clamp(below + u * width, kUMin, kUMax)), -bound, bound);
      } else {
        x = ppnd16(u);
      }
      lat[z] = x;
    }
    for (int i = lane; i < a.p3; i += kThreads) row[i] = a.nominal[i];
    __syncthreads();
    // the deltas and the perturbed coordinates
    for (int f = lane; f < a.f; f += kThreads) {
      double d;
      if (a.mixing) {
        const double* m = a.mixing + (size_t)f * a.z;
        d = 0.0;
        for (int z = 0; z < a.z; ++z) d = d + m[z] * lat[z];
      } else {
        d = a.scale[f] * lat[f];
      }
      dlt[f] = d;
      const int c = a.coords[f];
      if ((unsigned)c < (unsigned)a.p3) row[c] = a.nominal[c] + d;  // (distinct coordinates: no two lanes write one slot)
    }
    __syncthreads();
    ok = guards_hold(a.guards, row);
    if (ok || attempt + 1 >= a.max_attempts) break;
    ++attempt;
    __syncthreads();  // (every lane has read the row before the next attempt rewrites it)
  }
  double* out = a.hardpoints + local * (u64)a.p3;
  for (int i = lane; i < a.p3; i += kThreads) out[i] = row[i];
  if (a.latents)
    for (int z = lane; z < a.z; z += kThreads) a.latents[local * (u64)a.z + z] = lat[z];
  if (a.delta)
    for (int f = lane; f < a.f; f += kThreads) a.delta[local * (u64)a.f + f] = dlt[f];
  if (a.flags && lane == 0) a.flags[local] = (unsigned char)((attempt << 4) | (ok ? 0 : 1));
}

inline int half_bits_for(unsigned long long n_total) {
  int b = 2;
  while (b < 64 && (1ull << b) < n_total) b += 2;
  return b / 2;
}

// what okx_ensemble_sample_check reports
inline int check_arguments(const char* who, long long n_geom, long long offset, long long n_total, int n_points, const int32_t* coords, int n_coords,
                           const int32_t* kind, const double* bound, int n_latents, int has_mixing, const okx_sample_guard* guards, int n_guards,
                           int stratify, int max_attempts) {
  if (n_geom < 0 || offset < 0 || n_total < 0) return fail(OKX_ERR_INVALID, "%s: negative n_geometries, geometry_offset or n_total", who);
  if (n_points < 1 || n_points > OKX_MAX_POINTS) return fail(OKX_ERR_INVALID, "%s: %d points, 1 to %d allowed", who, n_points, (int)OKX_MAX_POINTS);
  if (n_coords < 1 || n_coords > kMaxF) return fail(OKX_ERR_INVALID, "%s: %d coordinates, 1 to %d allowed", who, n_coords, kMaxF);
  if (n_latents < 1 || n_latents > kMaxZ) return fail(OKX_ERR_INVALID, "%s: %d latents, 1 to %d allowed", who, n_latents, kMaxZ);
  if (!has_mixing && n_latents != n_coords)
    return fail(OKX_ERR_INVALID, "%s: without mixing every coordinate has its own latent (%d latents, %d coordinates)", who, n_latents, n_coords);
  if (coords) {
    bool seen[kMaxRow] = {};
    for (int i = 0; i < n_coords; ++i) {
      const int c = coords[i];
      if (c < 0 || c >= 3 * n_points) return fail(OKX_ERR_INVALID, "%s: coordinate %d is %d, outside [0, %d)", who, i, c, 3 * n_points);
      if (seen[c]) return fail(OKX_ERR_INVALID, "%s: coordinate %d repeats index %d", who, i, c);
      seen[c] = true;
    }
  }
  if (kind)
    for (int i = 0; i < n_latents; ++i) {
      if (kind[i] < OKX_SAMPLE_NORMAL || kind[i] > OKX_SAMPLE_TRUNCATED)
        return fail(OKX_ERR_INVALID, "%s: kind %d is %d, not 0 (normal), 1 (uniform) or 2 (truncated)", who, i, (int)kind[i]);
      if (kind[i] == OKX_SAMPLE_TRUNCATED && bound && !(std::isfinite(bound[i]) && bound[i] > 0.0))
        return fail(OKX_ERR_INVALID, "%s: bound %d is %g, not finite and greater than 0", who, i, bound[i]);
    }
  if (n_guards < 0 || n_guards > kMaxGuards) return fail(OKX_ERR_INVALID, "%s: %d guards, at most %d", who, n_guards, kMaxGuards);
  if (n_guards > 0 && !guards) return fail(OKX_ERR_INVALID, "%s: null guards", who);
  for (int i = 0; i < n_guards; ++i) {
    const okx_sample_guard& gd = guards[i];
    if (gd.kind < OKX_SAMPLE_GUARD_SIGN || gd.kind > OKX_SAMPLE_GUARD_OFF_LINE)
      return fail(OKX_ERR_INVALID, "%s: guard %d has kind %d, not 0 (sign), 1 (distinct) or 2 (off line)", who, i, (int)gd.kind);
    const int limit = gd.kind == OKX_SAMPLE_GUARD_SIGN ? 3 * n_points : n_points;
    const int used = gd.kind == OKX_SAMPLE_GUARD_SIGN ? 1 : gd.kind == OKX_SAMPLE_GUARD_DISTINCT ? 2 : 3;
    const int32_t index[3] = {gd.a, gd.b, gd.c};
    for (int j = 0; j < used; ++j)
      if (index[j] < 0 || index[j] >= limit) return fail(OKX_ERR_INVALID, "%s: guard %d names an index outside [0, %d)", who, i, limit);
    if (!std::isfinite(gd.eps) || (gd.kind == OKX_SAMPLE_GUARD_SIGN && gd.sign != 1.0 && gd.sign != -1.0))
      return fail(OKX_ERR_INVALID, "%s: guard %d needs a finite eps (and a sign of +1 or -1)", who, i);
  }
  if (stratify != OKX_SAMPLE_IID && stratify != OKX_SAMPLE_LHS) return fail(OKX_ERR_INVALID, "%s: stratify is %d, not 0 (iid) or 1 (lhs)", who, stratify);
  if (max_attempts < 1 || max_attempts > OKX_ENS_SAMPLE_MAX_ATTEMPTS)
    return fail(OKX_ERR_INVALID, "%s: max_attempts is %d, 1 to %d allowed", who, max_attempts, (int)OKX_ENS_SAMPLE_MAX_ATTEMPTS);
  if (stratify == OKX_SAMPLE_LHS) {
    if (n_total > (1ll << 32)) return fail(OKX_ERR_INVALID, "%s: %lld strata, at most 2^32 under LHS", who, n_total);
    if (offset + n_geom > n_total)
      return fail(OKX_ERR_INVALID, "%s: geometries [%lld, %lld) lie outside the %lld strata", who, offset, offset + n_geom, n_total);
  }
  return OKX_OK;
}

// ---- the pick-freeze draw (okx_ensemble_sample_families): families of M = n_groups + 2 geometries, interleaved ----
//
// Geometry g is member b = g % M of family i = g / M.  Member 0 is A, member 1 is B, member 2 + j is A with the latents of
// group j taken from B: latent z of g is the draw of SOURCE ROW src = 2 i + s at attempt 0, s = 1 for B and for a latent of
// the member's own group, else 0 - one counter word differs from okx_sample_draw.  Under LHS the stratum is pi_z(src) over
// the 2 n_families source rows.  One attempt: a redraw of one member would break the coordinates it shares with the others.
struct FamilyArgs {
  Args a;            // n_total = 2 n_families (the source rows), max_attempts unused
  const int* group;  // [z]: the latent's group in [0, n_groups), -1: never swapped
  u64 members;       // M
};

__global__ __launch_bounds__(kThreads) void okx_sample_draw_families(FamilyArgs fa) {
  __shared__ double row[kMaxRow];
  __shared__ double lat[kMaxZ];
  __shared__ double dlt[kMaxF];
  const Args& a = fa.a;
  const int lane = threadIdx.x;
  const u64 local = blockIdx.x;
  const u64 g = a.offset + local;
  const u64 family = g / fa.members;
  const int member = (int)(g - family * fa.members);
  for (int z = lane; z < a.z; z += kThreads) {
    const int gr = fa.group[z];
    const bool from_b = member == 1 || (member >= 2 && gr == member - 2);
    const u64 src = 2ull * family + (from_b ? 1ull : 0ull);
    u32 w[4];
    philox4x32_10((u32)src, (u32)(src >> 32), (u32)z, (u32)OKX_SAMPLE_PURPOSE_DRAW << 8, a.key0, a.key1, w);
    const u64 k = ((u64)w[0] << 20) | (u64)(w[1] >> 12);
    double u = ((double)k + 0.5) * 0x1.0p-52;
    if (a.lhs) {  // (src < n_total: the entry point checked the range, so the walk returns)
      u32 keys[4];
      philox4x32_10(0u, 0u, (u32)z, (u32)OKX_SAMPLE_PURPOSE_STRATA << 8, a.key0, a.key1, keys);
      u = clamp(__ddiv_rn((double)stratum(src, a.n_total, a.half_bits, keys) + u, a.n_total_f), kUMin, kUMax);
    }
    const int kind = a.kind[z];
    double x;
    if (kind == OKX_SAMPLE_UNIFORM) {
      x = 2.0 * u - 1.0;
    } else if (kind == OKX_SAMPLE_TRUNCATED) {
      const double bound = a.bound[3 * z], below = a.bound[3 * z + 1], width = a.bound[3 * z + 2];
      x = clamp(ppnd16(clamp(below + u * width, kUMin, kUMax)), -bound, bound);
    } else {
      x = ppnd16(u);
    }
    lat[z] = x;
  }
  for (int i = lane; i < a.p3; i += kThreads) row[i] = a.nominal[i];
  __syncthreads();
  for (int f = lane; f < a.f; f += kThreads) {
    double d;
    if (a.mixing) {
      const double* m = a.mixing + (size_t)f * a.z;
      d = 0.0;
      for (int z = 0; z < a.z; ++z) d = d + m[z] * lat[z];
    } else {
      d = a.scale[f] * lat[f];
    }
    dlt[f] = d;
    const int c = a.coords[f];
    if ((unsigned)c < (unsigned)a.p3) row[c] = a.nominal[c] + d;
  }
  __syncthreads();
  const bool ok = guards_hold(a.guards, row);
  double* out = a.hardpoints + local * (u64)a.p3;
  for (int i = lane; i < a.p3; i += kThreads) out[i] = row[i];
  if (a.latents)
    for (int z = lane; z < a.z; z += kThreads) a.latents[local * (u64)a.z + z] = lat[z];
  if (a.delta)
    for (int f = lane; f < a.f; f += kThreads) a.delta[local * (u64)a.f + f] = dlt[f];
  if (a.flags && lane == 0) a.flags[local] = (unsigned char)(ok ? 0 : 1);
}

// what okx_ensemble_sample_families_check reports: the plan's own checks, then the families'
inline int check_families(const char* who, long long n_geom, long long offset, long long n_families, int n_points, const int32_t* coords, int n_coords,
                          const int32_t* kind, const double* bound, int n_latents, int has_mixing, const int32_t* group, int n_groups,
                          const okx_sample_guard* guards, int n_guards, int stratify, int max_attempts) {
  if (n_geom < 0 || offset < 0 || n_families < 0) return fail(OKX_ERR_INVALID, "%s: negative n_geometries, geometry_offset or n_families", who);
  if (n_groups < 1 || n_groups > OKX_ENS_SOBOL_MAX_GROUPS)
    return fail(OKX_ERR_INVALID, "%s: %d groups, 1 to %d allowed", who, n_groups, (int)OKX_ENS_SOBOL_MAX_GROUPS);
  if (max_attempts != 1)
    return fail(OKX_ERR_INVALID, "%s: max_attempts is %d; a family is drawn once (a redraw of one member would break the frozen coordinates)", who,
                max_attempts);
  if (n_families > (1ll << 52)) return fail(OKX_ERR_INVALID, "%s: %lld families, at most 2^52", who, n_families);
  if (int rc = check_arguments(who, 0, 0, 2 * n_families, n_points, coords, n_coords, kind, bound, n_latents, has_mixing, guards, n_guards, stratify, 1))
    return rc;
  if (group) {
    bool seen[OKX_ENS_SOBOL_MAX_GROUPS] = {};
    for (int z = 0; z < n_latents; ++z) {
      if (group[z] < -1 || group[z] >= n_groups)
        return fail(OKX_ERR_INVALID, "%s: group %d is %d, outside [-1, %d)", who, z, (int)group[z], n_groups);
      if (group[z] >= 0) seen[group[z]] = true;
    }
    for (int j = 0; j < n_groups; ++j)
      if (!seen[j]) return fail(OKX_ERR_INVALID, "%s: group %d has no latent", who, j);
  }
  const long long members = n_groups + 2;
  if (stratify == OKX_SAMPLE_LHS && (offset + n_geom + members - 1) / members > n_families)
    return fail(OKX_ERR_INVALID, "%s: geometries [%lld, %lld) lie outside the %lld families of %lld", who, offset, offset + n_geom, n_families, members);
  return OKX_OK;
}

}  // namespace smp
}  // namespace okx

using okx::fail;

extern "C" {

int32_t okx_ensemble_sample_check(int64_t n_geometries, int64_t geometry_offset, int64_t n_total, int32_t n_points, const int32_t* coords,
                                  int32_t n_coords, const int32_t* kind, const double* bound, int32_t n_latents, int32_t has_mixing,
                                  const okx_sample_guard* guards, int32_t n_guards, int32_t stratify, int32_t max_attempts) {
  return okx::smp::check_arguments("okx_ensemble_sample", n_geometries, geometry_offset, n_total, n_points, coords, n_coords, kind, bound, n_latents,
                                   has_mixing, guards, n_guards, stratify, max_attempts);
}

int32_t okx_ensemble_sample(int64_t n_geometries, int64_t geometry_offset, int64_t n_total, uint64_t seed, int32_t n_points, const double* d_nominal,
                            const int32_t* d_coords, int32_t n_coords, const int32_t* d_kind, const double* d_bound, int32_t n_latents,
                            const double* d_mixing, const double* d_scale, const okx_sample_guard* guards, int32_t n_guards, int32_t stratify,
                            int32_t max_attempts, double* d_hardpoints, double* d_latents, double* d_delta, uint8_t* d_flags, void* stream) {
  namespace sm = okx::smp;
  const char* who = "okx_ensemble_sample";
  // (the device tables cannot be read here: okx_ensemble_sample_check takes their host copies; the kernel skips a
  //  coordinate outside the row and treats an unknown kind as normal)
  if (int rc = sm::check_arguments(who, n_geometries, geometry_offset, n_total, n_points, nullptr, n_coords, nullptr, nullptr, n_latents,
                                   d_mixing != nullptr, guards, n_guards, stratify, max_attempts))
    return rc;
  if (n_geometries > 0x7FFFFFFFll) return fail(OKX_ERR_INVALID, "%s: %lld geometries, at most 2^31 - 1 in one call", who, (long long)n_geometries);
  if (!d_nominal || !d_coords || !d_kind || !d_bound) return fail(OKX_ERR_INVALID, "%s: null nominal, coords, kind or bound table", who);
  if (!d_mixing && !d_scale) return fail(OKX_ERR_INVALID, "%s: neither mixing nor scale", who);
  if (n_geometries == 0) return OKX_OK;
  if (!d_hardpoints) return fail(OKX_ERR_INVALID, "%s: null hardpoint table", who);
  sm::Args a{};
  a.nominal = d_nominal; a.coords = d_coords; a.kind = d_kind; a.bound = d_bound; a.mixing = d_mixing; a.scale = d_scale;
  a.hardpoints = d_hardpoints; a.latents = d_latents; a.delta = d_delta; a.flags = d_flags;
  a.offset = (unsigned long long)geometry_offset; a.n_total = (unsigned long long)n_total; a.n_total_f = (double)n_total;
  a.key0 = (unsigned)(seed & 0xFFFFFFFFull); a.key1 = (unsigned)(seed >> 32);
  a.p3 = 3 * n_points; a.f = n_coords; a.z = n_latents; a.lhs = stratify == OKX_SAMPLE_LHS ? 1 : 0; a.max_attempts = max_attempts;
  a.half_bits = sm::half_bits_for(a.n_total);
  a.guards.n = n_guards;
  for (int i = 0; i < n_guards; ++i) a.guards.g[i] = guards[i];
  hipLaunchKernelGGL(sm::okx_sample_draw, dim3((unsigned)n_geometries), dim3(sm::kThreads), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return OKX_OK;
}

int32_t okx_ensemble_sample_families_check(int64_t n_geometries, int64_t geometry_offset, int64_t n_families, int32_t n_points, const int32_t* coords,
                                           int32_t n_coords, const int32_t* kind, const double* bound, int32_t n_latents, int32_t has_mixing,
                                           const int32_t* group, int32_t n_groups, const okx_sample_guard* guards, int32_t n_guards, int32_t stratify,
                                           int32_t max_attempts) {
  return okx::smp::check_families("okx_ensemble_sample_families", n_geometries, geometry_offset, n_families, n_points, coords, n_coords, kind, bound,
                                  n_latents, has_mixing, group, n_groups, guards, n_guards, stratify, max_attempts);
}

int32_t okx_ensemble_sample_families(int64_t n_geometries, int64_t geometry_offset, int64_t n_families, uint64_t seed, int32_t n_points,
                                     const double* d_nominal, const int32_t* d_coords, int32_t n_coords, const int32_t* d_kind, const double* d_bound,
                                     int32_t n_latents, const double* d_mixing, const double* d_scale, const int32_t* d_group, int32_t n_groups,
                                     const okx_sample_guard* guards, int32_t n_guards, int32_t stratify, double* d_hardpoints, double* d_latents,
                                     double* d_delta, uint8_t* d_flags, void* stream) {
  namespace sm = okx::smp;
  const char* who = "okx_ensemble_sample_families";
  // (the device tables cannot be read here: okx_ensemble_sample_families_check takes their host copies; the kernel compares a
  //  latent's group with the member's and never indexes by it)
  if (int rc = sm::check_families(who, n_geometries, geometry_offset, n_families, n_points, nullptr, n_coords, nullptr, nullptr, n_latents,
                                  d_mixing != nullptr, nullptr, n_groups, guards, n_guards, stratify, 1))
    return rc;
  if (n_geometries > 0x7FFFFFFFll) return fail(OKX_ERR_INVALID, "%s: %lld geometries, at most 2^31 - 1 in one call", who, (long long)n_geometries);
  if (!d_nominal || !d_coords || !d_kind || !d_bound || !d_group) return fail(OKX_ERR_INVALID, "%s: null nominal, coords, kind, bound or group table", who);
  if (!d_mixing && !d_scale) return fail(OKX_ERR_INVALID, "%s: neither mixing nor scale", who);
  if (n_geometries == 0) return OKX_OK;
  if (!d_hardpoints) return fail(OKX_ERR_INVALID, "%s: null hardpoint table", who);
  sm::FamilyArgs fa{};
  sm::Args& a = fa.a;
  a.nominal = d_nominal; a.coords = d_coords; a.kind = d_kind; a.bound = d_bound; a.mixing = d_mixing; a.scale = d_scale;
  a.hardpoints = d_hardpoints; a.latents = d_latents; a.delta = d_delta; a.flags = d_flags;
  a.offset = (unsigned long long)geometry_offset; a.n_total = 2ull * (unsigned long long)n_families; a.n_total_f = (double)a.n_total;
  a.key0 = (unsigned)(seed & 0xFFFFFFFFull); a.key1 = (unsigned)(seed >> 32);
  a.p3 = 3 * n_points; a.f = n_coords; a.z = n_latents; a.lhs = stratify == OKX_SAMPLE_LHS ? 1 : 0; a.max_attempts = 1;
  a.half_bits = sm::half_bits_for(a.n_total);
  a.guards.n = n_guards;
  for (int i = 0; i < n_guards; ++i) a.guards.g[i] = guards[i];
  fa.group = d_group;
  fa.members = (unsigned long long)n_groups + 2ull;
  hipLaunchKernelGGL(sm::okx_sample_draw_families, dim3((unsigned)n_geometries), dim3(sm::kThreads), 0, (hipStream_t)stream, fa);
  HIP_TRY(hipGetLastError());
  return OKX_OK;
}

}  // extern "C"
