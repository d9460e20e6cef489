// Tolerance what-ifs by likelihood reweighting (okx_ensemble_tilt_weights, okx_ensemble_reweigh, include/okx.h): the law of some
// latents changes from p to q, every geometry of the ensemble that is ALREADY evaluated gets the likelihood ratio w = q(z) / p(z)
// of the latents the sampler kept, and every what-if statistic is a weighted sum over the table - no further draw, no further solve.
//
// The WEIGHTS pass (okx_tilt_weights) is one thread per (geometry, scenario), the scenario fastest: the latents of a geometry are
// read by all its scenarios' lanes at once, the five doubles of a (scenario, latent) come from the small scenario table (cache), the
// weights of a geometry are stored side by side.  logw is one chain of rounded operations over the latents in ascending order and
// exp_unit is + - *, rint and ldexp alone: the bits of ensemble_sample.tilt_weights_host.
//
// The REWEIGH pass has the shape of okx_sobol_boot_partial (okx_bootstrap.hip): a lane owns one of 64 entries, a wavefront
// (= workgroup) walks the geometries of a slab, and the scenarios are tiled by ST = 8 so that the 10 ST sums of a lane (160 VGPRs)
// stay in registers at two wavefronts per SIMD.  The weights of the tile for a geometry are ST consecutive doubles at an address that
// is uniform over the wavefront (one scalar load), a scenario whose weight is 0 for the geometry is skipped by a uniform branch
// (adding +-0 to a sum that started at +0 changes no bit), and the next geometry's row, bytes and weights are loaded before this
// geometry's arithmetic.  blockIdx.x runs over (entry tile, scenario tile) with the tiles of one (entry tile, slab) adjacent, so
// workgroups resident together read the same rows from L2: HBM sees the table once, L2 once per scenario tile.  The per-scenario
// sums over geometries (d_joint) have no entry: okx_tilt_joint walks the same slabs with a lane per scenario.  okx_tilt_merge adds
// the slabs in ascending order, after d_acc's / d_joint's own content when the call accumulates.
// The slab plan never looks at the device, there is no floating-point atomic, and contraction is off for the unit: every
// difference and product is rounded on its own as ensemble_stats.reweigh_scenario_terms forms them, then added.  The bits repeat
// from run to run and from device to device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/okx.h"
#include "okx_enstable.hpp"
#include "okx_program.hpp"

#pragma clang fp contract(off)

namespace okx {
namespace tilt {

constexpr int kTile = 64;                // entries per workgroup: one per lane, one wavefront
constexpr int kFields = OKX_REWEIGH_FIELDS;
constexpr int kJoint = OKX_REWEIGH_JOINT_FIELDS;
constexpr int kParams = OKX_TILT_PARAMS;
constexpr int kST = 8;                   // scenarios per scenario tile: their weights are 64 consecutive bytes
constexpr long long kMinSlab = 32;       // geometries (as okx_sobol.hip)
constexpr long long kWantGroups = 2048;  // stage-1 wavefronts aimed at, over all tiles

// ---- the weights ----

constexpr double kLog2e = 1.4426950408889634;
constexpr double kLn2Hi = 0x1.62e42fee00000p-1;  // 0x3fe62e42fee00000: k * kLn2Hi is exact for |k| <= 1100
constexpr double kLn2Lo = 1.9082149292705877e-10;

// ensemble_sample.exp_unit: x < -708 and NaN give 0, x > 708 is taken as 708; 1 / n! are correctly rounded quotients of exact integers
__device__ __forceinline__ double exp_unit(double x) {
  if (!(x >= -708.0)) return 0.0;
  const double xs = x > 708.0 ? 708.0 : x;
  const double k = rint(xs * kLog2e);
  const double r = (xs - k * kLn2Hi) - k * kLn2Lo;
  double p = 1.0 / 6227020800.0;
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 1.0 / 2.0;
  p = p * r + 1.0;
  p = p * r + 1.0;
  return ldexp(p, (int)k);  // |k| <= 1022
}

// one thread per (geometry g, scenario s), s fastest
__global__ __launch_bounds__(256) void okx_tilt_weights(const double* latents, long long ldz, int n_latents, const double* table, int n_scenarios,
                                                        long long n_geom, double* weights, long long ldw) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_geom * n_scenarios) return;
  const long long g = t / n_scenarios;
  const int s = (int)(t % n_scenarios);
  const double* z = latents + g * ldz;
  const double* row = table + (long long)s * n_latents * kParams;
  double logw = 0.0;
  bool inside = true;
  for (int i = 0; i < n_latents; ++i) {
    const double x = z[i];
    const double a = row[0], b = row[1], c = row[2], lo = row[3], hi = row[4];
    row += kParams;
    inside = inside && lo <= x && x <= hi;
    logw = logw + ((c * x + b) * x + a);
  }
  weights[g * ldw + s] = inside ? exp_unit(logw) : 0.0;
}

// ---- the weighted sums ----

inline int scenario_tiles(int n_scenarios) { return (n_scenarios + kST - 1) / kST; }

inline void slab_plan(long long n_geom, long long n_entries, int n_scenarios, long long* n_slabs, long long* slab_len) {
  const long long per = scenario_tiles(n_scenarios);
  enstable::slab_plan(n_geom, n_entries, kTile, (kWantGroups + per - 1) / per, kMinSlab, 65535, n_slabs, slab_len);
}

struct Args {
  const double* values;
  const unsigned char* status;
  const unsigned char* mask;     // [n_geom] or null
  const double* shift;
  const double* weights;         // [n_geom][ldw]
  const double* limits;          // [n_entries][2] or null
  const unsigned char* verdict;  // [n_geom] or null
  double* partial;               // [n_slabs][n_scenarios][kFields][n_entries]
  double* joint_partial;         // [n_slabs][n_scenarios][kJoint]
  long long ld, status_stride;
  long long n_geom, steps;
  long long n_entries, slab_len, ldw;
  int n_columns, n_scenarios;
};

__global__ __launch_bounds__(kTile, 2) void okx_tilt_partial(Args a) {
  const int lane = threadIdx.x;
  const int sts = (a.n_scenarios + kST - 1) / kST;
  const long long tile = blockIdx.x / (unsigned)sts;
  const int s0 = (int)(blockIdx.x % (unsigned)sts) * kST;
  const int ns = a.n_scenarios - s0 < kST ? a.n_scenarios - s0 : kST;  // scenarios of the tile (>= 1)
  const long long e = tile * kTile + lane;
  const bool live = e < a.n_entries;
  const long long er = live ? e : 0;  // a lane past the table walks entry 0 and stores nothing
  const long long slab = blockIdx.y;
  const long long g0 = slab * a.slab_len;
  const long long g1 = g0 + a.slab_len < a.n_geom ? g0 + a.slab_len : a.n_geom;
  const enstable::Table t = OKX_ENS_TABLE_OF(a);
  const double* vp = enstable::entry_values(t, er);
  const unsigned char* sp = enstable::entry_status(t, er);
  const long long v_step = enstable::value_step(t), s_step = enstable::status_step(t);
  const double* wp = a.weights + s0;
  const double sh = a.shift[er];
  const double lim_lo = a.limits ? a.limits[2 * er] : -INFINITY, lim_hi = a.limits ? a.limits[2 * er + 1] : INFINITY;
  double count[kST], sw[kST], sww[kST], swd[kST], swdd[kST], swwd[kST], swwdd[kST], out_lo[kST], out_hi[kST], ww_out[kST];
#pragma unroll
  for (int i = 0; i < kST; ++i) count[i] = sw[i] = sww[i] = swd[i] = swdd[i] = swwd[i] = swwdd[i] = out_lo[i] = out_hi[i] = ww_out[i] = 0.0;
  double vn = 0.0, wn[kST];
  unsigned stn = 1u, mkn = 0u;
#pragma unroll
  for (int i = 0; i < kST; ++i) wn[i] = 0.0;
  if (g0 < g1) {
    vn = vp[g0 * v_step];
    stn = OKX_ENS_STATUS_AT(sp, g0, s_step);
    mkn = a.mask ? a.mask[g0] : 0u;
#pragma unroll
    for (int i = 0; i < kST; ++i) wn[i] = i < ns ? wp[g0 * a.ldw + i] : 0.0;  // (uniform over the wavefront; never beyond the row's n_scenarios)
  }
  for (long long g = g0; g < g1; ++g) {
    const double v = vn;
    const unsigned word = stn | ((mkn & 1u) << 2);  // a masked geometry reads as failed
    double w[kST];
#pragma unroll
    for (int i = 0; i < kST; ++i) w[i] = wn[i];
    if (g + 1 < g1) {  // the next geometry's row, bytes and weights, in flight over this geometry's arithmetic
      vn = vp[(g + 1) * v_step];
      stn = OKX_ENS_STATUS_AT(sp, g + 1, s_step);
      mkn = a.mask ? a.mask[g + 1] : 0u;
#pragma unroll
      for (int i = 0; i < kST; ++i) wn[i] = i < ns ? wp[(g + 1) * a.ldw + i] : 0.0;
    }
    const bool ok = OKX_ENS_ACCEPTED(word, v);
    const double d = ok ? v - sh : 0.0;
    const double one = ok ? 1.0 : 0.0;
    const bool below = ok && v < lim_lo, above = ok && v > lim_hi;
    const bool outside = below || above;
#pragma unroll
    for (int i = 0; i < kST; ++i) {
      if (w[i] != 0.0) {  // (uniform over the wavefront)
        const double wl = ok ? w[i] : 0.0;
        const double wwl = ok ? w[i] * w[i] : 0.0;
        const double wd = wl * d, wwd = wwl * d;
        if (w[i] > 0.0) count[i] += one;
        sw[i] += wl; sww[i] += wwl;
        swd[i] += wd; swdd[i] += wd * d;
        swwd[i] += wwd; swwdd[i] += wwd * d;
        out_lo[i] += below ? wl : 0.0; out_hi[i] += above ? wl : 0.0;
        ww_out[i] += outside ? wwl : 0.0;
      }
    }
  }
  if (!live) return;
  double* out = a.partial + ((slab * a.n_scenarios + s0) * kFields) * a.n_entries + e;
  const long long out_scenario = (long long)kFields * a.n_entries;
#pragma unroll
  for (int i = 0; i < kST; ++i)
    if (i < ns) {
      double* o = out + i * out_scenario;
      o[OKX_REWEIGH_COUNT * a.n_entries] = count[i]; o[OKX_REWEIGH_W * a.n_entries] = sw[i]; o[OKX_REWEIGH_WW * a.n_entries] = sww[i];
      o[OKX_REWEIGH_WD * a.n_entries] = swd[i]; o[OKX_REWEIGH_WDD * a.n_entries] = swdd[i];
      o[OKX_REWEIGH_WWD * a.n_entries] = swwd[i]; o[OKX_REWEIGH_WWDD * a.n_entries] = swwdd[i];
      o[OKX_REWEIGH_OUT_LO * a.n_entries] = out_lo[i]; o[OKX_REWEIGH_OUT_HI * a.n_entries] = out_hi[i];
      o[OKX_REWEIGH_WW_OUT * a.n_entries] = ww_out[i];
    }
}

// one thread per (slab, scenario), the scenario fastest: the per-scenario sums over the slab's geometries whose mask bit is clear
__global__ __launch_bounds__(kTile) void okx_tilt_joint(Args a) {
  const int s = blockIdx.x * kTile + threadIdx.x;
  if (s >= a.n_scenarios) return;
  const long long slab = blockIdx.y;
  const long long g0 = slab * a.slab_len;
  const long long g1 = g0 + a.slab_len < a.n_geom ? g0 + a.slab_len : a.n_geom;
  double seen = 0.0, seen_ww = 0.0, pass = 0.0, pass_ww = 0.0, outside = 0.0, unresolved = 0.0, n = 0.0;
  for (long long g = g0; g < g1; ++g) {
    if (a.mask && (a.mask[g] & 1u)) continue;
    const unsigned flag = a.verdict ? a.verdict[g] : 0u;
    const double w = a.weights[g * a.ldw + s];
    const double ww = w * w;
    n += 1.0;
    seen += w; seen_ww += ww;
    pass += flag == 0u ? w : 0.0; pass_ww += flag == 0u ? ww : 0.0;
    outside += (flag & (unsigned)OKX_SCREEN_OUTSIDE) ? w : 0.0;
    unresolved += (flag & (unsigned)OKX_SCREEN_UNRESOLVED) ? w : 0.0;
  }
  double* o = a.joint_partial + (slab * a.n_scenarios + s) * kJoint;
  o[OKX_REWEIGH_JOINT_SEEN] = seen; o[OKX_REWEIGH_JOINT_SEEN_WW] = seen_ww; o[OKX_REWEIGH_JOINT_PASS] = pass; o[OKX_REWEIGH_JOINT_PASS_WW] = pass_ww;
  o[OKX_REWEIGH_JOINT_OUTSIDE] = outside; o[OKX_REWEIGH_JOINT_UNRESOLVED] = unresolved; o[OKX_REWEIGH_JOINT_GEOMETRIES] = n;
}

// One thread per word of a table laid out as a slab's partial is (`per` words): the slabs in ascending order, after the table's
// own content when the call accumulates; eight slabs' loads in flight, added in the same order (as okx_sobol_merge).
__global__ __launch_bounds__(256) void okx_tilt_merge(const double* partial, long long n_slabs, long long per, int accumulate, double* acc) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= per) return;
  const double* in = partial + t;
  double x = accumulate ? acc[t] : 0.0;
  long long k = 0;
  for (; k + 8 <= n_slabs; k += 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = in[(k + i) * per];
#pragma unroll
    for (int i = 0; i < 8; ++i) x += v[i];
  }
  for (; k < n_slabs; ++k) x += in[k * per];
  acc[t] = x;
}

inline int check_scenarios(const char* who, int n_scenarios) {
  if (n_scenarios < 1 || n_scenarios > OKX_ENS_TILT_MAX_SCENARIOS)
    return fail(OKX_ERR_INVALID, "%s: %d scenarios, 1 to %d allowed", who, n_scenarios, (int)OKX_ENS_TILT_MAX_SCENARIOS);
  return OKX_OK;
}

inline int check_latents(const char* who, int n_latents) {
  if (n_latents < 1 || n_latents > OKX_ENS_SAMPLE_MAX_LATENTS)
    return fail(OKX_ERR_INVALID, "%s: %d latents, 1 to %d allowed", who, n_latents, (int)OKX_ENS_SAMPLE_MAX_LATENTS);
  return OKX_OK;
}

// the scratch buffer: the entries' partials, then the per-scenario partials (each a multiple of 8 bytes)
struct Layout {
  long long n_slabs, slab_len;
  size_t partial_bytes, joint_bytes;
  size_t total() const { return partial_bytes + joint_bytes; }
};

inline Layout layout(long long n_geom, long long n_entries, int n_scenarios) {
  Layout l{};
  slab_plan(n_geom, n_entries, n_scenarios, &l.n_slabs, &l.slab_len);
  l.partial_bytes = sizeof(double) * (size_t)l.n_slabs * (size_t)n_scenarios * (size_t)kFields * (size_t)n_entries;
  l.joint_bytes = sizeof(double) * (size_t)l.n_slabs * (size_t)n_scenarios * (size_t)kJoint;
  return l;
}

}  // namespace tilt
}  // namespace okx

using okx::fail;
namespace et = okx::enstable;

extern "C" {

int32_t okx_ensemble_tilt_check(const double* tilt, int32_t n_scenarios, int32_t n_latents) {
  namespace tl = okx::tilt;
  const char* who = "okx_ensemble_tilt_weights";
  if (int rc = tl::check_scenarios(who, n_scenarios)) return rc;
  if (int rc = tl::check_latents(who, n_latents)) return rc;
  if (!tilt) return fail(OKX_ERR_INVALID, "%s: null scenario table", who);
  for (int s = 0; s < n_scenarios; ++s)
    for (int z = 0; z < n_latents; ++z) {
      const double* p = tilt + ((long long)s * n_latents + z) * tl::kParams;
      if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2]))
        return fail(OKX_ERR_INVALID, "%s: scenario %d, latent %d: a, b or c is not finite", who, s, z);
      if (!(p[3] <= p[4])) return fail(OKX_ERR_INVALID, "%s: scenario %d, latent %d: the window is NaN or has lo > hi", who, s, z);
    }
  return OKX_OK;
}

int32_t okx_ensemble_tilt_weights(int64_t n_geometries, const double* d_latents, int64_t ldz, int32_t n_latents, const double* d_tilt,
                                  int32_t n_scenarios, double* d_weights, int64_t ldw, void* stream) {
  namespace tl = okx::tilt;
  const char* who = "okx_ensemble_tilt_weights";
  if (int rc = et::check_counts(who, n_geometries, 0, 0)) return rc;
  if (int rc = tl::check_scenarios(who, n_scenarios)) return rc;
  if (int rc = tl::check_latents(who, n_latents)) return rc;
  if (n_geometries > (1ll << 38) / n_scenarios) return fail(OKX_ERR_LIMIT, "%s: too many geometries for one call", who);
  if (n_geometries == 0) return OKX_OK;
  if (!d_latents || ldz < n_latents) return fail(OKX_ERR_INVALID, "%s: null latent table or ldz < n_latents", who);
  if (!d_tilt) return fail(OKX_ERR_INVALID, "%s: null scenario table", who);
  if (!d_weights || ldw < n_scenarios) return fail(OKX_ERR_INVALID, "%s: null weight table or ldw < n_scenarios", who);
  const long long threads = (long long)n_geometries * n_scenarios;
  OKX_LAUNCH(tl::okx_tilt_weights, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_latents, (long long)ldz, n_latents, d_tilt,
             n_scenarios, (long long)n_geometries, d_weights, (long long)ldw);
  return OKX_OK;
}

size_t okx_ensemble_reweigh_scratch_bytes(int64_t n_geometries, int64_t steps, int32_t n_columns, int32_t n_scenarios) {
  namespace tl = okx::tilt;
  if (n_geometries <= 0 || steps < 0 || n_columns < 0 || n_scenarios < 1 || n_scenarios > OKX_ENS_TILT_MAX_SCENARIOS) return 0;
  return tl::layout(n_geometries, (long long)steps * n_columns, n_scenarios).total();
}

int32_t okx_ensemble_reweigh(int64_t n_geometries, int64_t steps, int32_t n_columns, const double* d_values, int64_t ld, const uint8_t* d_status,
                             int64_t status_stride, const uint8_t* d_mask, const double* d_shift, const double* d_weights, int64_t ldw,
                             int32_t n_scenarios, const double* d_limits, const uint8_t* d_verdict, int32_t accumulate, double* d_acc, double* d_joint,
                             void* d_scratch, size_t scratch_bytes, void* stream) {
  namespace tl = okx::tilt;
  const char* who = "okx_ensemble_reweigh";
  if (int rc = et::check_counts(who, n_geometries, steps, n_columns)) return rc;
  if (int rc = tl::check_scenarios(who, n_scenarios)) return rc;
  // (one thread per (scenario, field, entry) in the merge, and (entry tile, scenario tile) in blockIdx.x)
  if (int rc = et::check_entries(who, steps, n_columns, (1ll << 38) / ((long long)tl::kFields * n_scenarios))) return rc;
  if (n_geometries > (1ll << 38) / n_scenarios) return fail(OKX_ERR_LIMIT, "%s: too many geometries for one call", who);
  const long long n_entries = (long long)steps * n_columns;
  if (!d_joint || (n_entries > 0 && (!d_acc || !d_shift))) return fail(OKX_ERR_INVALID, "%s: null accumulator or shift table", who);
  if (n_geometries > 0 && (!d_weights || ldw < n_scenarios)) return fail(OKX_ERR_INVALID, "%s: null weight table or ldw < n_scenarios", who);
  if (int rc = et::check_table(who, n_entries > 0 && n_geometries > 0, d_values, ld, n_columns, d_status, status_stride)) return rc;
  const size_t need = okx_ensemble_reweigh_scratch_bytes(n_geometries, steps, n_columns, n_scenarios);
  if (need > 0) {
    if (int rc = et::check_scratch(who, "okx_ensemble_reweigh_scratch_bytes", need, d_scratch, scratch_bytes)) return rc;
    if (reinterpret_cast<uintptr_t>(d_scratch) % 8) return fail(OKX_ERR_INVALID, "%s: the scratch buffer must be 8-byte aligned", who);
  }
  const hipStream_t st = (hipStream_t)stream;
  const tl::Layout l = tl::layout(n_geometries, n_entries, n_scenarios);
  double* partial = static_cast<double*>(d_scratch);
  double* joint_partial = l.n_slabs > 0 ? reinterpret_cast<double*>(static_cast<unsigned char*>(d_scratch) + l.partial_bytes) : nullptr;
  const long long tiles = (n_entries + tl::kTile - 1) / tl::kTile;
  const long long sts = tl::scenario_tiles(n_scenarios);
  if (tiles * sts > 0x7fffffffll) return fail(OKX_ERR_LIMIT, "%s: too many entries for one call", who);
  if (l.n_slabs > 0) {
    tl::Args a{};
    et::set_table(&a, et::table_view(d_values, ld, d_status, status_stride, n_geometries, steps, n_columns));
    a.mask = d_mask; a.shift = d_shift; a.weights = d_weights; a.limits = d_limits; a.verdict = d_verdict;
    a.partial = partial; a.joint_partial = joint_partial;
    a.n_entries = n_entries; a.slab_len = l.slab_len; a.ldw = ldw; a.n_scenarios = n_scenarios;
    if (n_entries > 0) OKX_LAUNCH(tl::okx_tilt_partial, dim3((unsigned)(tiles * sts), (unsigned)l.n_slabs), dim3(tl::kTile), 0, st, a);
    OKX_LAUNCH(tl::okx_tilt_joint, dim3((unsigned)((n_scenarios + tl::kTile - 1) / tl::kTile), (unsigned)l.n_slabs), dim3(tl::kTile), 0, st, a);
  }
  const long long words = (long long)n_scenarios * tl::kFields * n_entries;
  if (words > 0)
    OKX_LAUNCH(tl::okx_tilt_merge, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, partial, l.n_slabs, words, accumulate ? 1 : 0, d_acc);
  const long long joint_words = (long long)n_scenarios * tl::kJoint;
  OKX_LAUNCH(tl::okx_tilt_merge, dim3((unsigned)((joint_words + 255) / 256)), dim3(256), 0, st, joint_partial, l.n_slabs, joint_words, accumulate ? 1 : 0,
             d_joint);
  return OKX_OK;
}

}  // extern "C"
