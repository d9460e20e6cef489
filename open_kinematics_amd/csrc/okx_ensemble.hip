// Ensemble reduction (okx_ensemble_reduce, include/okx.h): moments, extremes and factor cross-moments of a table of metric
// columns [G * S][ld] over its G geometries, per (step, column) entry, fp64 throughout, no floating-point atomics.
//
// Row g * S + s of the table is contiguous in (s, k), so a lane owns one entry e = s * K + k and walks geometries: every
// wave-instruction reads 64 consecutive doubles (ld == K), the factors of a geometry are uniform over the wavefront (the
// compiler reads them through the scalar cache) and every accumulator lives in registers - 8 moments + up to 32 cross sums.
// Stage 1 (okx_ensemble_partial): one workgroup per (tile of 64 entries, slab of geometries, block of 32 factors); its four
// wavefronts take the slab's four contiguous quarters and wave 0 merges them through LDS in ascending order, so a
// workgroup leaves ONE partial accumulator in scratch [slab][field][entry].  Stage 2 (okx_ensemble_merge): one thread per
// (entry, field) merges the slabs in ascending order, after what d_acc already holds when the call accumulates.
// The order of every addition is a function of (G, S, K) alone - the slab count never looks at the device - so the bits
// are the same from run to run and from machine to machine.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/okx.h"
#include "okx_enstable.hpp"
#include "okx_program.hpp"

namespace okx {
namespace ens {

constexpr int kTile = 64;       // entries per workgroup: one per lane
constexpr int kWaves = 4;       // quarters of a slab
constexpr int kThreads = kTile * kWaves;
constexpr int kFactorBlock = 32;  // cross sums a lane keeps in registers
constexpr int kFields = OKX_ENS_FIELDS;
constexpr long long kMinSlab = 16;       // geometries: below this a slab costs more in stage 2 than it spreads in stage 1
constexpr long long kWantGroups = 512;   // stage-1 workgroups aimed at (two per CU of a 256-CU part, from the problem size alone)

struct EnsArgs {
  const double* values;
  const unsigned char* status;
  const double* factors;
  const double* shift;
  double* partial;          // [n_slabs][fields + P][n_entries]
  long long ld, status_stride;
  long long n_geom, steps, n_entries, slab_len, geometry_offset;
  int n_columns, n_factors;
};

// slabs of a call: from the problem size only
inline void slab_plan(long long n_geom, long long n_entries, long long* n_slabs, long long* slab_len) {
  enstable::slab_plan(n_geom, n_entries, kTile, kWantGroups, kMinSlab, enstable::kNoCap, n_slabs, slab_len);
}

inline long long factor_moments(int p) { return p > 0 ? (long long)p + (long long)p * (p + 1) / 2 + 1 : 0; }

// an extreme (value, index) against the one held: strictly better wins, a tie goes to the LOWER index; index < 0: nothing there
template <bool kMin>
__device__ inline void take_extreme(double v, double i, double& held, double& held_i) {
  if (i < 0.0) return;
  if (held_i < 0.0 || (kMin ? v < held : v > held) || (v == held && i < held_i)) { held = v; held_i = i; }
}

template <int PB>
__global__ __launch_bounds__(kThreads) void okx_ensemble_partial(EnsArgs a) {
  extern __shared__ double ens_lds[];  // [kWaves - 1][kFields + PB][kTile]
  constexpr int kC = PB > 0 ? PB : 1;
  constexpr int kUnroll = PB >= 16 ? 1 : (PB > 0 ? 2 : 4);  // (a geometry's factors sit in scalar registers: more in flight would spill them)
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform, and known to be: the factor reads go through the scalar cache)
  const long long e = (long long)blockIdx.x * kTile + lane;
  const bool live = e < a.n_entries;
  const long long er = live ? e : 0;  // a lane past the table walks entry 0 and stores nothing
  const long long slab = blockIdx.y;
  const int p0 = (int)blockIdx.z * PB;
  const int np = a.n_factors - p0 < PB ? a.n_factors - p0 : PB;
  const long long g0 = slab * a.slab_len;
  const long long g1 = g0 + a.slab_len < a.n_geom ? g0 + a.slab_len : a.n_geom;
  const long long quarter = (g1 - g0 + kWaves - 1) / kWaves;
  const long long ga = g0 + wave * quarter < g1 ? g0 + wave * quarter : g1;
  const long long gb = ga + quarter < g1 ? ga + quarter : g1;
  const enstable::Table t = OKX_ENS_TABLE_OF(a);
  const double* vp = enstable::entry_values(t, er);
  const unsigned char* sp = enstable::entry_status(t, er);
  const long long v_step = enstable::value_step(t), s_step = enstable::status_step(t);
  const double sh = a.shift[er];
  double count = 0.0, rejected = 0.0, sum = 0.0, sumsq = 0.0;
  double mn = __builtin_inf(), mx = -__builtin_inf(), amin = -1.0, amax = -1.0;
  double c[kC];
#pragma unroll
  for (int p = 0; p < kC; ++p) c[p] = 0.0;
  // One geometry into the accumulators.  kWhole: the PB factors from f[0] on are read with constant offsets (wide scalar
  // loads); slots past the block's last factor then read into the FOLLOWING geometries' rows and sum junk nobody stores -
  // legal only while those reads end inside the table: the last geometries (one for P >= PB / 2, up to PB - 1 for P = 1)
  // take the selecting form.
  auto geometry = [&](long long g, auto whole) {
    constexpr bool kWhole = decltype(whole)::value;
    const double v = vp[g * v_step];
    const bool ok = OKX_ENS_ACCEPTED(OKX_ENS_STATUS_AT(sp, g, s_step), v);
    const double d = ok ? v - sh : 0.0;
    count += ok ? 1.0 : 0.0;
    rejected += ok ? 0.0 : 1.0;
    sum += d;
    sumsq = fma(d, d, sumsq);
    const double gi = (double)(a.geometry_offset + g);
    if (ok && v < mn) { mn = v; amin = gi; }
    if (ok && v > mx) { mx = v; amax = gi; }
    if (PB > 0) {
      const double* f = a.factors + g * a.n_factors + p0;  // uniform over the wavefront
#pragma unroll
      for (int p = 0; p < PB; ++p) c[p] = fma(f[kWhole ? p : (p < np ? p : 0)], d, c[p]);
    }
  };
  // (whole reads of geometry g end at double g P + p0 + PB of the [G][P] table: legal while that is <= G P)
  const long long room = a.n_geom * a.n_factors - p0 - PB;
  const long long whole_end = np == PB ? gb : (room < 0 ? 0 : room / (a.n_factors > 0 ? a.n_factors : 1) + 1);
  const long long g_whole = whole_end < gb ? whole_end : gb;
#pragma unroll kUnroll
  for (long long g = ga; g < g_whole; ++g) geometry(g, std::true_type{});
  for (long long g = g_whole > ga ? g_whole : ga; g < gb; ++g) geometry(g, std::false_type{});
  // the quarters of the slab, merged by wave 0 in ascending order
  constexpr int kRows = kFields + PB;
  if (wave > 0) {
    double* w = ens_lds + (long long)(wave - 1) * kRows * kTile + lane;
    w[0 * kTile] = count; w[1 * kTile] = rejected; w[2 * kTile] = sum; w[3 * kTile] = sumsq;
    w[4 * kTile] = mn; w[5 * kTile] = mx; w[6 * kTile] = amin; w[7 * kTile] = amax;
#pragma unroll
    for (int p = 0; p < PB; ++p) w[(kFields + p) * kTile] = c[p];
  }
  __syncthreads();
  if (wave > 0 || !live) return;
#pragma unroll 1
  for (int q = 0; q < kWaves - 1; ++q) {
    const double* w = ens_lds + (long long)q * kRows * kTile + lane;
    count += w[0 * kTile]; rejected += w[1 * kTile]; sum += w[2 * kTile]; sumsq += w[3 * kTile];
    take_extreme<true>(w[4 * kTile], w[6 * kTile], mn, amin);
    take_extreme<false>(w[5 * kTile], w[7 * kTile], mx, amax);
#pragma unroll
    for (int p = 0; p < PB; ++p) c[p] += w[(kFields + p) * kTile];
  }
  const long long rows = kFields + a.n_factors;
  double* out = a.partial + slab * rows * a.n_entries + e;
  if (blockIdx.z == 0) {
    out[0 * a.n_entries] = count; out[1 * a.n_entries] = rejected; out[2 * a.n_entries] = sum; out[3 * a.n_entries] = sumsq;
    out[4 * a.n_entries] = mn; out[5 * a.n_entries] = mx; out[6 * a.n_entries] = amin; out[7 * a.n_entries] = amax;
  }
#pragma unroll
  for (int p = 0; p < PB; ++p)
    if (p < np) out[(kFields + p0 + p) * a.n_entries] = c[p];
}

template <int PB>
inline hipError_t launch_partial(const EnsArgs& a, long long n_slabs, hipStream_t st) {
  const unsigned tiles = (unsigned)((a.n_entries + kTile - 1) / kTile);
  const unsigned blocks = PB > 0 ? (unsigned)((a.n_factors + PB - 1) / PB) : 1u;
  const size_t lds = sizeof(double) * (size_t)(kWaves - 1) * (size_t)(kFields + PB) * (size_t)kTile;
  hipLaunchKernelGGL(okx_ensemble_partial<PB>, dim3(tiles, (unsigned)n_slabs, blocks), dim3(kThreads), lds, st, a);
  return hipGetLastError();
}

// One thread per (field, entry): the slabs in ascending order, after d_acc's own content when the call accumulates.
__global__ __launch_bounds__(256) void okx_ensemble_merge(const double* partial, long long n_slabs, long long n_entries, int rows,
                                                          int accumulate, double* acc) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_entries * rows) return;
  const int field = (int)(t / n_entries);
  const long long e = t % n_entries;
  if (field == OKX_ENS_ARGMIN || field == OKX_ENS_ARGMAX) return;  // written with their extreme
  double* out = acc + e * rows;
  const double* in = partial + (long long)field * n_entries + e;
  const long long step = (long long)rows * n_entries;
  if (field == OKX_ENS_MIN || field == OKX_ENS_MAX) {
    const bool is_min = field == OKX_ENS_MIN;
    double held = accumulate ? out[field] : (is_min ? __builtin_inf() : -__builtin_inf());
    double held_i = accumulate ? out[field + 2] : -1.0;
    for (long long k = 0; k < n_slabs; ++k) {
      const double v = in[k * step], i = in[k * step + 2 * n_entries];
      if (is_min) take_extreme<true>(v, i, held, held_i);
      else take_extreme<false>(v, i, held, held_i);
    }
    out[field] = held;
    out[field + 2] = held_i;
    return;
  }
  double x = accumulate ? out[field] : 0.0;
  for (long long k = 0; k < n_slabs; ++k) x += in[k * step];
  out[field] = x;
}

// The unmasked factor moments: element i of [sum f_p | sum f_p f_q (q <= p, row-major lower triangle) | count].
__device__ inline void factor_element(long long i, int n_factors, int* p, int* q) {
  if (i < n_factors) { *p = (int)i; *q = -1; return; }
  long long k = i - n_factors;
  int row = 0;
  while (k > row) { k -= row + 1; ++row; }
  if (row >= n_factors) { *p = -1; *q = -1; return; }  // the count
  *p = row; *q = (int)k;
}

__global__ __launch_bounds__(256) void okx_ensemble_factor_partial(const double* factors, int n_factors, long long n_geom, long long slab_len,
                                                                   long long n_moments, double* partial) {
  const long long slab = blockIdx.x;
  const long long g0 = slab * slab_len;
  const long long g1 = g0 + slab_len < n_geom ? g0 + slab_len : n_geom;
  for (long long i = threadIdx.x; i < n_moments; i += blockDim.x) {
    int p, q;
    factor_element(i, n_factors, &p, &q);
    double x = 0.0;
    if (p < 0) x = (double)(g1 - g0);
    else if (q < 0) for (long long g = g0; g < g1; ++g) x += factors[g * n_factors + p];
    else for (long long g = g0; g < g1; ++g) x = fma(factors[g * n_factors + p], factors[g * n_factors + q], x);
    partial[slab * n_moments + i] = x;
  }
}

__global__ __launch_bounds__(256) void okx_ensemble_factor_merge(const double* partial, long long n_slabs, long long n_moments, int accumulate,
                                                                 double* acc) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_moments) return;
  double x = accumulate ? acc[i] : 0.0;
  for (long long k = 0; k < n_slabs; ++k) x += partial[k * n_moments + i];
  acc[i] = x;
}

}  // namespace ens
}  // namespace okx

using okx::fail;
namespace et = okx::enstable;

extern "C" {

size_t okx_ensemble_scratch_bytes(int64_t n_geometries, int64_t steps, int32_t n_columns, int32_t n_factors) {
  namespace en = okx::ens;
  if (n_geometries <= 0 || steps < 0 || n_columns < 0 || n_factors < 0) return 0;
  const long long n_entries = (long long)steps * n_columns;
  long long n_slabs, slab_len;
  en::slab_plan(n_geometries, n_entries, &n_slabs, &slab_len);
  return sizeof(double) * (size_t)n_slabs * ((size_t)(en::kFields + n_factors) * (size_t)n_entries + (size_t)en::factor_moments(n_factors));
}

int32_t okx_ensemble_reduce(int64_t n_geometries, int64_t steps, int32_t n_columns, const double* d_values, int64_t ld,
                            const uint8_t* d_status, int64_t status_stride, const double* d_factors, int32_t n_factors,
                            const double* d_shift, int64_t geometry_offset, int32_t accumulate, double* d_acc, double* d_factor_acc,
                            void* d_scratch, size_t scratch_bytes, void* stream) {
  namespace en = okx::ens;
  if (int rc = et::check_counts("okx_ensemble_reduce", n_geometries, steps, n_columns)) return rc;
  if (n_factors < 0 || n_factors > OKX_ENS_MAX_FACTORS) return fail(OKX_ERR_LIMIT, "okx_ensemble_reduce: at most %d factors", OKX_ENS_MAX_FACTORS);
  if (geometry_offset < 0 || geometry_offset + n_geometries > (1ll << 53)) return fail(OKX_ERR_LIMIT, "okx_ensemble_reduce: geometry indices beyond 2^53");
  const long long n_entries = (long long)steps * n_columns;
  if (int rc = et::check_entries("okx_ensemble_reduce", steps, n_columns, (1ll << 38) / (en::kFields + n_factors))) return rc;
  if (n_entries > 0 && (!d_acc || !d_shift)) return fail(OKX_ERR_INVALID, "okx_ensemble_reduce: null accumulator or shift table");
  if (int rc = et::check_table("okx_ensemble_reduce", n_entries > 0 && n_geometries > 0, d_values, ld, n_columns, d_status, status_stride)) return rc;
  if (n_factors > 0 && n_geometries > 0 && !d_factors) return fail(OKX_ERR_INVALID, "okx_ensemble_reduce: n_factors > 0 without a factor table");
  if (d_factor_acc && n_factors < 1) return fail(OKX_ERR_INVALID, "okx_ensemble_reduce: factor moments need factors");
  const size_t need = okx_ensemble_scratch_bytes(n_geometries, steps, n_columns, n_factors);
  if (need > 0)
    if (int rc = et::check_scratch("okx_ensemble_reduce", "okx_ensemble_scratch_bytes", need, d_scratch, scratch_bytes)) return rc;
  long long n_slabs, slab_len;
  en::slab_plan(n_geometries, n_entries, &n_slabs, &slab_len);
  if (n_slabs > 65535) return fail(OKX_ERR_LIMIT, "okx_ensemble_reduce: too many geometries for one call");
  const hipStream_t st = (hipStream_t)stream;
  const int rows = en::kFields + n_factors;
  double* partial = static_cast<double*>(d_scratch);
  if (n_entries > 0) {
    if (n_slabs > 0) {
      en::EnsArgs a{};
      et::set_table(&a, et::table_view(d_values, ld, d_status, status_stride, n_geometries, steps, n_columns));
      a.factors = d_factors; a.shift = d_shift; a.partial = partial;
      a.n_entries = n_entries; a.slab_len = slab_len; a.geometry_offset = geometry_offset; a.n_factors = n_factors;
      // the cross sums of a lane stay in registers: blocks of 8, 16 or 32 factors, more than 32 as further workgroups
      if (n_factors == 0) HIP_TRY(en::launch_partial<0>(a, n_slabs, st));
      else if (n_factors <= 8) HIP_TRY(en::launch_partial<8>(a, n_slabs, st));
      else if (n_factors <= 16) HIP_TRY(en::launch_partial<16>(a, n_slabs, st));
      else HIP_TRY(en::launch_partial<en::kFactorBlock>(a, n_slabs, st));
    }
    const long long threads = n_entries * rows;
    OKX_LAUNCH(en::okx_ensemble_merge, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, partial, n_slabs, n_entries, rows,
               accumulate ? 1 : 0, d_acc);
  }
  if (d_factor_acc) {
    const long long n_moments = en::factor_moments(n_factors);
    double* fpart = partial + (size_t)n_slabs * (size_t)rows * (size_t)n_entries;
    if (n_slabs > 0) {
      OKX_LAUNCH(en::okx_ensemble_factor_partial, dim3((unsigned)n_slabs), dim3(256), 0, st, d_factors, n_factors, (long long)n_geometries,
                 slab_len, n_moments, fpart);
    }
    OKX_LAUNCH(en::okx_ensemble_factor_merge, dim3((unsigned)((n_moments + 255) / 256)), dim3(256), 0, st, fpart, n_slabs, n_moments,
               accumulate ? 1 : 0, d_factor_acc);
  }
  return OKX_OK;
}

}  // extern "C"
