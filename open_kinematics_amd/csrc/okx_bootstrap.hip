// Poisson bootstrap of the ensemble chain (okx_ensemble_bootstrap_weights, okx_ensemble_sobol_bootstrap, include/okx.h): R
// replicates of the Sobol' accumulators of okx_sobol.hip, replicate r with every family's term multiplied by the family's
// Poisson(1) weight - a pure function of (seed, global family index, r), so chunks, devices and ranks form the same replicates
// and merge by addition.
//
// Three kernels fill the scratch buffer, a fourth merges it:
//  - okx_boot_weights: one thread per (row, four replicates) - one Philox4x32-10 call, four weights by thirteen integer
//    comparisons each (the thresholds of the header), stored as bytes [row][ld].  The public entry point stores [n][R]; the
//    Sobol' pass pads a row to a multiple of RT with zeros, so that its kernel reads a replicate tile's weights as ONE
//    aligned 8-byte word - a wave-uniform (scalar) load per family, never a draw per lane or per term.
//  - okx_boot_counts: the counting rule of okx_ensemble_sobol once per (family, entry), a byte [family][entry]: the rule
//    reads all M members of a family, and the replicate kernel below would otherwise read them all in every one of its
//    (group tile x replicate tile) workgroups; with the byte a workgroup reads only the 2 + GT members whose terms it forms.
//  - okx_sobol_boot_partial: the layout of okx_sobol_partial - a lane owns one of 64 entries, a wavefront (= workgroup)
//    walks the families of a slab - with the groups tiled by GT = 4 and the replicates by RT = 8.  The six common fields are
//    a tile of their own (two rows per family, 6 RT sums); a group tile reads A, B and its four members and keeps 3 GT RT =
//    96 sums (192 VGPRs), so no workgroup holds (6 + 3 GT) RT.  The next family's rows are loaded before this family's
//    arithmetic.  Built for TWO wavefronts per SIMD (256 VGPRs, 28 bytes of scratch per lane): at one wavefront the same
//    body needs 262 registers and no scratch and took 1.20 to 1.31 times as long at C5's shape (profiles/r21/).  The weights of the tile are in scalar registers; a replicate whose weight is 0 for the family is skipped
//    by a scalar branch (37 % of them - adding +0 to a sum that started at +0 changes no bit).  blockIdx.x runs over
//    (entry tile, replicate tile, group tile) with the tiles of one (entry tile, slab) adjacent, so workgroups resident
//    together read the same rows from L2.
//  - okx_sobol_boot_merge: one thread per (replicate, field, entry), the slabs in ascending order after d_acc's own content
//    when the call accumulates.
// The slab plan never looks at the device, there is no floating-point atomic, and contraction is off for the unit: every
// difference and product is rounded on its own as ensemble_stats.sobol_terms forms them, then term * (double)w, then the
// add - ensemble_stats.sobol_bootstrap_host.  The bits repeat from run to run and from device to device.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/okx.h"
#include "okx_enstable.hpp"
#include "okx_philox.hpp"
#include "okx_program.hpp"

#pragma clang fp contract(off)

namespace okx {
namespace boot {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int kTile = 64;                // entries per workgroup: one per lane, one wavefront
constexpr int kFields = OKX_SOBOL_FIELDS;
constexpr int kGT = 4;                   // groups per group tile
constexpr int kRT = 8;                   // replicates per replicate tile: their weights are one 8-byte word
constexpr long long kMinSlab = 32;       // families (as okx_sobol.hip)
constexpr long long kWantGroups = 2048;  // stage-1 wavefronts aimed at, over all tiles
constexpr int kMaxWeight = OKX_ENS_BOOTSTRAP_MAX_WEIGHT;

// floor(2^32 sum_{j <= k} e^-1 / j!), k = 0 .. 12 (include/okx.h; ensemble_stats.BOOTSTRAP_THRESHOLDS)
__constant__ const u32 kThreshold[kMaxWeight] = {0x5e2d58d8u, 0xbc5ab1b1u, 0xeb715e1du, 0xfb239797u, 0xff1025f5u, 0xffd90f3bu, 0xfffa8b71u,
                                                 0xffff540cu, 0xffffed1fu, 0xfffffe21u, 0xffffffd4u, 0xfffffffcu, 0xffffffffu};

// ---- the weights ----

// One thread per (row, word group q): weights of replicates 4 q .. 4 q + 3 of global row offset + row, bytes at
// weights[row * ld + r] for r < ld (r >= n_replicates: padding, 0).  ld >= n_replicates.
__global__ __launch_bounds__(256) void okx_boot_weights(unsigned char* weights, long long n_rows, long long ld, int n_replicates, u64 offset, u32 key0,
                                                        u32 key1) {
  const long long quads = (ld + 3) / 4;
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rows * quads) return;
  const long long row = t / quads;
  const int q = (int)(t % quads);
  const u64 i = offset + (u64)row;
  u32 word[4] = {0u, 0u, 0u, 0u};
  if (4 * q < n_replicates) rng::philox4x32_10((u32)i, (u32)(i >> 32), (u32)q, (u32)OKX_SAMPLE_PURPOSE_BOOTSTRAP << 8, key0, key1, word);
  unsigned char* out = weights + row * ld;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long r = 4ll * q + k;
    if (r >= ld) continue;
    u32 w = 0u;
#pragma unroll
    for (int j = 0; j < kMaxWeight; ++j) w += word[k] >= kThreshold[j] ? 1u : 0u;
    out[r] = (unsigned char)(r < n_replicates ? w : 0u);
  }
}

inline int check_weights(const char* who, long long n_rows, long long row_offset, int n_replicates) {
  if (n_rows < 0 || row_offset < 0) return fail(OKX_ERR_INVALID, "%s: negative row count or offset", who);
  if (n_replicates < 1 || n_replicates > OKX_ENS_BOOTSTRAP_MAX_REPLICATES)
    return fail(OKX_ERR_INVALID, "%s: %d replicates, 1 to %d allowed", who, n_replicates, (int)OKX_ENS_BOOTSTRAP_MAX_REPLICATES);
  if (n_rows > (1ll << 38) / ((n_replicates + 3) / 4 + 2)) return fail(OKX_ERR_LIMIT, "%s: too many rows for one call", who);
  return OKX_OK;
}

inline int launch_weights(unsigned char* weights, long long n_rows, long long ld, int n_replicates, long long row_offset, uint64_t seed,
                          hipStream_t st) {
  const long long threads = n_rows * ((ld + 3) / 4);
  if (threads == 0) return OKX_OK;
  OKX_LAUNCH(okx_boot_weights, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, weights, n_rows, ld, n_replicates, (u64)row_offset,
             (u32)(seed & 0xFFFFFFFFull), (u32)(seed >> 32));
  return OKX_OK;
}

// ---- the Sobol' replicates ----

inline int group_tiles(int n_groups) { return (n_groups + kGT - 1) / kGT; }
inline int replicate_tiles(int n_replicates) { return (n_replicates + kRT - 1) / kRT; }
// workgroups per (entry tile, slab): per replicate tile the common fields' tile and the group tiles
inline long long tiles_per_slab(int n_groups, int n_replicates) { return (1ll + group_tiles(n_groups)) * replicate_tiles(n_replicates); }

inline void slab_plan(long long n_families, long long n_entries, int n_groups, int n_replicates, long long* n_slabs, long long* slab_len) {
  const long long per = tiles_per_slab(n_groups, n_replicates);
  enstable::slab_plan(n_families, n_entries, kTile, (kWantGroups + per - 1) / per, kMinSlab, 65535, n_slabs, slab_len);
}

struct Args {
  const double* values;
  const unsigned char* status;
  const unsigned char* mask;     // [n_geom] or null
  const double* shift;
  const unsigned char* weights;  // [n_families][w_ld], w_ld a multiple of kRT, 8-byte aligned
  unsigned char* counts;         // [n_families][n_entries]: 1 where the family counts
  double* partial;               // [n_slabs][n_replicates][kFields + 3 D][n_entries]
  long long ld, status_stride;
  long long n_geom, steps;       // n_geom = n_families * members
  long long n_families, n_entries, slab_len, w_ld;
  int n_columns, n_groups, members, n_replicates, families_per_group;
};

// The counting rule, once per (family, entry): blockIdx.y owns families_per_group consecutive families.
__global__ __launch_bounds__(kTile) void okx_boot_counts(Args a) {
  const long long e = (long long)blockIdx.x * kTile + threadIdx.x;
  if (e >= a.n_entries) return;
  const enstable::Table t = OKX_ENS_TABLE_OF(a);
  const double* vp = enstable::entry_values(t, e);
  const unsigned char* sp = enstable::entry_status(t, e);
  const long long v_step = enstable::value_step(t), s_step = enstable::status_step(t);
  const long long f0 = (long long)blockIdx.y * a.families_per_group;
  const long long f1 = f0 + a.families_per_group < a.n_families ? f0 + a.families_per_group : a.n_families;
  for (long long f = f0; f < f1; ++f) {
    const long long g = f * a.members;
    bool ok = true;
    for (int m = 0; m < a.members; ++m) {
      const double v = vp[(g + m) * v_step];
      ok = ok && OKX_ENS_ACCEPTED(OKX_ENS_STATUS_AT(sp, g + m, s_step), v);
    }
    if (a.mask) {  // (bytes uniform over the wavefront)
      unsigned bad = 0u;
      for (int m = 0; m < a.members; ++m) bad |= a.mask[g + m];
      ok = ok && (bad & 1u) == 0u;
    }
    a.counts[f * a.n_entries + e] = ok ? 1 : 0;
  }
}

// sums[i] += (double)w_i * term for the replicates of the tile whose weight is not 0 (w: eight weights, one per byte)
#define OKX_BOOT_FOR_WEIGHTS(w, i, wd)                                  \
  _Pragma("unroll") for (int i = 0; i < kRT; ++i)                       \
    if (const u32 w_##i = (u32)((w) >> (8 * i)) & 0xFFu)                \
      if (const double wd = (double)w_##i; true)

__global__ __launch_bounds__(kTile, 2) void okx_sobol_boot_partial(Args a) {
  const int lane = threadIdx.x;
  const int gts = 1 + (a.n_groups + kGT - 1) / kGT;              // tiles per replicate tile: the common fields', then the groups'
  const int per = gts * ((a.n_replicates + kRT - 1) / kRT);
  const long long tile = blockIdx.x / (unsigned)per;
  const int z = (int)(blockIdx.x % (unsigned)per);
  const int gt = z % gts, rt = z / gts;
  const int r0 = rt * kRT;
  const int nr = a.n_replicates - r0 < kRT ? a.n_replicates - r0 : kRT;  // replicates of the tile (>= 1)
  const long long e = tile * kTile + lane;
  const bool live = e < a.n_entries;
  const long long er = live ? e : 0;  // a lane past the table walks entry 0 and stores nothing
  const long long slab = blockIdx.y;
  const long long f0 = slab * a.slab_len;
  const long long f1 = f0 + a.slab_len < a.n_families ? f0 + a.slab_len : a.n_families;
  const enstable::Table t = OKX_ENS_TABLE_OF(a);
  const double* vp = enstable::entry_values(t, er);
  const long long v_step = enstable::value_step(t);
  const unsigned char* cp = a.counts + er;
  const unsigned char* wp = a.weights + r0;  // (w_ld and r0 multiples of 8: an aligned word per family)
  const double sh = a.shift[er];
  const long long rows = kFields + 3ll * a.n_groups;
  double* out = a.partial + ((slab * a.n_replicates + r0) * rows) * a.n_entries + e;
  const long long out_rep = rows * a.n_entries;
  if (gt == 0) {
    // the six common fields
    double count[kRT], dropped[kRT], sum_a[kRT], sum_b[kRT], sq_a[kRT], sq_b[kRT];
#pragma unroll
    for (int i = 0; i < kRT; ++i) count[i] = dropped[i] = sum_a[i] = sum_b[i] = sq_a[i] = sq_b[i] = 0.0;
    double va = 0.0, vb = 0.0;
    unsigned char ok8 = 0;
    u64 wn = 0;
    if (f0 < f1) {
      va = vp[f0 * a.members * v_step]; vb = vp[(f0 * a.members + 1) * v_step]; ok8 = cp[f0 * a.n_entries];
      wn = *reinterpret_cast<const u64*>(wp + f0 * a.w_ld);  // (uniform over the wavefront: a scalar load)
    }
    for (long long f = f0; f < f1; ++f) {
      const double ca = va, cb = vb;
      const bool ok = ok8 != 0;
      const u64 w = wn;
      if (f + 1 < f1) {  // the next family's rows and weights, in flight over this family's arithmetic
        const long long g = (f + 1) * a.members;
        va = vp[g * v_step]; vb = vp[(g + 1) * v_step]; ok8 = cp[(f + 1) * a.n_entries];
        wn = *reinterpret_cast<const u64*>(wp + (f + 1) * a.w_ld);
      }
      const double da = ok ? ca - sh : 0.0, db = ok ? cb - sh : 0.0;
      const double one = ok ? 1.0 : 0.0, none = ok ? 0.0 : 1.0;
      const double aa = da * da, bb = db * db;
      OKX_BOOT_FOR_WEIGHTS(w, i, wd) {
        count[i] += wd * one; dropped[i] += wd * none;
        sum_a[i] += wd * da; sum_b[i] += wd * db;
        sq_a[i] += wd * aa; sq_b[i] += wd * bb;
      }
    }
    if (!live) return;
#pragma unroll
    for (int i = 0; i < kRT; ++i)
      if (i < nr) {
        double* o = out + i * out_rep;
        o[OKX_SOBOL_COUNT * a.n_entries] = count[i]; o[OKX_SOBOL_DROPPED * a.n_entries] = dropped[i];
        o[OKX_SOBOL_SUM_A * a.n_entries] = sum_a[i]; o[OKX_SOBOL_SUM_B * a.n_entries] = sum_b[i];
        o[OKX_SOBOL_SUMSQ_A * a.n_entries] = sq_a[i]; o[OKX_SOBOL_SUMSQ_B * a.n_entries] = sq_b[i];
      }
    return;
  }
  // a tile of kGT groups: P_j, Q_j, R_j
  const int j0 = (gt - 1) * kGT;                                 // the tile's first group
  const int nj = a.n_groups - j0 < kGT ? a.n_groups - j0 : kGT;  // and how many it has (>= 1)
  double p[kRT][kGT], q[kRT][kGT], r[kRT][kGT];
#pragma unroll
  for (int i = 0; i < kRT; ++i)
#pragma unroll
    for (int j = 0; j < kGT; ++j) p[i][j] = q[i][j] = r[i][j] = 0.0;
  double va = 0.0, vb = 0.0, vj[kGT];
#pragma unroll
  for (int j = 0; j < kGT; ++j) vj[j] = 0.0;
  unsigned char ok8 = 0;
  u64 wn = 0;
  if (f0 < f1) {
    const long long g = f0 * a.members;
    va = vp[g * v_step]; vb = vp[(g + 1) * v_step]; ok8 = cp[f0 * a.n_entries];
    wn = *reinterpret_cast<const u64*>(wp + f0 * a.w_ld);
#pragma unroll
    for (int j = 0; j < kGT; ++j) vj[j] = vp[(g + (j < nj ? 2 + j0 + j : 0)) * v_step];  // (slots past the last group read A again; nobody stores their sums)
  }
  for (long long f = f0; f < f1; ++f) {
    const double ca = va, cb = vb;
    double cj[kGT];
#pragma unroll
    for (int j = 0; j < kGT; ++j) cj[j] = vj[j];
    const bool ok = ok8 != 0;
    const u64 w = wn;
    if (f + 1 < f1) {
      const long long g = (f + 1) * a.members;
      va = vp[g * v_step]; vb = vp[(g + 1) * v_step]; ok8 = cp[(f + 1) * a.n_entries];
      wn = *reinterpret_cast<const u64*>(wp + (f + 1) * a.w_ld);
#pragma unroll
      for (int j = 0; j < kGT; ++j) vj[j] = vp[(g + (j < nj ? 2 + j0 + j : 0)) * v_step];
    }
    const double da = ok ? ca - sh : 0.0, db = ok ? cb - sh : 0.0;
    double tp[kGT], tq[kGT], tr[kGT];
#pragma unroll
    for (int j = 0; j < kGT; ++j) {
      const double dj = ok ? cj[j] - sh : 0.0;
      const double ua = da - dj, ub = db - dj;
      tp[j] = db * (dj - da);
      tq[j] = ua * ua;
      tr[j] = ub * ub;
    }
    OKX_BOOT_FOR_WEIGHTS(w, i, wd) {
#pragma unroll
      for (int j = 0; j < kGT; ++j) {
        p[i][j] += wd * tp[j];
        q[i][j] += wd * tq[j];
        r[i][j] += wd * tr[j];
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int i = 0; i < kRT; ++i)
    if (i < nr) {
#pragma unroll
      for (int j = 0; j < kGT; ++j)
        if (j < nj) {
          double* o = out + i * out_rep + (kFields + 3ll * (j0 + j)) * a.n_entries;
          o[0] = p[i][j]; o[a.n_entries] = q[i][j]; o[2 * a.n_entries] = r[i][j];
        }
    }
}

// One thread per (replicate, field, entry): the slabs in ascending order, after d_acc's own content when the call
// accumulates; eight slabs' loads in flight, added in the same order (as okx_sobol_merge).
__global__ __launch_bounds__(256) void okx_sobol_boot_merge(const double* partial, long long n_slabs, long long n_entries, int rows, int n_replicates,
                                                            int accumulate, double* acc) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long per = n_entries * rows;
  if (t >= per * n_replicates) return;
  const long long rep = t / per, u = t % per;
  const int field = (int)(u / n_entries);
  const long long e = u % n_entries;
  double* out = acc + (rep * n_entries + e) * rows + field;
  const double* in = partial + t;  // [slab][replicate][field][entry]
  const long long step = per * n_replicates;
  double x = accumulate ? *out : 0.0;
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

inline int check_sizes(const char* who, long long n_families, long long family_offset, int n_groups, long long steps, int n_columns,
                       int n_replicates) {
  if (int rc = enstable::check_counts(who, n_families, steps, n_columns)) return rc;
  if (family_offset < 0) return fail(OKX_ERR_INVALID, "%s: negative family_offset", who);
  if (n_groups < 1 || n_groups > OKX_ENS_SOBOL_MAX_GROUPS)
    return fail(OKX_ERR_INVALID, "%s: %d groups, 1 to %d allowed", who, n_groups, (int)OKX_ENS_SOBOL_MAX_GROUPS);
  if (n_replicates < 1 || n_replicates > OKX_ENS_BOOTSTRAP_MAX_REPLICATES)
    return fail(OKX_ERR_INVALID, "%s: %d replicates, 1 to %d allowed", who, n_replicates, (int)OKX_ENS_BOOTSTRAP_MAX_REPLICATES);
  if (n_families > (1ll << 53) / (n_groups + 2)) return fail(OKX_ERR_LIMIT, "%s: geometry indices beyond 2^53", who);
  if (n_families > (1ll << 38) / ((n_replicates + kRT - 1) / kRT * kRT)) return fail(OKX_ERR_LIMIT, "%s: too many families for one call", who);
  // (one thread per (replicate, field, entry) in the merge, and (entry tile, tile) in blockIdx.x)
  return enstable::check_entries(who, steps, n_columns, (1ll << 38) / ((long long)(kFields + 3 * n_groups) * n_replicates));
}

// the scratch buffer: partials, then the padded weights, then the counting bytes (each a multiple of 8 bytes)
struct Layout {
  long long n_slabs, slab_len, w_ld;
  size_t partial_bytes, weight_bytes, count_bytes;
  size_t total() const { return partial_bytes + weight_bytes + count_bytes; }
};

inline Layout layout(long long n_families, int n_groups, long long n_entries, int n_replicates) {
  Layout l{};
  slab_plan(n_families, n_entries, n_groups, n_replicates, &l.n_slabs, &l.slab_len);
  l.w_ld = (long long)replicate_tiles(n_replicates) * kRT;
  l.partial_bytes = sizeof(double) * (size_t)l.n_slabs * (size_t)n_replicates * (size_t)(kFields + 3 * n_groups) * (size_t)n_entries;
  l.weight_bytes = (size_t)n_families * (size_t)l.w_ld;
  l.count_bytes = ((size_t)n_families * (size_t)n_entries + 7) / 8 * 8;
  return l;
}

}  // namespace boot
}  // namespace okx

using okx::fail;
namespace et = okx::enstable;

extern "C" {

int32_t okx_ensemble_bootstrap_weights(int64_t n_rows, int64_t row_offset, uint64_t seed, int32_t n_replicates, uint8_t* d_weights, void* stream) {
  namespace bt = okx::boot;
  const char* who = "okx_ensemble_bootstrap_weights";
  if (int rc = bt::check_weights(who, n_rows, row_offset, n_replicates)) return rc;
  if (n_rows == 0) return OKX_OK;
  if (!d_weights) return fail(OKX_ERR_INVALID, "%s: null weight table", who);
  return bt::launch_weights(d_weights, n_rows, n_replicates, n_replicates, row_offset, seed, (hipStream_t)stream);
}

size_t okx_ensemble_sobol_bootstrap_scratch_bytes(int64_t n_families, int32_t n_groups, int64_t steps, int32_t n_columns, int32_t n_replicates) {
  namespace bt = okx::boot;
  if (n_families <= 0 || steps < 0 || n_columns < 0 || n_groups < 1 || n_groups > OKX_ENS_SOBOL_MAX_GROUPS || n_replicates < 1 ||
      n_replicates > OKX_ENS_BOOTSTRAP_MAX_REPLICATES)
    return 0;
  return bt::layout(n_families, n_groups, (long long)steps * n_columns, n_replicates).total();
}

int32_t okx_ensemble_sobol_bootstrap(int64_t n_families, int64_t family_offset, int32_t n_groups, int64_t steps, int32_t n_columns,
                                     const double* d_values, int64_t ld, const uint8_t* d_status, int64_t status_stride, const uint8_t* d_mask,
                                     const double* d_shift, uint64_t seed, int32_t n_replicates, int32_t accumulate, double* d_acc, void* d_scratch,
                                     size_t scratch_bytes, void* stream) {
  namespace bt = okx::boot;
  const char* who = "okx_ensemble_sobol_bootstrap";
  if (int rc = bt::check_sizes(who, n_families, family_offset, n_groups, steps, n_columns, n_replicates)) return rc;
  const long long n_entries = (long long)steps * n_columns;
  if (n_entries > 0 && (!d_acc || !d_shift)) return fail(OKX_ERR_INVALID, "%s: null accumulator or shift table", who);
  if (int rc = et::check_table(who, n_entries > 0 && n_families > 0, d_values, ld, n_columns, d_status, status_stride)) return rc;
  const size_t need = okx_ensemble_sobol_bootstrap_scratch_bytes(n_families, n_groups, steps, n_columns, n_replicates);
  if (need > 0) {
    if (int rc = et::check_scratch(who, "okx_ensemble_sobol_bootstrap_scratch_bytes", need, d_scratch, scratch_bytes)) return rc;
    if (reinterpret_cast<uintptr_t>(d_scratch) % 8) return fail(OKX_ERR_INVALID, "%s: the scratch buffer must be 8-byte aligned", who);
  }
  if (n_entries == 0) return OKX_OK;
  const hipStream_t st = (hipStream_t)stream;
  const int rows = bt::kFields + 3 * n_groups;
  const bt::Layout l = bt::layout(n_families, n_groups, n_entries, n_replicates);
  double* partial = static_cast<double*>(d_scratch);
  if (l.n_slabs > 0) {
    unsigned char* weights = static_cast<unsigned char*>(d_scratch) + l.partial_bytes;
    const long long members = n_groups + 2;
    const long long tiles = (n_entries + bt::kTile - 1) / bt::kTile;
    const long long per = bt::tiles_per_slab(n_groups, n_replicates);
    if (tiles * per > 0x7fffffffll) return fail(OKX_ERR_LIMIT, "%s: too many entries for one call", who);
    if (int rc = bt::launch_weights(weights, n_families, l.w_ld, n_replicates, family_offset, seed, st)) return rc;
    bt::Args a{};
    et::set_table(&a, et::table_view(d_values, ld, d_status, status_stride, n_families * members, steps, n_columns));
    a.mask = d_mask; a.shift = d_shift; a.weights = weights; a.counts = weights + l.weight_bytes; a.partial = partial;
    a.n_families = n_families; a.n_entries = n_entries; a.slab_len = l.slab_len; a.w_ld = l.w_ld;
    a.n_groups = n_groups; a.members = (int)members; a.n_replicates = n_replicates;
    a.families_per_group = (int)((n_families + 65534) / 65535 < 8 ? 8 : (n_families + 65534) / 65535);
    OKX_LAUNCH(bt::okx_boot_counts, dim3((unsigned)tiles, (unsigned)((n_families + a.families_per_group - 1) / a.families_per_group)), dim3(bt::kTile), 0,
               st, a);
    OKX_LAUNCH(bt::okx_sobol_boot_partial, dim3((unsigned)(tiles * per), (unsigned)l.n_slabs), dim3(bt::kTile), 0, st, a);
  }
  const long long threads = n_entries * rows * n_replicates;
  OKX_LAUNCH(bt::okx_sobol_boot_merge, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, partial, l.n_slabs, n_entries, rows, n_replicates,
             accumulate ? 1 : 0, d_acc);
  return OKX_OK;
}

}  // extern "C"
