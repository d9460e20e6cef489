// Ensemble selection (okx_ensemble_select*, include/okx.h): exact order statistics and spec-limit counts of a table of metric
// columns [G * S][ld] over its G geometries, per (step, column) entry - a radix select on order-preserving 64-bit keys,
// integer counting only, so that every partial result merges by integer addition in any order (chunks, slabs, ranks).
//
// A finite double orders like key = bits ^ (sign ? ~0 : 1 << 63) (okx_diagnose.hip's observation).  A selection (entry,
// probability q, side lo / hi) carries the key bits fixed so far (`prefix`) and the rank still wanted among the values
// that share them.  A round fixes OKX_ENS_SELECT_BITS more bits, from the top:
//   count   (okx_select_count):   histogram [entry][selection][bin] += accepted values whose fixed bits equal the prefix,
//                                 bin = the round's bits of the key;
//   descend (okx_select_descend): the bin that holds the rank, prefix |= bin, rank -= what lies below; histogram re-zeroed.
// Round 0 has no prefix yet: the selections of an entry share ONE histogram (selection 0's), and selection 1's first two
// counters carry the limit counts (below lo, above hi) - everything that depends on the data lives in the histogram.
//
// Count pass: as in okx_ensemble.hip a lane owns an entry and walks geometries, so a wave-instruction reads 64 consecutive
// doubles (ld == K).  A workgroup is (tile of kTile entries) x (slab of geometries); its four wavefronts interleave the
// slab's geometries.  The workgroup's histogram lives in LDS as uint32 [selection][bin][tile + 1] (the pad keeps the
// flush, which walks bins fastest, off one bank) beside the tile's prefixes, and is flushed with one 64-bit integer atomic
// add per non-zero counter, 16 consecutive counters per 128 bytes.  When a tile's histogram would not fit the LDS budget
// (many probabilities, or 8 bits per round) the tile narrows to 32, 16, ... entries and a wavefront reads that many
// consecutive doubles of 64 / tile geometries.  The slab count is a function of the sizes alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/okx.h"
#include "okx_enstable.hpp"
#include "okx_program.hpp"

namespace okx {
namespace sel {

constexpr int kBits = OKX_ENS_SELECT_BITS;
constexpr int kBins = 1 << kBits;
constexpr int kRounds = 64 / kBits;
constexpr int kThreads = 256;
constexpr int kMaxTile = 64;                // entries per workgroup: one per lane of a wavefront
constexpr long long kLdsBudget = 64 * 1024;  // bytes of LDS a workgroup may take: two workgroups and more per CU
constexpr long long kMinSlab = 16;           // geometries: below this a slab costs more in its flush than it spreads
constexpr long long kWantGroups = 1024;      // count workgroups aimed at (four per CU of a 256-CU part, from the sizes alone)
static_assert(kBits == 4 || kBits == 8, "OKX_ENS_SELECT_BITS is 4 or 8");

typedef unsigned long long u64;

// state [int64 words]: prefix [E][2Q] | rank [E][2Q] (< 0: nothing to select) | count [E] | outside [E][2]
inline long long state_words(long long n_entries, int n_sel) { return 2 * n_entries * n_sel + 3 * n_entries; }

struct State {
  u64* prefix;
  long long* rank;
  long long* count;
  long long* outside;
};

__host__ __device__ inline State state_of(void* base, long long n_entries, int n_sel) {
  State s;
  s.prefix = static_cast<u64*>(base);
  s.rank = reinterpret_cast<long long*>(s.prefix + n_entries * n_sel);
  s.count = s.rank + n_entries * n_sel;
  s.outside = s.count + n_entries;
  return s;
}

// entries per workgroup: the widest power of two whose histogram and prefixes fit the budget (0: not even one entry)
inline int tile_for(int n_sel) {
  for (int tile = kMaxTile; tile >= 1; tile >>= 1)
    if ((long long)n_sel * kBins * (tile + 1) * 4 + (long long)n_sel * tile * 8 <= kLdsBudget) return tile;
  return 0;
}

inline size_t lds_bytes(int n_sel, int tile) { return (size_t)n_sel * kBins * (tile + 1) * 4 + (size_t)n_sel * tile * 8; }

__device__ inline u64 key_of(double v) {
  const u64 b = (u64)__double_as_longlong(v);
  return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}

__device__ inline double value_of(u64 key) {
  const u64 b = (key >> 63) ? key ^ (1ull << 63) : ~key;
  return __longlong_as_double((long long)b);
}

struct CountArgs {
  const double* values;
  const unsigned char* status;
  const double* limits;     // [S][K][2] or null
  const u64* prefix;        // state: [E][n_sel]
  u64* hist;                // [E][n_sel][kBins]
  long long ld, status_stride;
  long long n_geom, steps, n_entries, slab_len;
  int n_columns, n_sel, round, tile;
};

__global__ __launch_bounds__(kThreads) void okx_select_count(CountArgs a) {
  extern __shared__ u64 sel_lds[];  // prefix [n_sel][tile] u64 | counters [n_sel][kBins][tile + 1] uint32
  const int tile = a.tile, pitch = tile + 1;
  const int n_live = a.round == 0 ? 1 : a.n_sel;  // round 0: one histogram for the entry's selections
  u64* pre = sel_lds;
  unsigned* cnt = reinterpret_cast<unsigned*>(sel_lds + (long long)a.n_sel * tile);
  const int n_cnt = n_live * kBins * pitch;
  const long long e0 = (long long)blockIdx.x * tile;
  for (int i = threadIdx.x; i < n_cnt; i += kThreads) cnt[i] = 0u;
  if (a.round > 0)
    for (int i = threadIdx.x; i < a.n_sel * tile; i += kThreads) {
      const int j = i / tile, el = i % tile;
      pre[i] = e0 + el < a.n_entries ? a.prefix[(e0 + el) * a.n_sel + j] : 0ull;
    }
  __syncthreads();
  const int el = threadIdx.x % tile;      // the entry of the tile this lane owns
  const int sub = threadIdx.x / tile;     // which of the kThreads / tile geometries in flight
  const int in_flight = kThreads / tile;
  const long long e = e0 + el;
  const bool live = e < a.n_entries;
  const long long er = live ? e : 0;  // a lane past the table walks entry 0 and counts nothing
  const long long g0 = (long long)blockIdx.y * a.slab_len;
  const long long g1 = g0 + a.slab_len < a.n_geom ? g0 + a.slab_len : a.n_geom;
  const enstable::Table t = OKX_ENS_TABLE_OF(a);
  const double* vp = enstable::entry_values(t, er);
  const unsigned char* sp = enstable::entry_status(t, er);
  const long long v_step = enstable::value_step(t), s_step = enstable::status_step(t);
  const int shift = 64 - kBits * (a.round + 1);
  const int fixed_shift = 64 - kBits * a.round;  // (round > 0) key >> fixed_shift: the bits already fixed
  const bool limited = a.round == 0 && a.limits != nullptr;
  const double lo = limited ? a.limits[2 * er] : 0.0, hi = limited ? a.limits[2 * er + 1] : 0.0;
  unsigned below = 0u, above = 0u;
  auto geometry = [&](long long g) {
    const double v = vp[g * v_step];
    const unsigned st = OKX_ENS_STATUS_AT(sp, g, s_step);
    const bool ok = live && OKX_ENS_ACCEPTED(st, v);
    if (!ok) return;
    const u64 key = key_of(v);
    const unsigned bin = (unsigned)(key >> shift) & (unsigned)(kBins - 1);
    if (a.round == 0) {
      atomicAdd(&cnt[bin * pitch + el], 1u);
      if (limited) { below += v < lo ? 1u : 0u; above += v > hi ? 1u : 0u; }
      return;
    }
    const u64 head = key >> fixed_shift;
    for (int j = 0; j < a.n_sel; ++j)
      if ((pre[j * tile + el] >> fixed_shift) == head) atomicAdd(&cnt[(j * kBins + bin) * pitch + el], 1u);
  };
#pragma unroll 4
  for (long long g = g0 + sub; g < g1; g += in_flight) geometry(g);
  __syncthreads();
  // flush: bins fastest, so 16 consecutive lanes add into 128 consecutive bytes
  const int n_flush = tile * n_live * kBins;
  for (int i = threadIdx.x; i < n_flush; i += kThreads) {
    const int bin = i % kBins, j = (i / kBins) % n_live, fe = i / (kBins * n_live);
    const unsigned c = cnt[(j * kBins + bin) * pitch + fe];
    if (c != 0u && e0 + fe < a.n_entries) atomicAdd(&a.hist[((e0 + fe) * a.n_sel + j) * kBins + bin], (u64)c);
  }
  if (limited && live) {
    u64* out = a.hist + (e * a.n_sel + 1) * kBins;
    if (below != 0u) atomicAdd(&out[0], (u64)below);
    if (above != 0u) atomicAdd(&out[1], (u64)above);
  }
}

__global__ __launch_bounds__(256) void okx_select_init(u64* state, long long state_len, u64* hist, long long hist_len) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < state_len + hist_len; i += stride) {
    if (i < state_len) state[i] = 0ull;
    else hist[i - state_len] = 0ull;
  }
}

// One thread per (entry, selection), the selections of an entry in one workgroup: all of them read before any re-zeroes.
__global__ __launch_bounds__(256) void okx_select_descend(void* state_base, u64* hist, const double* probs, long long n_entries, int n_sel,
                                                          int round, int per_block) {
  const int el = threadIdx.x / n_sel, j = threadIdx.x % n_sel;
  const long long e = (long long)blockIdx.x * per_block + el;
  const bool live = el < per_block && e < n_entries;
  const State st = state_of(state_base, n_entries, n_sel);
  if (live) {
    const long long at = e * n_sel + j;
    const u64* h = hist + (e * n_sel + (round == 0 ? 0 : j)) * kBins;
    long long rank;
    if (round == 0) {
      long long n = 0;
      for (int b = 0; b < kBins; ++b) n += (long long)h[b];
      const double p = probs[j >> 1];
      rank = -1;
      if (n > 0 && p >= 0.0 && p <= 1.0) {
        const double at_h = (double)(n - 1) * p;  // fp64, one rounding: NumPy's (n - 1) * p
        rank = (long long)((j & 1) ? ceil(at_h) : floor(at_h));
        if (rank > n - 1) rank = n - 1;
      }
      if (j == 0) st.count[e] = n;
      if (j == 1) {
        const u64* o = hist + (e * n_sel + 1) * kBins;
        st.outside[2 * e] = (long long)o[0];
        st.outside[2 * e + 1] = (long long)o[1];
      }
    } else {
      rank = st.rank[at];
    }
    if (rank >= 0) {
      long long below = 0;
      int pick = -1;
      for (int b = 0; b < kBins; ++b) {
        const long long c = (long long)h[b];
        if (pick < 0 && rank < below + c) pick = b;
        if (pick < 0) below += c;
      }
      if (pick < 0) rank = -1;  // (counts that do not hold the rank: a histogram that is not this state's)
      else {
        rank -= below;
        st.prefix[at] = (round == 0 ? 0ull : st.prefix[at]) | ((u64)pick << (64 - kBits * (round + 1)));
      }
    }
    st.rank[at] = rank;
  }
  __syncthreads();
  if (live) {
    u64* mine = hist + (e * n_sel + j) * kBins;
    for (int b = 0; b < kBins; ++b) mine[b] = 0ull;
  }
}

__global__ __launch_bounds__(256) void okx_select_finish(const void* state_base, long long n_entries, int n_sel, double* order, long long* count,
                                                         long long* outside) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_entries * n_sel) return;
  const State st = state_of(const_cast<void*>(state_base), n_entries, n_sel);
  order[t] = st.rank[t] >= 0 ? value_of(st.prefix[t]) : __builtin_nan("");
  const long long e = t / n_sel;
  if (t % n_sel == 0) count[e] = st.count[e];
  if (t % n_sel == 1 && outside) { outside[2 * e] = st.outside[2 * e]; outside[2 * e + 1] = st.outside[2 * e + 1]; }
}

inline int check_sizes(const char* who, long long steps, int n_columns, int n_probs) {
  if (steps < 0 || n_columns < 0) return fail(OKX_ERR_INVALID, "%s: negative step or column count", who);
  if (n_probs < 1 || n_probs > OKX_ENS_SELECT_MAX_PROBS || tile_for(2 * n_probs) < 1)
    return fail(OKX_ERR_LIMIT, "%s: 1 to %d probabilities", who, OKX_ENS_SELECT_MAX_PROBS);
  return enstable::check_entries(who, steps, n_columns, (1ll << 38) / (2ll * n_probs * kBins));
}

}  // namespace sel
}  // namespace okx

using okx::fail;
namespace et = okx::enstable;

extern "C" {

int32_t okx_ensemble_select_rounds(void) { return okx::sel::kRounds; }

int64_t okx_ensemble_select_hist_len(int64_t steps, int32_t n_columns, int32_t n_probs) {
  if (steps <= 0 || n_columns <= 0 || n_probs <= 0) return 0;
  return (int64_t)steps * n_columns * 2 * n_probs * okx::sel::kBins;
}

size_t okx_ensemble_select_state_bytes(int64_t steps, int32_t n_columns, int32_t n_probs) {
  if (steps <= 0 || n_columns <= 0 || n_probs <= 0) return 0;
  return sizeof(int64_t) * (size_t)okx::sel::state_words((long long)steps * n_columns, 2 * n_probs);
}

size_t okx_ensemble_select_scratch_bytes(int64_t steps, int32_t n_columns, int32_t n_probs) {
  return okx_ensemble_select_state_bytes(steps, n_columns, n_probs) +
         sizeof(int64_t) * (size_t)okx_ensemble_select_hist_len(steps, n_columns, n_probs);
}

int32_t okx_ensemble_select_check(const double* probs, int32_t n_probs, const double* limits, int64_t n_limits) {
  if (n_probs < 1 || n_probs > OKX_ENS_SELECT_MAX_PROBS)
    return fail(OKX_ERR_LIMIT, "okx_ensemble_select: 1 to %d probabilities", OKX_ENS_SELECT_MAX_PROBS);
  if (!probs || n_limits < 0 || (n_limits > 0 && !limits)) return fail(OKX_ERR_INVALID, "okx_ensemble_select: null probabilities or limits");
  for (int32_t q = 0; q < n_probs; ++q)
    if (!(probs[q] >= 0.0 && probs[q] <= 1.0))
      return fail(OKX_ERR_INVALID, "okx_ensemble_select: probability %d is %g, outside [0, 1]", (int)q, probs[q]);
  return et::check_limits("okx_ensemble_select", limits, n_limits);
}

int32_t okx_ensemble_select_begin(int64_t steps, int32_t n_columns, int32_t n_probs, void* d_state, int64_t* d_hist, void* stream) {
  namespace sl = okx::sel;
  if (int rc = sl::check_sizes("okx_ensemble_select_begin", steps, n_columns, n_probs)) return rc;
  const long long n_entries = (long long)steps * n_columns;
  if (n_entries == 0) return OKX_OK;
  if (!d_state || !d_hist) return fail(OKX_ERR_INVALID, "okx_ensemble_select_begin: null state or histogram");
  const long long state_len = sl::state_words(n_entries, 2 * n_probs), hist_len = okx_ensemble_select_hist_len(steps, n_columns, n_probs);
  const long long blocks = (state_len + hist_len + 255) / 256;
  OKX_LAUNCH(sl::okx_select_init, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream,
             static_cast<sl::u64*>(d_state), state_len, reinterpret_cast<sl::u64*>(d_hist), hist_len);
  return OKX_OK;
}

int32_t okx_ensemble_select_count(int32_t round, int64_t n_geometries, int64_t steps, int32_t n_columns, const double* d_values, int64_t ld,
                                  const uint8_t* d_status, int64_t status_stride, int32_t n_probs, const double* d_limits,
                                  const void* d_state, int64_t* d_hist, void* stream) {
  namespace sl = okx::sel;
  if (int rc = sl::check_sizes("okx_ensemble_select_count", steps, n_columns, n_probs)) return rc;
  if (round < 0 || round >= sl::kRounds) return fail(OKX_ERR_INVALID, "okx_ensemble_select_count: round %d of %d", (int)round, sl::kRounds);
  if (n_geometries < 0) return fail(OKX_ERR_INVALID, "okx_ensemble_select_count: negative geometry count");
  const long long n_entries = (long long)steps * n_columns;
  if (n_entries == 0 || n_geometries == 0) return OKX_OK;
  if (!d_state || !d_hist) return fail(OKX_ERR_INVALID, "okx_ensemble_select_count: null state or histogram");
  if (int rc = et::check_table("okx_ensemble_select_count", true, d_values, ld, n_columns, d_status, status_stride)) return rc;
  const int n_sel = 2 * n_probs, tile = sl::tile_for(n_sel);
  long long n_slabs, slab_len;
  et::slab_plan(n_geometries, n_entries, tile, sl::kWantGroups, sl::kMinSlab, 65535, &n_slabs, &slab_len);  // from the sizes alone
  const long long tiles = (n_entries + tile - 1) / tile;
  if (tiles > 0x7fffffffll) return fail(OKX_ERR_LIMIT, "okx_ensemble_select_count: too many entries for one call");
  sl::CountArgs a{};
  et::set_table(&a, et::table_view(d_values, ld, d_status, status_stride, n_geometries, steps, n_columns));
  a.limits = d_limits;
  a.prefix = sl::state_of(const_cast<void*>(d_state), n_entries, n_sel).prefix;
  a.hist = reinterpret_cast<sl::u64*>(d_hist);
  a.n_entries = n_entries; a.slab_len = slab_len; a.n_sel = n_sel; a.round = round; a.tile = tile;
  OKX_LAUNCH(sl::okx_select_count, dim3((unsigned)tiles, (unsigned)n_slabs), dim3(sl::kThreads), sl::lds_bytes(n_sel, tile), (hipStream_t)stream, a);
  return OKX_OK;
}

int32_t okx_ensemble_select_descend(int32_t round, int64_t steps, int32_t n_columns, const double* d_probs, int32_t n_probs, void* d_state,
                                    int64_t* d_hist, void* stream) {
  namespace sl = okx::sel;
  if (int rc = sl::check_sizes("okx_ensemble_select_descend", steps, n_columns, n_probs)) return rc;
  if (round < 0 || round >= sl::kRounds) return fail(OKX_ERR_INVALID, "okx_ensemble_select_descend: round %d of %d", (int)round, sl::kRounds);
  const long long n_entries = (long long)steps * n_columns;
  if (n_entries == 0) return OKX_OK;
  if (!d_state || !d_hist || !d_probs) return fail(OKX_ERR_INVALID, "okx_ensemble_select_descend: null state, histogram or probabilities");
  const int n_sel = 2 * n_probs, per_block = 256 / n_sel;
  OKX_LAUNCH(sl::okx_select_descend, dim3((unsigned)((n_entries + per_block - 1) / per_block)), dim3(256), 0, (hipStream_t)stream, d_state,
             reinterpret_cast<sl::u64*>(d_hist), d_probs, n_entries, n_sel, (int)round, per_block);
  return OKX_OK;
}

int32_t okx_ensemble_select_finish(int64_t steps, int32_t n_columns, int32_t n_probs, const void* d_state, double* d_order, int64_t* d_count,
                                   int64_t* d_outside, void* stream) {
  namespace sl = okx::sel;
  if (int rc = sl::check_sizes("okx_ensemble_select_finish", steps, n_columns, n_probs)) return rc;
  const long long n_entries = (long long)steps * n_columns;
  if (n_entries == 0) return OKX_OK;
  if (!d_state) return fail(OKX_ERR_INVALID, "okx_ensemble_select_finish: null state");
  if (!d_order || !d_count) return fail(OKX_ERR_INVALID, "okx_ensemble_select_finish: null order-statistic or count table");
  const long long threads = n_entries * 2 * n_probs;
  OKX_LAUNCH(sl::okx_select_finish, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_state, n_entries, 2 * n_probs,
             d_order, reinterpret_cast<long long*>(d_count), reinterpret_cast<long long*>(d_outside));
  return OKX_OK;
}

int32_t okx_ensemble_select(int64_t n_geometries, int64_t steps, int32_t n_columns, const double* d_values, int64_t ld, const uint8_t* d_status,
                            int64_t status_stride, const double* d_probs, int32_t n_probs, const double* d_limits, double* d_order,
                            int64_t* d_count, int64_t* d_outside, void* d_scratch, size_t scratch_bytes, void* stream) {
  namespace sl = okx::sel;
  if (int rc = sl::check_sizes("okx_ensemble_select", steps, n_columns, n_probs)) return rc;
  if (n_geometries < 0) return fail(OKX_ERR_INVALID, "okx_ensemble_select: negative geometry count");
  const long long n_entries = (long long)steps * n_columns;
  if (n_entries == 0) return OKX_OK;
  if (!d_order || !d_count) return fail(OKX_ERR_INVALID, "okx_ensemble_select: null order-statistic or count table");
  if (!d_probs) return fail(OKX_ERR_INVALID, "okx_ensemble_select: null probabilities");
  if (d_outside && !d_limits) return fail(OKX_ERR_INVALID, "okx_ensemble_select: limit counts asked for without limits");
  if (int rc = et::check_table("okx_ensemble_select", n_geometries > 0, d_values, ld, n_columns, d_status, status_stride)) return rc;
  const size_t need = okx_ensemble_select_scratch_bytes(steps, n_columns, n_probs);
  if (int rc = et::check_scratch("okx_ensemble_select", "okx_ensemble_select_scratch_bytes", need, d_scratch, scratch_bytes)) return rc;
  void* state = d_scratch;
  int64_t* hist = reinterpret_cast<int64_t*>(static_cast<char*>(d_scratch) + okx_ensemble_select_state_bytes(steps, n_columns, n_probs));
  if (int rc = okx_ensemble_select_begin(steps, n_columns, n_probs, state, hist, stream)) return rc;
  for (int round = 0; round < sl::kRounds; ++round) {
    if (int rc = okx_ensemble_select_count(round, n_geometries, steps, n_columns, d_values, ld, d_status, status_stride, n_probs, d_limits,
                                           state, hist, stream))
      return rc;
    if (int rc = okx_ensemble_select_descend(round, steps, n_columns, d_probs, n_probs, state, hist, stream)) return rc;
  }
  return okx_ensemble_select_finish(steps, n_columns, n_probs, state, d_order, d_count, d_outside, stream);
}

}  // extern "C"
