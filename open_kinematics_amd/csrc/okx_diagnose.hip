// Sweep diagnostics on solved records (okx_diagnose_sweeps_batch, include/okx.h): the reference's diagnose_sweep
// (core/diagnostics.py:114-226, axle/mechanisms.py:119-163, 432-549) for batches of sweeps, fp64 throughout.
//
// One wavefront walks a run of consecutive states of one sweep.  Its lanes read consecutive doubles of a state's record
// (coalesced: a batch of up to 8 records is one contiguous block, up to 8 independent loads per lane, the next batch in
// flight while this one is worked on) into wave-private LDS slots; the last state of a batch stays as the one in front of
// the next, so every state is fetched once per wavefront that owns it (plus one re-read of the state before the run, from
// L2).  From the slots lane j takes the step displacement of tracked point j, lanes 48..55 the U-bar checks (side =
// lane & 1: chirality and the three transmission joints), lanes 56..63 the batch's solver records.  The displacements go to a [point][step] array:
// in LDS when a whole sweep fits one workgroup (okx_diagnose_short: state pass and selection in one launch), else in a
// scratch buffer in global memory (okx_diagnose_states, then okx_diagnose_select with one wavefront per sweep and point).
// The median of the positive displacements is exact: positive doubles order like their bit patterns, so a bisection over
// the 63 value bits with wavefront ballots finds the lower middle order statistic, one more pass the upper one; only
// (a + b) / 2 is arithmetic.  Both paths run the same two device functions, so their records are bit-identical.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstddef>

#include "../../include/okx.h"
#include "okx_program.hpp"

namespace okx {
namespace diag {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTracked = OKX_MAX_VARS / 3;
constexpr int kLoads = 8;                               // doubles of a batch of states per lane: batch * rowd <= 512
constexpr int kLongChunk = 64;                          // states per wavefront on the long path
constexpr double kEpsGeometric = 1e-6;
constexpr double kJumpFloor = 5.0, kJumpFactor = 4.0, kTransmissionWarning = 0.15;

// A role point: ref >= 0 is its first double inside a state's record, ref < 0 a fixed point -(ref + 1) of the design table.
struct SideRefs {
  int rocker, arm, axis_a, axis_b, push_in, push_out;  // refs
  int rocker_pt, arm_pt;                               // program points (design volume)
  int has_rocker, pad;
};

struct DiagArgs {
  const double* pos;
  const okx_info* info;
  const double* design;      // [P][3] of the program, or [n_sweeps][P][3]
  long long design_stride;   // 0, or 3 P
  okx_diag_summary* summary;
  okx_diag_issue* issues;
  long long capacity;
  unsigned long long* count;
  double* disp;              // long path: [n_sweeps][n_points][steps - 1]
  long long n_sweeps, steps;
  double residual_tolerance;
  int rowd, n_points, n_sides, bar_a, bar_b;
  int batch;                 // states per LDS batch of a wavefront: max(1, min(8, 512 / rowd))
  int pt_off[kTracked];
  SideRefs side[2];
};

__device__ inline double wave_fmax(double v) {
  for (int m = 32; m > 0; m >>= 1) v = fmax(v, __shfl_xor(v, m));
  return v;
}
__device__ inline double wave_fmin(double v) {
  for (int m = 32; m > 0; m >>= 1) v = fmin(v, __shfl_xor(v, m));
  return v;
}

__device__ inline void emit(const DiagArgs& a, long long sweep, int step, int category, int subject, double value, double threshold) {
  const unsigned long long at = atomicAdd(a.count, 1ull);
  if (a.issues && at < (unsigned long long)a.capacity) {
    okx_diag_issue r;
    r.sweep = sweep; r.step = step; r.category = category; r.subject = subject; r.reserved = 0;
    r.value = value; r.threshold = threshold;
    a.issues[at] = r;
  }
  atomicAdd(&a.summary[sweep].n_issues[category], 1);
  atomicMin(reinterpret_cast<unsigned int*>(&a.summary[sweep].first_step[category]), (unsigned int)step);
}

// worst[] holds non-negative doubles (or +inf): they order like their bit patterns
__device__ inline void worst_max(const DiagArgs& a, long long sweep, int category, double v) {
  atomicMax(reinterpret_cast<unsigned long long*>(&a.summary[sweep].worst[category]), (unsigned long long)__double_as_longlong(v));
}
__device__ inline void worst_min(const DiagArgs& a, long long sweep, int category, double v) {
  atomicMin(reinterpret_cast<unsigned long long*>(&a.summary[sweep].worst[category]), (unsigned long long)__double_as_longlong(v));
}

__device__ inline void role_point(int ref, const volatile double* rec, const double* design, double out[3]) {
  if (ref >= 0) { out[0] = rec[ref]; out[1] = rec[ref + 1]; out[2] = rec[ref + 2]; }
  else { const double* q = design + 3 * (-(ref + 1)); out[0] = q[0]; out[1] = q[1]; out[2] = q[2]; }
}
__device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ inline double norm3(const double* a) { return sqrt(dot3(a, a)); }
__device__ inline void sub3(const double* a, const double* b, double* o) { o[0] = a[0] - b[0]; o[1] = a[1] - b[1]; o[2] = a[2] - b[2]; }
__device__ inline void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ inline double triple3(const double* a, const double* b, const double* c) { double t[3]; cross3(b, c, t); return dot3(a, t); }
__device__ inline int sign_of(double v) { return (v > 0.0) - (v < 0.0); }

// calculate_transmission_margin (mechanisms.py:145-163); false: undefined
__device__ inline bool transmission_margin(const double* driven, const double* axis_point, const double* axis, const double* link,
                                           double* margin) {
  const double axis_norm = norm3(axis), link_norm = norm3(link);
  if (axis_norm == 0.0 || link_norm == 0.0) return false;
  const double u[3] = {axis[0] / axis_norm, axis[1] / axis_norm, axis[2] / axis_norm};
  double radius[3];
  sub3(driven, axis_point, radius);
  const double along = dot3(radius, u);
  radius[0] -= u[0] * along; radius[1] -= u[1] * along; radius[2] -= u[2] * along;
  double tangent[3];
  cross3(u, radius, tangent);
  const double tangent_norm = norm3(tangent);
  if (tangent_norm == 0.0) return false;
  const double l[3] = {link[0] / link_norm, link[1] / link_norm, link[2] / link_norm};
  const double t[3] = {tangent[0] / tangent_norm, tangent[1] / tangent_norm, tangent[2] / tangent_norm};
  *margin = fabs(dot3(l, t));
  return true;
}

// States [s_begin, s_end) of one sweep by one wavefront.  slots: this wavefront's [batch + 1][rowd] doubles of LDS.
// disp: [n_points][steps - 1] of this sweep (LDS or global).
__device__ inline void state_pass(const DiagArgs& a, long long sweep, long long s_begin, long long s_end, volatile double* slots,
                                  double* disp) {
  if (s_begin >= s_end) return;
  const int lane = threadIdx.x & 63;
  const int rowd = a.rowd;
  const long long steps = a.steps;
  const double* base = a.pos + sweep * steps * rowd;
  const double* design = a.design + sweep * a.design_stride;
  // LDS of this wavefront: slot 0 holds the state in front of the batch, slots 1..batch the batch itself
  const int batch = a.batch;
  if (s_begin > 0)
    for (int k = lane; k < rowd; k += 64) slots[k] = base[(s_begin - 1) * rowd + k];
  double next[kLoads];  // the next batch, in flight while this one is worked on (batch * rowd <= 64 * kLoads)
  {
    const long long count = (s_end - s_begin < batch ? s_end - s_begin : batch) * rowd;
#pragma unroll
    for (int q = 0; q < kLoads; ++q) {
      const int k = q * 64 + lane;
      next[q] = k < count ? base[s_begin * rowd + k] : 0.0;
    }
  }
  const int job = lane - 48;  // lanes 48..55: side = job & 1, what = job >> 1 (0 chirality, 1..3 transmission joint 0..2)
  const bool side_lane = job >= 0 && job < 8 && (job & 1) < a.n_sides;
  const int side = job & 1, what = job >> 1;
  double bar_a[3] = {0, 0, 0}, bar_axis[3] = {0, 0, 0}, bar_len = 0.0;
  int design_sign = 0;
  if (side_lane) {
    const SideRefs& r = a.side[side];
    double b[3], dr[3], du[3], t0[3], t1[3];
    role_point(-(a.bar_a + 1), nullptr, design, bar_a);
    role_point(-(a.bar_b + 1), nullptr, design, b);
    sub3(b, bar_a, bar_axis);
    bar_len = norm3(bar_axis);
    role_point(-(r.rocker_pt + 1), nullptr, design, dr);
    role_point(-(r.arm_pt + 1), nullptr, design, du);
    sub3(dr, bar_a, t0);
    sub3(du, bar_a, t1);
    design_sign = sign_of(triple3(bar_axis, t0, t1));
  }
  double max_jump = 0.0, max_residual = 0.0, min_chirality = __builtin_inf(), min_transmission = __builtin_inf();
  for (long long b0 = s_begin; b0 < s_end; b0 += batch) {
    const int nb = (int)(s_end - b0 < batch ? s_end - b0 : batch);
#pragma unroll
    for (int q = 0; q < kLoads; ++q) {
      const int k = q * 64 + lane;
      if (k < nb * rowd) slots[rowd + k] = next[q];
    }
    if (b0 + batch < s_end) {
      const long long left = s_end - (b0 + batch);
      const long long count = (left < batch ? left : batch) * rowd;
#pragma unroll
      for (int q = 0; q < kLoads; ++q) {
        const int k = q * 64 + lane;
        if (k < count) next[q] = base[(b0 + batch) * rowd + k];
      }
    }
    // (the slots are this wavefront's own and its LDS operations complete in order; the fence and the wave barrier say
    //  so to the compiler - no read of another lane's element moves above the writes - and the volatile accesses keep it
    //  from caching a slot element in a register across iterations)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (a.info && lane >= 56 && lane - 56 < nb) {  // the batch's solver records, one lane each
      const long long s = b0 + (lane - 56);
      const okx_info& info = a.info[sweep * steps + s];
      if (!(info.flags & 1)) emit(a, sweep, (int)s, OKX_DIAG_CONVERGENCE, 0, 0.0, 0.0);
      if (info.max_residual > a.residual_tolerance) emit(a, sweep, (int)s, OKX_DIAG_RESIDUAL, 0, info.max_residual, a.residual_tolerance);
      max_residual = fmax(max_residual, info.max_residual);
    }
    for (int i = 0; i < nb; ++i) {
    const long long s = b0 + i;
    const volatile double* cur = slots + (i + 1) * rowd;
    const volatile double* prv = slots + i * rowd;
    if (lane < a.n_points) {
      if (s > 0) {
        const int o = a.pt_off[lane];
        const double dx = cur[o] - prv[o], dy = cur[o + 1] - prv[o + 1], dz = cur[o + 2] - prv[o + 2];
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        disp[(long long)lane * (steps - 1) + (s - 1)] = d;
        max_jump = fmax(max_jump, d);
      }
    } else if (side_lane) {
      const SideRefs& r = a.side[side];
      double rocker[3], arm[3];
      role_point(r.rocker, cur, design, rocker);
      role_point(r.arm, cur, design, arm);
      if (what == 0) {
        double ra[3], ua[3];
        sub3(rocker, bar_a, ra);
        sub3(arm, bar_a, ua);
        const double volume = triple3(bar_axis, ra, ua);
        const double scale = bar_len * norm3(ra) * norm3(ua);
        const double margin = scale <= kEpsGeometric ? 0.0 : volume / scale;
        if (fabs(margin) <= kEpsGeometric) emit(a, sweep, (int)s, OKX_DIAG_CHIRALITY, side | 2, margin, kEpsGeometric);
        else if (volume != volume || sign_of(volume) != design_sign) emit(a, sweep, (int)s, OKX_DIAG_CHIRALITY, side, volume, 0.0);
        min_chirality = fmin(min_chirality, fabs(margin));
      } else if (what == 1 || r.has_rocker) {
        double link[3], margin = 0.0;
        bool defined;
        sub3(arm, rocker, link);
        if (what == 1) {
          defined = transmission_margin(arm, bar_a, bar_axis, link, &margin);
        } else {
          double xa[3], xb[3], axis[3];
          role_point(r.axis_a, cur, design, xa);
          role_point(r.axis_b, cur, design, xb);
          sub3(xb, xa, axis);
          if (what == 2) {
            double pi[3], po[3];
            role_point(r.push_in, cur, design, pi);
            role_point(r.push_out, cur, design, po);
            sub3(po, pi, link);
            defined = transmission_margin(pi, xa, axis, link, &margin);
          } else {
            defined = transmission_margin(rocker, xa, axis, link, &margin);
          }
        }
        if (defined) {
          if (margin < kTransmissionWarning) emit(a, sweep, (int)s, OKX_DIAG_TRANSMISSION, side | ((what - 1) << 1), margin, kTransmissionWarning);
          min_transmission = fmin(min_transmission, margin);
        }
      }
    }
    }
    // the batch's last state becomes the one in front of the next batch
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int k = lane; k < rowd; k += 64) slots[k] = slots[nb * rowd + k];
  }
  max_jump = wave_fmax(max_jump);
  max_residual = wave_fmax(max_residual);
  min_chirality = wave_fmin(min_chirality);
  min_transmission = wave_fmin(min_transmission);
  if (lane == 0) {
    if (max_jump > 0.0) worst_max(a, sweep, OKX_DIAG_JUMP, max_jump);
    if (max_residual > 0.0) worst_max(a, sweep, OKX_DIAG_RESIDUAL, max_residual);
    if (min_chirality < __builtin_inf()) worst_min(a, sweep, OKX_DIAG_CHIRALITY, min_chirality);
    if (min_transmission < __builtin_inf()) worst_min(a, sweep, OKX_DIAG_TRANSMISSION, min_transmission);
  }
}

// The jumps of tracked point j of one sweep from its n step displacements d[], by one wavefront.
__device__ inline void select_pass(const DiagArgs& a, long long sweep, int j, const double* d, long long n) {
  const int lane = threadIdx.x & 63;
  long long k = 0;
  for (long long i0 = 0; i0 < n; i0 += 64) {
    const long long i = i0 + lane;
    k += __popcll(__ballot(i < n && d[i] > 0.0));
  }
  double typical = 0.0;
  if (k > 0) {
    long long r = (k - 1) / 2;
    unsigned long long prefix = 0;
    for (int bit = 62; bit >= 0; --bit) {
      const unsigned long long mask = ~((1ull << bit) - 1ull);
      long long c = 0;  // candidates whose next bit is 0
      for (long long i0 = 0; i0 < n; i0 += 64) {
        const long long i = i0 + lane;
        const double v = i < n ? d[i] : 0.0;
        c += __popcll(__ballot(v > 0.0 && ((unsigned long long)__double_as_longlong(v) & mask) == prefix));
      }
      if (r >= c) { r -= c; prefix |= 1ull << bit; }
    }
    const double lower = __longlong_as_double((long long)prefix);
    double upper = lower;
    if (k / 2 != (k - 1) / 2) {  // even count: the next order statistic
      long long not_above = 0;
      double above = __builtin_inf();
      for (long long i0 = 0; i0 < n; i0 += 64) {
        const long long i = i0 + lane;
        const double v = i < n ? d[i] : 0.0;
        not_above += __popcll(__ballot(v > 0.0 && v <= lower));
        if (v > lower) above = fmin(above, v);
      }
      if (not_above <= k / 2) upper = wave_fmin(above);
    }
    typical = (lower + upper) / 2.0;
  }
  const double threshold = fmax(kJumpFloor, kJumpFactor * typical);
  for (long long i0 = 0; i0 < n; i0 += 64) {
    const long long i = i0 + lane;
    if (i < n && !(d[i] <= threshold)) emit(a, sweep, (int)(i + 1), OKX_DIAG_JUMP, j, d[i], threshold);
  }
}

__global__ void okx_diagnose_init(okx_diag_summary* summary, long long n_sweeps, unsigned long long* count) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) *count = 0ull;
  if (g >= n_sweeps) return;
  okx_diag_summary s;
  for (int c = 0; c < 5; ++c) { s.n_issues[c] = 0; s.first_step[c] = -1; s.worst[c] = c >= OKX_DIAG_CHIRALITY ? __builtin_inf() : 0.0; }
  summary[g] = s;
}

// One workgroup per sweep: displacements [n_points][steps - 1] in LDS, then the wavefronts share the points.
__global__ __launch_bounds__(kThreads) void okx_diagnose_short(DiagArgs a) {
  extern __shared__ double diag_lds[];
  const int wave = threadIdx.x >> 6;
  double* disp = diag_lds;
  volatile double* slots = diag_lds + (long long)a.n_points * (a.steps - 1) + wave * (a.batch + 1) * a.rowd;
  const long long chunk = (a.steps + kWaves - 1) / kWaves;
  for (long long sweep = blockIdx.x; sweep < a.n_sweeps; sweep += gridDim.x) {
    const long long s_begin = wave * chunk;
    const long long s_end = s_begin + chunk < a.steps ? s_begin + chunk : a.steps;
    state_pass(a, sweep, s_begin, s_end, slots, disp);
    __syncthreads();
    for (int j = wave; j < a.n_points; j += kWaves) select_pass(a, sweep, j, disp + (long long)j * (a.steps - 1), a.steps - 1);
    __syncthreads();
  }
}

// Long sweeps, first launch: a workgroup per tile of kWaves * kLongChunk states of one sweep; displacements to global memory.
__global__ __launch_bounds__(kThreads) void okx_diagnose_states(DiagArgs a, long long tiles_per_sweep) {
  extern __shared__ double diag_lds[];
  const int wave = threadIdx.x >> 6;
  volatile double* slots = diag_lds + wave * (a.batch + 1) * a.rowd;
  const long long n_tiles = tiles_per_sweep * a.n_sweeps;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long sweep = tile / tiles_per_sweep;
    const long long s_begin = ((tile % tiles_per_sweep) * kWaves + wave) * kLongChunk;
    const long long s_end = s_begin + kLongChunk < a.steps ? s_begin + kLongChunk : a.steps;
    state_pass(a, sweep, s_begin, s_end, slots, a.disp + sweep * a.n_points * (a.steps - 1));
  }
}

// Long sweeps, second launch: one wavefront per (sweep, tracked point).
__global__ __launch_bounds__(64) void okx_diagnose_select(DiagArgs a) {
  const long long n_jobs = a.n_sweeps * a.n_points;
  for (long long job = blockIdx.x; job < n_jobs; job += gridDim.x) {
    const long long sweep = job / a.n_points;
    const int j = (int)(job % a.n_points);
    select_pass(a, sweep, j, a.disp + job * (a.steps - 1), a.steps - 1);
  }
}

}  // namespace diag
}  // namespace okx

using okx::fail;

extern "C" {

static_assert(sizeof(okx_diag_roles) == 232 && sizeof(okx_diag_summary) == 80 && sizeof(okx_diag_issue) == 40,
              "the okx_diag_* layouts are part of the ABI (ctypes / NumPy mirrors in diagnostics.py)");

/* The program's grow-only displacement scratch of okx_diagnose_sweeps_batch (long sweeps), at least `need` doubles. */
static int32_t diag_scratch(okx_program* p, long long need, long long steps_per_sweep, hipStream_t st, double** disp) {
  std::lock_guard<std::mutex> lock(p->head_mutex);
  if (need > p->diag_scratch_len) {
    if (okx::stream_is_capturing(st))
      return fail(OKX_ERR_INVALID, "okx_diagnose_sweeps_batch: sweeps of %lld steps need a scratch buffer; run this shape once outside the stream capture first", steps_per_sweep);
    if (p->diag_scratch) {  // replaced in stream order, like the geometry-table scratch of the solve
      double* old = p->diag_scratch;
      p->diag_scratch = nullptr;
      p->diag_scratch_len = 0;
      HIP_TRY(hipFreeAsync(old, st));
    }
    double* fresh = nullptr;
    HIP_TRY(hipMallocAsync((void**)&fresh, sizeof(double) * (size_t)need, st));
    p->diag_scratch = fresh;
    p->diag_scratch_len = need;
  }
  *disp = p->diag_scratch;
  return OKX_OK;
}

int32_t okx_diagnose_sweeps_batch(okx_program* p, const okx_diag_roles* roles, int64_t n_sweeps, int64_t steps_per_sweep,
                                  int32_t layout, const double* d_pos, const okx_info* d_info, const double* d_geom_pos,
                                  double residual_tolerance, okx_diag_summary* d_summary, okx_diag_issue* d_issues,
                                  int64_t capacity, int64_t* d_issue_count, void* stream) {
  namespace dg = okx::diag;
  if (!p || !roles) return fail(OKX_ERR_INVALID, "null program or roles");
  if (n_sweeps < 0 || steps_per_sweep < 1) return fail(OKX_ERR_INVALID, "bad sweep count or steps_per_sweep");
  if (layout != OKX_OUTPUT_RECORDS && layout != OKX_OUTPUT_FREE) return fail(OKX_ERR_INVALID, "layout must be OKX_OUTPUT_RECORDS or OKX_OUTPUT_FREE");
  if (!d_issue_count || capacity < 0 || (capacity > 0 && !d_issues)) return fail(OKX_ERR_INVALID, "null issue count / issue buffer");
  if (n_sweeps > 0 && (!d_pos || !d_summary)) return fail(OKX_ERR_INVALID, "null pointer");
  if (steps_per_sweep > 0x7fffffffll || n_sweeps > 0x7fffffffll) return fail(OKX_ERR_LIMIT, "too many sweeps or steps for one launch");
  const okx::DevProgram& h = p->host;
  if (roles->n_points < 0 || roles->n_points > dg::kTracked) return fail(OKX_ERR_LIMIT, "at most %d tracked points", dg::kTracked);
  if (roles->n_sides != 0 && roles->n_sides != 2) return fail(OKX_ERR_INVALID, "n_sides must be 0 or 2");
  const int n_rows = layout == OKX_OUTPUT_RECORDS ? h.n_out : h.n_free;
  const int32_t* rows = layout == OKX_OUTPUT_RECORDS ? h.out_point : h.free_point;
  if (n_rows < 1) return fail(OKX_ERR_INVALID, "the layout carries no point");
  auto row_of = [&](int point) { for (int k = 0; k < n_rows; ++k) if (rows[k] == point) return k; return -1; };
  auto moving = [&](int point) {
    for (int k = 0; k < h.n_free; ++k) if (h.free_point[k] == point) return true;
    for (int k = 0; k < h.n_derived; ++k) if (h.dop_out[k] == point) return true;
    return false;
  };
  int bad = 0;
  // a role point's reference: its first double in a record, or -(point + 1) for a fixed point the layout leaves out
  auto ref_of = [&](int point, const char* what) {
    if (point < 0 || point >= h.n_points) { if (!bad) { bad = 1; fail(OKX_ERR_INVALID, "%s: point index %d out of range", what, point); } return 0; }
    const int row = row_of(point);
    if (row >= 0) return 3 * row;
    if (moving(point)) { if (!bad) { bad = 1; fail(OKX_ERR_INVALID, "%s: moving point %d is not part of the %s layout", what, point, layout == OKX_OUTPUT_RECORDS ? "records" : "free-point"); } return 0; }
    return -(point + 1);
  };
  dg::DiagArgs a{};
  a.pos = d_pos;
  a.info = d_info;
  a.summary = d_summary;
  a.issues = capacity > 0 ? d_issues : nullptr;
  a.capacity = capacity;
  a.count = reinterpret_cast<unsigned long long*>(d_issue_count);
  a.n_sweeps = n_sweeps;
  a.steps = steps_per_sweep;
  a.residual_tolerance = residual_tolerance;
  a.rowd = 3 * n_rows;
  a.batch = 512 / a.rowd < 1 ? 1 : (512 / a.rowd > 8 ? 8 : 512 / a.rowd);
  a.n_points = roles->n_points;
  a.n_sides = roles->n_sides;
  if (d_geom_pos) {
    a.design = d_geom_pos;
    a.design_stride = 3ll * h.n_points;
  } else {
    a.design = reinterpret_cast<const double*>(reinterpret_cast<const char*>(p->dev) + offsetof(okx::DevProgram, design_pos));
    a.design_stride = 0;
  }
  for (int k = 0; k < roles->n_points; ++k) {
    const int ref = ref_of(roles->point[k], "tracked point");
    if (!bad && ref < 0) { bad = 1; fail(OKX_ERR_INVALID, "tracked point %d is a fixed point", roles->point[k]); }
    a.pt_off[k] = ref;
  }
  for (int s = 0; s < roles->n_sides && !bad; ++s) {
    const okx_diag_side& r = roles->side[s];
    dg::SideRefs& o = a.side[s];
    o.rocker = ref_of(r.droplink_rocker, "droplink_rocker");
    o.arm = ref_of(r.droplink_u_bar, "droplink_u_bar");
    o.rocker_pt = r.droplink_rocker;
    o.arm_pt = r.droplink_u_bar;
    o.has_rocker = r.rocker_axis_a >= 0 && r.rocker_axis_b >= 0 && r.pushrod_inboard >= 0 && r.pushrod_outboard >= 0;
    if (o.has_rocker) {
      o.axis_a = ref_of(r.rocker_axis_a, "rocker_axis_a");
      o.axis_b = ref_of(r.rocker_axis_b, "rocker_axis_b");
      o.push_in = ref_of(r.pushrod_inboard, "pushrod_inboard");
      o.push_out = ref_of(r.pushrod_outboard, "pushrod_outboard");
    }
  }
  if (roles->n_sides && !bad) {
    if (roles->bar_axis_a < 0 || roles->bar_axis_a >= h.n_points || roles->bar_axis_b < 0 || roles->bar_axis_b >= h.n_points)
      return fail(OKX_ERR_INVALID, "bar axis point out of range");
    a.bar_a = roles->bar_axis_a;
    a.bar_b = roles->bar_axis_b;
  }
  if (bad) return OKX_ERR_INVALID;
  const hipStream_t st = (hipStream_t)stream;
  {
    const long long init_blocks = (n_sweeps > 0 ? n_sweeps + 255 : 256) / 256;
    hipLaunchKernelGGL(dg::okx_diagnose_init, dim3((unsigned)init_blocks), dim3(256), 0, st, d_summary, (long long)n_sweeps, a.count);
    HIP_TRY(hipGetLastError());
  }
  if (n_sweeps == 0) return OKX_OK;
  const size_t slot_bytes = sizeof(double) * (size_t)(a.batch + 1) * (size_t)a.rowd * dg::kWaves;
  const size_t short_bytes = slot_bytes + sizeof(double) * (size_t)a.n_points * (size_t)(steps_per_sweep - 1);
  if (short_bytes <= 64 * 1024) {
    // a whole sweep per workgroup (ensembles of short sweeps): displacements in LDS
    const long long grid = n_sweeps < (long long)p->n_cu * 64 ? n_sweeps : (long long)p->n_cu * 64;
    hipLaunchKernelGGL(dg::okx_diagnose_short, dim3((unsigned)grid), dim3(dg::kThreads), short_bytes, st, a);
    HIP_TRY(hipGetLastError());
    return OKX_OK;
  }
  // long sweeps: displacements staged in the program's scratch buffer, then one wavefront per sweep and tracked point
  const long long need = n_sweeps * (long long)a.n_points * (steps_per_sweep - 1);
  if (const int32_t rc = diag_scratch(p, need, steps_per_sweep, st, &a.disp)) return rc;
  const long long per_tile = (long long)dg::kWaves * dg::kLongChunk;
  const long long tiles_per_sweep = (steps_per_sweep + per_tile - 1) / per_tile;
  const long long n_tiles = tiles_per_sweep * n_sweeps;
  const long long cap = (long long)p->n_cu * 64;
  hipLaunchKernelGGL(dg::okx_diagnose_states, dim3((unsigned)(n_tiles < cap ? n_tiles : cap)), dim3(dg::kThreads), slot_bytes, st, a,
                     tiles_per_sweep);
  HIP_TRY(hipGetLastError());
  if (a.n_points > 0) {
    const long long jobs = n_sweeps * a.n_points;
    hipLaunchKernelGGL(dg::okx_diagnose_select, dim3((unsigned)(jobs < cap ? jobs : cap)), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  return OKX_OK;
}

}  // extern "C"
