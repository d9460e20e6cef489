// okx_launch.cpp — the launch planner (okx_launch.hpp).  No heap, no strings: the plan is a stack struct of the caller.
#include "okx_launch.hpp"

#include <cstdarg>
#include <cstdio>

namespace okx {

namespace {

int refuse(LaunchPlan* plan, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(plan->message, sizeof(plan->message), fmt, ap);
  va_end(ap);
  plan->status = code;
  return code;
}

// The span (consecutive problems of one geometry) and the chain length the request names: > 0 explicit (chain = 1: the
// whole span), < 0 auto - sized once the family is known (auto_chain_len).
struct Span {
  long long span, n_spans, len0;
};

Span span_of(const LaunchRequest& rq) {
  Span s;
  s.span = rq.steps_per_geometry > 0 ? rq.steps_per_geometry : rq.n_problems;
  s.n_spans = rq.n_problems / s.span;
  s.len0 = rq.chain_len;
  if (s.len0 == 0) s.len0 = rq.chain ? s.span : 1;
  return s;
}

int grid_of(long long units, long long cap) { return (int)(units < cap ? (units < 1 ? 1 : units) : cap); }

}  // namespace

// Rounds of the lane and the quad kernel for this launch (one wavefront per SIMD either way): lane wave units hold 64
// problems of ONE geometry, so an ensemble with few steps per geometry leaves lanes idle and may be the quad kernel's after
// all.  The parallel unit is a CHAIN (a problem when chains have length 1): an explicit chain length - or chain = 1, the whole
// span - is counted as such; chain_len = -1 (auto) sizes its chains to the kernel chosen, from the problem count.
bool lane_pays(const okx_launch_caps& caps, const LaunchRequest& rq) {
  const Span s = span_of(rq);
  const long long simds = (long long)caps.n_cu * 4;
  long long len0 = s.len0;
  if (len0 < 1) len0 = 1;  // (auto)
  if (len0 > s.span) len0 = s.span;
  const long long chains_per_span = (s.span + len0 - 1) / len0;
  const long long lane_waves = s.n_spans * ((chains_per_span + 63) / 64);
  const long long quad_waves = (s.n_spans * chains_per_span + 15) / 16;
  const long long lane_rounds = (lane_waves + simds - 1) / simds, quad_rounds = (quad_waves + simds - 1) / simds;
  return 26 * lane_rounds < 19 * quad_rounds + 3;  // us per round (and chain step) of either kernel, measured on C2 / C4 shapes
}

// chain_len < 0: about one chain per resident problem slot of the family, balanced inside a geometry
long long auto_chain_len(const okx_launch_caps& caps, int family, long long n_problems, long long span) {
  long long slots = family == kFamilyLane     ? (long long)caps.n_cu * 4 * 64
                    : family == kFamilyQuad   ? (long long)caps.n_cu * caps.quad_waves_per_cu * caps.quad_ppw
                    : family == kFamilyPacked ? (long long)caps.n_cu * caps.packed_blocks_per_cu * caps.groups
                                              : (long long)caps.n_cu * caps.blocks_per_cu;
  if (slots < 1) slots = 1;  // (no program reports none; hand-made capabilities may)
  const long long ideal = (n_problems + slots - 1) / slots;
  if (ideal >= span) return span;
  long long per_span = (span + ideal - 1) / ideal;
  // lane kernel: a wave unit is 64 chains of ONE span, so the chains of a span come in multiples of 64
  if (family == kFamilyLane) per_span = (per_span + 63) / 64 * 64;
  if (per_span > span) per_span = span;
  return (span + per_span - 1) / per_span;
}

int plan_launch(const okx_launch_caps& caps, const LaunchRequest& rq, const char* quad_note, const char* lane_note,
                const char* ev_note, LaunchPlan* plan) {
  plan->status = OKX_OK;
  plan->message[0] = 0;
  plan->family = 0;
  plan->start = kStartCold;
  plan->auto_cold = plan->shared_first_step = plan->cold_if_table = false;
  plan->chain_len = plan->span = plan->units = 0;
  plan->grid = 0;
  // the predicted-convergence ending is not offered along the reference's zero-gradient
  // point-on-line valley: the step length says nothing about the distance there
  plan->confirm = (rq.confirm_full_pass != 0 || caps.line_row) ? 1 : 0;
  const Span s = span_of(rq);
  const bool use_quad = caps.has_quad && (rq.kernel == 0 || rq.kernel == 3 || rq.kernel == 4);
  if (rq.kernel == 3 && !use_quad) return refuse(plan, OKX_ERR_INVALID, "quad kernel requested but not available: %s", quad_note);
  if (rq.evaluated && !use_quad)
    return refuse(plan, OKX_ERR_INVALID, "evaluated solves run the generated kernels only (kernel = 0, 3 or 4)");
  // Lane kernel (one lane per problem, 64 per wavefront): auto selection from lane_min_problems on, when nothing the
  // quad kernel alone offers is asked for (fitted model, trace); kernel == 4 forces it.
  // (which body a launch needs is known once the chain length is: a body auto selection may not use sends the launch
  //  back to the quad kernel below)
  bool use_lane = caps.has_lane && use_quad && rq.predictor == 0 && (!caps.trace || caps.lane_timeline) &&
                  (rq.kernel == 4 || (rq.kernel == 0 && rq.n_problems >= caps.lane_min_problems && lane_pays(caps, rq)));
  const bool lane_auto = use_lane && rq.chain_len == -1 && !rq.evaluated;
  // "auto" on a sweep that fills wave units of 256 consecutive steps: the nested start mode (okx_lane_nest_*: four steps per
  // lane, 256 per wave unit) - every step but a lane's first starts from the interpolant of already solved neighbours (one
  // full pass + the confirming evaluation)
  const bool nested = lane_auto && caps.has_nest && s.span >= 256 && (s.span % 256 == 0 || s.span >= 2048);
  // ... or the coarse-to-fine start (okx_lane_refc_* / okx_lane_refw_*): every fourth step cold, the steps between from the
  // cubic interpolant of those: spans of at least 64 coarse steps
  const bool refined = lane_auto && !nested && caps.has_refine && rq.output != OKX_OUTPUT_NONE && rq.grad_tol == 0.0 &&
                       s.span >= 256 && s.span % 4 == 0;
  bool auto_cold = false;
  if (use_lane && rq.kernel == 0 && !nested) {
    const bool cold_launch = s.len0 == 1 || s.span == 1;
    if (s.len0 == -1 && !caps.lane_chain_ok && caps.lane_cold_ok) {
      // "auto" may also mean independent solves: where the lane kernel's chain body spills but its independent-solve body
      // does not (the double wishbone), cold starts on the lane kernel beat the quad kernel's chains (measured on 4096
      // geometries x 256 steps: 0.50 ms against 0.71 ms)
      auto_cold = true;
    } else if (cold_launch ? !caps.lane_cold_ok : !caps.lane_chain_ok) {
      use_lane = false;
    }
  }
  if (rq.evaluated && use_lane) {
    // the lane form of the evaluated module has the independent-solve bodies only: chains go to the quad kernel
    const bool cold_launch = s.len0 == 1 || s.span == 1 || auto_cold;
    if (!caps.ev_lane || !cold_launch) {
      if (rq.kernel == 4)
        return refuse(plan, OKX_ERR_INVALID, "no evaluated lane kernel for this launch: %s", caps.ev_lane ? "chains" : ev_note);
      use_lane = false;
      auto_cold = false;
    }
  }
  if (rq.kernel == 4 && !use_lane)
    return refuse(plan, OKX_ERR_INVALID, "lane kernel requested but not available: %s", lane_note[0] ? lane_note : "predictor / trace in use");
  // Kernel choice (profiles/r01/config_sweep_v3.txt).  The packed kernel keeps more problems in
  // flight per CU (G lane groups x resident waves): measured 1.5x on saturating batches of
  // n <= 15 systems (MacPherson grid), no gain for n = 18 (DW corner), so auto = packed only
  // for n <= 15 and batches of at least 8 problems per resident slot.
  bool use_packed = false;
  if (caps.has_packed && !use_quad) {
    const long long single_slots = (long long)caps.n_cu * caps.blocks_per_cu;
    if (rq.kernel == 2) use_packed = true;
    else if (rq.kernel == 0) use_packed = caps.nreg <= 15 && rq.n_problems >= 8 * single_slots;
  }
  plan->family = use_lane ? kFamilyLane : use_quad ? kFamilyQuad : use_packed ? kFamilyPacked : kFamilyInterpreter;
  long long len = s.len0;
  if (len < 0) len = auto_chain_len(caps, plan->family, rq.n_problems, s.span);
  if (auto_cold || (refined && use_lane)) len = 1;
  if (nested) len = kNestedChainLen;
  if (len < 1) len = 1;
  if (len > s.span) len = s.span;
  plan->chain_len = len;
  plan->span = s.span;
  plan->auto_cold = auto_cold;
  plan->start = nested ? kStartNested : (refined && use_lane) ? kStartRefined : len == 1 ? kStartCold : kStartChain;
  const long long chains_per_span = (s.span + len - 1) / len;
  if (use_quad) {
    // Shared first step: the design state's Jacobian, J^T J and damped factorisation are common to every problem
    // of a geometry, so they are evaluated once per geometry (one quad each) instead of once per chain head.
    plan->shared_first_step = caps.has_head && rq.shared_first_step != 0 && rq.grad_tol == 0.0 && caps.n_targets > 0;
  }
  if (use_lane) {
    plan->units = s.n_spans * ((chains_per_span + 63) / 64);
    plan->grid = grid_of(plan->units, (long long)caps.n_cu * 4);  // one wavefront per SIMD (512 registers, ~37 KB LDS)
  } else if (use_quad) {
    plan->units = (s.n_spans * chains_per_span + caps.quad_ppw - 1) / caps.quad_ppw;
    plan->grid = grid_of(plan->units, (long long)caps.n_cu * caps.quad_waves_per_cu);
    // independent solves from the own geometry's design state with its first-step table and nothing the general body
    // alone offers (fitted model, LM trace, gradient stop): the cold body
    // (not for programs with the reference's zero-gradient line row: their solves reject steps as a matter of course,
    //  which the cold body answers by starting over in its general loop - measured 4 % slower than the general body)
    plan->cold_if_table = caps.has_cold && !caps.line_row && !rq.geometry_tables && len == 1 && plan->shared_first_step &&
                          !(rq.predictor != 0 && caps.predictor) && (!caps.trace || caps.quad_timeline) && rq.grad_tol == 0.0 &&
                          !caps.no_cold && (!rq.evaluated || caps.ev_cold);
  } else if (use_packed) {
    plan->units = (s.n_spans * chains_per_span + caps.groups - 1) / caps.groups;
    plan->grid = grid_of(plan->units, (long long)caps.n_cu * caps.packed_blocks_per_cu);
  } else {
    long long cap = (long long)caps.n_cu * caps.blocks_per_cu;
    if (cap < 1) cap = 1;
    plan->units = s.n_spans * chains_per_span;
    plan->grid = grid_of(plan->units, cap);
  }
  return OKX_OK;
}

int lane_refine_grid(const okx_launch_caps& caps, const LaunchPlan& plan, long long n_problems, int offset) {
  const long long per_span = (plan.span - offset + 3) / 4;
  return grid_of((n_problems / plan.span) * ((per_span + 63) / 64), (long long)caps.n_cu * 4);
}

// Lane form (one lane per state, 64 per wavefront: a third of the quad form's instructions per state) once the batch
// gives every SIMD a wave unit; an ensemble's wave units hold states of ONE geometry, so few steps per geometry leave
// lanes idle and stay with the quad form.
bool evaluate_on_lane(const okx_launch_caps& caps, long long n_problems, long long steps_per_geometry, long long* units) {
  const long long span = steps_per_geometry > 0 ? steps_per_geometry : n_problems;
  *units = (n_problems / span) * ((span + 63) / 64);
  const bool fills = *units >= (long long)caps.n_cu * 4 && n_problems >= 48 * *units;
  return caps.ev_lane_pos && !caps.evaluate_quad && (fills || caps.evaluate_lane);
}

}  // namespace okx
