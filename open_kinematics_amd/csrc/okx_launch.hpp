// okx_launch.hpp — the launch planner: which kernel family, start mode, chain length and grid serve one launch.
// Plain C++ (no HIP, no okx_program): the launching entry points of okx_api.hip fill an okx_launch_caps from their program,
// call plan_launch and run what the plan says; tests plan from hand-made capabilities (okx_debug_plan_launch).
// "One choice per batch"  rests on this selection being a function of the capabilities and the request alone.
#pragma once

#include "../../include/okx_debug.h"

namespace okx {

enum LaunchFamily { kFamilyInterpreter = 1, kFamilyPacked = 2, kFamilyQuad = 3, kFamilyLane = 4 };  // = okx_solve_opts.kernel
enum LaunchStart { kStartCold = 0, kStartChain = 1, kStartNested = 2, kStartRefined = 3 };
constexpr int kNestedChainLen = 4;  // = kLaneNestSteps of okx_quad.hpp (asserted where both are seen, okx_api.hip)

// what the selection reads of a launch: the okx_solve_opts fields and the batch's shape
struct LaunchRequest {
  long long n_problems, steps_per_geometry, chain_len;
  int chain, kernel, predictor, output, confirm_full_pass, shared_first_step;
  double grad_tol;
  bool geometry_tables, evaluated;
};

inline LaunchRequest launch_request(const okx_solve_opts& o, long long n_problems, bool geometry_tables, bool evaluated) {
  return {n_problems, o.steps_per_geometry, o.chain_len, o.chain, o.kernel, o.predictor, o.output, o.confirm_full_pass,
          o.shared_first_step, o.grad_tol, geometry_tables, evaluated};
}

struct LaunchPlan {
  int status;              // okx_status; not OKX_OK: `message` says why the request cannot be served
  int family;              // LaunchFamily
  int start;               // LaunchStart (the lane kernel's nested and refined modes; cold = chains of length 1)
  bool auto_cold;          // chain_len = -1 resolved to independent solves on the lane kernel
  int confirm;             // SolveArgs / QuadArgs confirm
  bool shared_first_step;  // the launch looks for a first-step table (whether it gets one is known at launch only)
  bool cold_if_table;      // quad kernel: take the cold body if that table is there
  long long chain_len;
  long long span;          // consecutive problems of one geometry
  long long units;         // parallel units of the family: chains (interpreter) or wave units (packed, quad, lane)
  int grid;
  char message[512];
};

// The notes say why a kernel is absent (okx_program_kernel_note / _lane_note / _evaluation_note); never null.
int plan_launch(const okx_launch_caps& caps, const LaunchRequest& rq, const char* quad_note, const char* lane_note,
                const char* ev_note, LaunchPlan* plan);

// grid of launch `offset` (0 .. 3) of the refined start mode's four launches
int lane_refine_grid(const okx_launch_caps& caps, const LaunchPlan& plan, long long n_problems, int offset);

// okx_evaluate_batch: lane form (true; *units = its wave units) or quad form
bool evaluate_on_lane(const okx_launch_caps& caps, long long n_problems, long long steps_per_geometry, long long* units);

// the selection's arithmetic, by name
bool lane_pays(const okx_launch_caps& caps, const LaunchRequest& rq);
long long auto_chain_len(const okx_launch_caps& caps, int family, long long n_problems, long long span);

}  // namespace okx
