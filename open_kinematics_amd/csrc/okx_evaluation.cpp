// okx_evaluation.cpp — the evaluated modules of a program (include/okx.h): enabling them for a corner's or an axle's metric
// roles, their precompile entry points, and okx_evaluate_batch on given states.  Host code on the HIP runtime API only (no
// kernel is named here): built as plain C++, like okx_attach.cpp.
#include "okx_program.hpp"

#include <cstdio>
#include <cstring>

#include "okx_launch.hpp"

using okx::fail;

extern "C" {

int32_t okx_program_enable_evaluation(okx_program* p, const okx_corner_roles* roles) {
  if (!p || !roles) return fail(OKX_ERR_INVALID, "null program or roles");
  if (int32_t rc = okx::check_corner_roles(roles, p->host.n_out, "roles")) return rc;
  okx::attach_when_ready(p, true);  // the evaluated kernels share the solve kernels' first-step tables: those first
  okx::EvalSpec spec;
  std::string why;
  if (!okx::eval_spec_from_roles(p->host, *roles, &spec, &why)) return fail(OKX_ERR_INVALID, "%s", why.c_str());
  bool with_lane = false;
  {
    std::shared_lock<std::shared_mutex> readers(p->kern_mutex);
    if (!p->quad_fn_u || p->quad_ppw != 16) {
      const std::string note = p->quad_note[0] ? p->quad_note : "a pair-mode program";
      readers.unlock();
      std::unique_lock<std::shared_mutex> writer(p->kern_mutex);
      std::snprintf(p->ev_note, sizeof(p->ev_note), "no single-mode quad kernel (%.180s)", note.c_str());
      return fail(OKX_ERR_INVALID, "evaluated solves need the program's single-mode quad kernel: %s", p->ev_note);
    }
    if (p->ev_solve_u && std::memcmp(&spec, &p->ev_spec, sizeof(spec)) == 0) {
      // same role points as before: only the numbers change (launches read them as a kernel argument)
      readers.unlock();
      std::unique_lock<std::shared_mutex> writer(p->kern_mutex);
      okx::eval_scalars_from_roles(*roles, &p->ev_cfg);
      return OKX_OK;
    }
    with_lane = p->lane_fn_u != nullptr && !okx::dev_switch("no_lane");
  }
  // generate + compile (or fetch from the cache) outside the lock: launches of this program go on meanwhile
  std::string code, lcode, lwhy;
  int lane_scratch = -1;
  if (!okx::quad_eval_build(p->host, spec, okx::quad_waves_per_simd(), &code, &why)) {
    std::unique_lock<std::shared_mutex> writer(p->kern_mutex);
    std::snprintf(p->ev_note, sizeof(p->ev_note), "%.250s", why.c_str());
    return fail(OKX_ERR_LIMIT, "no evaluated kernels for this program: %s", why.c_str());
  }
  const bool lane_built = with_lane && okx::lane_eval_build(p->host, spec, &lcode, &lwhy, false, &lane_scratch);
  std::unique_lock<std::shared_mutex> kernels(p->kern_mutex);
  hipFunction_t su = nullptr;
  if (const int32_t rc = okx::load_evaluated_module(p, code, &su)) return rc;
  p->ev_spec = spec;
  p->ev_axle = false;
  okx::eval_scalars_from_roles(*roles, &p->ev_cfg);
  // the lane form, for programs whose solves have one (failure only means the quad form serves every batch size)
  if (with_lane && !lane_built) {
    std::snprintf(p->ev_note, sizeof(p->ev_note), "no lane form: %.230s", lwhy.c_str());
  } else if (with_lane && lane_scratch > 512) {
    std::snprintf(p->ev_note, sizeof(p->ev_note), "the lane form spills %d B of scratch: not used", lane_scratch);
  } else if (with_lane) {
    hipModule_t lmod = nullptr;
    if (hipModuleLoadData(&lmod, lcode.data()) == hipSuccess &&
        hipModuleGetFunction(&p->ev_lane_u, lmod, "okx_lane_evsolve_u") == hipSuccess &&
        hipModuleGetFunction(&p->ev_lane_g, lmod, "okx_lane_evsolve_g") == hipSuccess) {
      p->ev_lane_mod = lmod;
      p->ev_lane_scratch = lane_scratch;
      // the same epilogue on given states (optional: programs whose free points are not all output points have none)
      if (hipModuleGetFunction(&p->ev_lane_pos_u, lmod, "okx_lane_evaluate_u") != hipSuccess ||
          hipModuleGetFunction(&p->ev_lane_pos_g, lmod, "okx_lane_evaluate_g") != hipSuccess) {
        (void)hipGetLastError();
        p->ev_lane_pos_u = p->ev_lane_pos_g = nullptr;
      }
    } else {
      (void)hipGetLastError();
      if (lmod) (void)hipModuleUnload(lmod);
      p->ev_lane_u = p->ev_lane_g = nullptr;
      p->ev_lane_pos_u = p->ev_lane_pos_g = nullptr;
      std::snprintf(p->ev_note, sizeof(p->ev_note), "the lane form's code object did not load");
    }
  }
  p->ev_solve_u = su;  // the gate of the evaluated launch paths
  return OKX_OK;
}

int32_t okx_program_evaluation(const okx_program* p) { return p && p->ev_solve_u ? 1 | (p->ev_lane_u ? 2 : 0) : 0; }
const char* okx_program_evaluation_note(const okx_program* p) { return p ? p->ev_note : ""; }
int32_t okx_program_eval_columns(const okx_program* p) {
  return p && p->ev_solve_u ? (p->ev_axle ? OKX_EVAL_AXLE_COLUMNS : OKX_EVAL_COLUMNS) : 0;
}

static int32_t check_axle_roles(const okx_axle_roles* roles, int32_t n_out) {
  if (int32_t rc = okx::check_corner_roles(&roles->left, n_out, "left")) return rc;
  if (int32_t rc = okx::check_corner_roles(&roles->right, n_out, "right")) return rc;
  if (roles->n_roles < 0 || roles->n_roles > OKX_MAX_ROTATIONS) return fail(OKX_ERR_INVALID, "n_roles must be 0 .. %d", OKX_MAX_ROTATIONS);
  return OKX_OK;
}

static void axle_numbers_from_roles(okx_program* p, const okx_axle_roles* roles) {
  okx::eval_scalars_from_roles(roles->left, &p->ev_cfg);
  okx::eval_scalars_from_roles(roles->right, &p->ev_cfg_r);
  std::memset(p->ev_roles, 0, sizeof(p->ev_roles));
  for (int k = 0; k < roles->n_roles; ++k) {
    const okx_rotation_role& r = roles->roles[k];
    okx::EvalRoleNum& n = p->ev_roles[k];
    for (int i = 0; i < 3; ++i) n.design[i] = r.design[i], n.axis_point[i] = r.axis_point[i], n.axis_dir[i] = r.axis_dir[i];
    n.scale = r.scale;
  }
}

/* okx_program_enable_evaluation for a composed axle (pair-mode program): see okx.h. */
int32_t okx_program_enable_axle_evaluation(okx_program* p, const okx_axle_roles* roles) {
  if (!p || !roles) return fail(OKX_ERR_INVALID, "null program or roles");
  if (int32_t rc = check_axle_roles(roles, p->host.n_out)) return rc;
  okx::attach_when_ready(p, true);
  okx::AxleEvalSpec spec;
  std::memset(&spec, 0, sizeof(spec));
  std::string why;
  if (!okx::axle_eval_spec_from_roles(p->host, *roles, &spec, &why)) return fail(OKX_ERR_INVALID, "%s", why.c_str());
  {
    std::shared_lock<std::shared_mutex> readers(p->kern_mutex);
    if (!p->quad_fn_u || p->quad_ppw != 8) {
      const std::string note = p->quad_note[0] ? p->quad_note : "a single-mode program (use okx_program_enable_evaluation)";
      readers.unlock();
      std::unique_lock<std::shared_mutex> writer(p->kern_mutex);
      std::snprintf(p->ev_note, sizeof(p->ev_note), "no pair-mode quad kernel (%.180s)", note.c_str());
      return fail(OKX_ERR_INVALID, "an axle's evaluated solves need the program's pair-mode quad kernel: %s", p->ev_note);
    }
    if (p->ev_solve_u && p->ev_axle && std::memcmp(&spec, &p->ev_axle_spec, sizeof(spec)) == 0) {
      readers.unlock();
      std::unique_lock<std::shared_mutex> writer(p->kern_mutex);
      axle_numbers_from_roles(p, roles);  // same points: only the numbers change (launches read them as kernel arguments)
      return OKX_OK;
    }
  }
  std::string code;
  if (!okx::quad_axle_eval_build(p->host, spec, okx::quad_waves_per_simd(), &code, &why)) {
    std::unique_lock<std::shared_mutex> writer(p->kern_mutex);
    std::snprintf(p->ev_note, sizeof(p->ev_note), "%.250s", why.c_str());
    return fail(OKX_ERR_LIMIT, "no evaluated kernels for this program: %s", why.c_str());
  }
  std::unique_lock<std::shared_mutex> kernels(p->kern_mutex);
  hipFunction_t su = nullptr;
  if (const int32_t rc = okx::load_evaluated_module(p, code, &su)) return rc;
  p->ev_axle = true;
  p->ev_axle_spec = spec;
  axle_numbers_from_roles(p, roles);
  p->ev_solve_u = su;  // the gate of the evaluated launch paths
  return OKX_OK;
}

int32_t okx_precompile_axle_evaluation(const okx_program_desc* desc, const okx_axle_roles* roles) {
  if (!desc || !roles) return fail(OKX_ERR_INVALID, "null pointer");
  return okx::with_dev_program(desc, [&](const okx::DevProgram& program) {
    if (int32_t rc = check_axle_roles(roles, program.n_out)) return (int)rc;
    okx::AxleEvalSpec spec;
    std::memset(&spec, 0, sizeof(spec));
    std::string why, code;
    if (!okx::axle_eval_spec_from_roles(program, *roles, &spec, &why)) return fail(OKX_ERR_INVALID, "%s", why.c_str());
    if (!okx::quad_axle_eval_build(program, spec, okx::quad_waves_per_simd(), &code, &why))
      return fail(why.compare(0, 14, "compile failed") == 0 ? OKX_ERR_DEVICE : OKX_ERR_LIMIT, "no evaluated kernels for this program: %s", why.c_str());
    return (int)OKX_OK;
  });
}

int32_t okx_evaluate_batch(okx_program* p, int64_t n_problems, int64_t steps_per_geometry, const double* d_pos,
                           const double* d_geom_pos, const double* d_geom_row_param, double* d_tangents, double* d_eval,
                           void* stream) {
  if (!p) return fail(OKX_ERR_INVALID, "null program");
  std::shared_lock<std::shared_mutex> kernels(p->kern_mutex);
  if (!p->ev_solve_u) return fail(OKX_ERR_INVALID, "okx_evaluate_batch needs okx_program_enable_evaluation first%s%s", p->ev_note[0] ? ": " : "", p->ev_note);
  if (n_problems < 0) return fail(OKX_ERR_INVALID, "negative problem count");
  if (n_problems == 0) return OKX_OK;
  if (!d_pos || (!d_tangents && !d_eval)) return fail(OKX_ERR_INVALID, "null pointer");
  if (!okx::geometry_tables_paired(d_geom_pos, d_geom_row_param))
    return fail(OKX_ERR_INVALID, "geometry positions and row parameters must be given together");
  if (!okx::steps_per_geometry_fits(n_problems, steps_per_geometry, d_geom_pos != nullptr)) return fail(OKX_ERR_INVALID, "bad steps_per_geometry");
  {
    okx_launch_caps caps;
    okx::fill_launch_caps(p, &caps);  // (evaluate_on_lane reads n_cu, ev_lane_pos and the evaluate_quad / evaluate_lane switches of it)
    long long units = 0;
    if (okx::evaluate_on_lane(caps, n_problems, steps_per_geometry, &units)) {
      okx::QuadEvArgs qe{};
      okx::QuadArgs& a = qe.q;
      a.targets = d_pos;  // (the GIVEN bodies read the records through this pointer: okx_lanegen.cpp)
      a.geom_pos = d_geom_pos;
      a.geom_row_param = d_geom_row_param;
      a.n_problems = n_problems;
      a.steps_per_geometry = steps_per_geometry;
      a.chain_len = 1;
      okx::set_program_tables(p, &a);
      a.out_mode = OKX_OUTPUT_NONE;  // (no records, no info; iteration limits, tolerances, trace, predictor and table stay zero)
      qe.tan = d_tangents;
      qe.ev = d_eval;
      qe.cfg = p->ev_cfg;
      const long long cap = (long long)p->n_cu * 4;
      void* kargs[] = {(void*)&qe};
      HIP_TRY(hipModuleLaunchKernel(d_geom_pos ? p->ev_lane_pos_g : p->ev_lane_pos_u, (int)(units < cap ? units : cap), 1, 1, okx::kWave, 1, 1,
                                    0, (hipStream_t)stream, kargs, nullptr));
      return OKX_OK;
    }
  }
  okx::QuadEvPosArgs q;
  q.pos = d_pos;
  q.geom_pos = d_geom_pos;
  q.geom_row_param = d_geom_row_param;
  q.tan = d_tangents;
  q.ev = d_eval;
  q.n_problems = n_problems;
  q.steps_per_geometry = steps_per_geometry > 0 ? steps_per_geometry : n_problems;
  okx::set_program_tables(p, &q);
  q.cfg = p->ev_cfg;
  q.cfg_r = p->ev_cfg_r;
  std::memcpy(q.roles, p->ev_roles, sizeof(q.roles));
  const long long waves = (n_problems + p->quad_ppw - 1) / p->quad_ppw;
  // (a streaming launch: several rounds' worth of workgroups - but an axle's own-geometry body keeps its chain constants and
  //  fixed points across a persistent loop: one wavefront per SIMD)
  const long long cap = (long long)p->n_cu * p->quad_waves_per_cu * (p->ev_axle && !d_geom_pos ? 1 : 8);
  void* kargs[] = {(void*)&q};
  HIP_TRY(hipModuleLaunchKernel(d_geom_pos ? p->ev_pos_g : p->ev_pos_u, (int)(waves < cap ? waves : cap), 1, 1, okx::kWave, 1, 1, 0,
                                (hipStream_t)stream, kargs, nullptr));
  return OKX_OK;
}

int32_t okx_precompile_evaluation(const okx_program_desc* desc, const okx_corner_roles* roles) {
  if (!desc || !roles) return fail(OKX_ERR_INVALID, "null pointer");
  return okx::with_dev_program(desc, [&](const okx::DevProgram& program) {
    okx::EvalSpec spec;
    std::string why, code;
    if (!okx::eval_spec_from_roles(program, *roles, &spec, &why)) return fail(OKX_ERR_INVALID, "%s", why.c_str());
    if (!okx::quad_eval_build(program, spec, okx::quad_waves_per_simd(), &code, &why))
      return fail(why.compare(0, 14, "compile failed") == 0 ? OKX_ERR_DEVICE : OKX_ERR_LIMIT, "no evaluated kernels for this program: %s", why.c_str());
    if (program.n_free <= okx::kLaneMaxFree) {
      std::string lcode, lwhy;
      (void)okx::lane_eval_build(program, spec, &lcode, &lwhy);  // (programs / variants it does not fit simply have no lane form)
    }
    return (int)OKX_OK;
  });
}

}  // extern "C"
