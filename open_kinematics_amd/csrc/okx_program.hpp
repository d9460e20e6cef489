// okx_program.hpp — the program object behind include/okx.h and what the units of the C-ABI share.  Which unit holds what:
//   okx_api.hip         the interpreter kernels (okx_kernels.hip, okx_packed.hip) and everything that must see them: program
//                       life cycle and kernel selection, source and precompile entry points, the solve path and the plan
//                       entry points, okx_eval_batch, okx_rebind_design, okx_expand_positions_batch, okx_tangent_batch, the
//                       okx_debug_* hooks
//   okx_attach.cpp      generated kernels: compile job, module loads, first-step tables (HIP runtime API only)
//   okx_evaluation.cpp  the evaluated modules: enabling, precompiling, okx_evaluate_batch (HIP runtime API only)
//   okx_predictor.cpp   okx_program_fit_predictor (on top of the public okx_solve_batch)
//   okx_metrics.hip, okx_shim_api.hip (kernel: okx_shim.hip), okx_diagnose.hip, okx_ensemble.hip, okx_select.hip,
//   okx_screen.hip, okx_covariance.hip, okx_curves.hip, okx_front.hip, okx_sample.hip: one pass each - kernels, launch plan,
//   argument checks and entry points together (what the six passes over an ensemble table share: okx_enstable.hpp)
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <functional>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include "okx_quad.hpp"

struct okx_launch_caps;  // include/okx_debug.h

struct okx_program {
  okx::DevProgram host{};      // host copy (dimensions, launch sizing)
  okx::DevProgram* dev = nullptr;  // device copy
  int device = 0;
  int n_cu = 0;
  size_t lds_bytes = 0;        // eval / rebind / single-problem solve kernels
  size_t solve_lds_bytes = 0;  // selected solve kernel
  int blocks_per_cu = 0;
  int nreg = 0;                // padded row length of the register-resident factorisation
  const void* solve_fn = nullptr;    // okx_solve_kernel<NREG> (one problem per wavefront; two wavefronts for n > 63)
  const void* eval_fn = nullptr;     // okx_eval_kernel<threads>
  int threads = 0;             // threads per problem of the generic kernels: 64, or 128 for n > 63
  const void* tangent_fn = nullptr;  // okx_tangent_kernel<NREG> (generic tangents)
  int groups = 0;              // problems per wavefront of the packed kernel (1 = not available)
  int group_width = 0;         // lanes per problem in the packed kernel
  const void* packed_fn = nullptr;   // okx_solve_packed_kernel<NREG, G> or null
  size_t packed_lds_bytes = 0;
  int packed_blocks_per_cu = 0;
  bool line_row = false;       // the program has the reference's zero-gradient point-on-line row
  // runtime-specialised quad kernel (okx_quadgen.cpp / okx_jit.cpp); null when not available
  hipModule_t quad_mod = nullptr;
  hipFunction_t quad_fn_u = nullptr;  // program's own geometry
  hipFunction_t quad_fn_g = nullptr;  // per-geometry tables
  hipFunction_t quad_fn_eval = nullptr;  // parity kernel
  hipFunction_t quad_fn_expand = nullptr;  // positions from free coordinates (single mode)
  hipFunction_t quad_fn_tan_u = nullptr, quad_fn_tan_g = nullptr;  // tangents (null when a free point is not an output point)
  int quad_waves_per_cu = 0;
  int quad_ppw = 0;             // problems per wavefront: 16 (one quad each) or 8 (pair mode: one quad per half)
  char quad_note[256] = "";     // why the quad kernel is not in use (empty when it is)
  double* predictor_dev = nullptr;  // chain-head model fitted by okx_program_fit_predictor, or null
  long long predictor_len = 0;  // doubles in it
  // shared first step of the chain heads (okx_quad_head_u/_g; null functions: not generated for this program)
  hipFunction_t quad_fn_head_u = nullptr, quad_fn_head_g = nullptr;
  hipFunction_t quad_fn_cold_u = nullptr;  // independent solves from the own geometry's design state with its first-step table (null: none)
  int head_stride = 0;          // doubles per geometry in the table (okx::quad_head_stride)
  // own geometry's tables, one per lambda0 ever asked for (never overwritten: launches on other streams may still be
  // reading an older one); the default lambda0's is filled synchronously at okx_program_create, any other on first use on
  // the caller's stream, with an event that launches on other streams wait for
  struct HeadTable { double lambda0; double* dev; hipEvent_t ready; hipStream_t filled_on; };
  std::vector<HeadTable> head_tables;
  std::mutex head_mutex;
  // Tiered start.  A program whose generated kernels are not in the kernel cache is served by the interpreter kernels
  // while a host thread runs the compiler (hiprtc: no device call on that thread); the first entry point that finds the
  // job finished loads the code objects and switches the program over, under `head_mutex`.  Null: nothing pending.
  // The job owns everything it touches (its own copy of the host program, the code objects it produced): the program may
  // be destroyed while the compiler runs, and the switch-over loads the job's results from memory - the kernel cache on disk
  // is only a cache (a read-only cache directory must not cost a second compile).
  struct JitJob {
    std::thread thread;
    std::atomic<int> finished{0};
    std::atomic<int> quad_ready{0};   // the quad module is compiled (the lane module may still be in the works)
    std::atomic<int> quad_attached{0};  // ... and already switched over to (written under the program's jit_mutex)
    okx::DevProgram host;
    bool want_quad = false, want_lane = false;   // what was not in the cache at create
    bool quad_ok = false, lane_ok = false;
    std::string quad_code, quad_why, lane_code, lane_why;
    std::vector<okx::LaneOverride> lane_overrides;
  };
  std::atomic<JitJob*> jit{nullptr};
  std::mutex jit_mutex;
  // Generated-kernel state (module handles, function pointers, notes) is read by every launching entry point under a
  // shared lock and rewritten by the switch-over / okx_program_enable_evaluation under the exclusive one.
  std::shared_mutex kern_mutex;
  double* head_geom_dev = nullptr;  // scratch table of the latest launch with geometry tables (grow-only)
  long long head_geom_cap = 0;      // geometries it holds
  double* diag_scratch = nullptr;   // step displacements of okx_diagnose_sweeps_batch's long sweeps (grow-only)
  long long diag_scratch_len = 0;   // doubles it holds
  double* quad_trace = nullptr;     // diagnostic hook, see okx_debug_quad_trace (null: off)
  long long quad_trace_problem = 0;
  // lane kernel (okx_lanegen.cpp): one lane per problem, for batches of at least lane_min_problems; null when the
  // program does not fit one lane's registers (or the quad kernel, whose first-step tables it shares, is absent)
  hipModule_t lane_mod = nullptr;
  std::vector<hipModule_t> lane_extra_mods;  // modules single kernels are taken from (okx::LaneOverride)
  hipFunction_t lane_fn_u = nullptr, lane_fn_g = nullptr, lane_fn_eval = nullptr;  // independent solves (chain_len 1), parity kernel
  hipFunction_t lane_chain_u = nullptr, lane_chain_g = nullptr;  // chains
  hipFunction_t lane_compact[4] = {};                // the same four with compact outputs (solve_u, solve_g, chain_u, chain_g)
  hipFunction_t lane_nest[4] = {};                   // nested start mode: u, g, u compact, g compact (null: none)
  hipFunction_t lane_refine[8] = {};                 // coarse-to-fine start (developer switch lane_refine): coarse u, g, u compact, g compact; warm likewise
  int lane_nest_scratch = 0;
  long long lane_min_problems = 0;
  int lane_cold_scratch = 0, lane_chain_scratch = 0;  // private-segment bytes of the two bodies (code object metadata)
  bool lane_cold_ok = false, lane_chain_ok = false;   // bodies that auto selection may use
  char lane_note[256] = "";
  // evaluated modules (okx_program_enable_evaluation): the solve bodies with the tangent / metric epilogue, specialised to
  // one set of metric role points; null until enabled
  hipModule_t ev_mod = nullptr, ev_lane_mod = nullptr;
  hipFunction_t ev_solve_u = nullptr, ev_solve_g = nullptr, ev_cold_u = nullptr, ev_pos_u = nullptr, ev_pos_g = nullptr;  // quad form (single mode)
  hipFunction_t ev_lane_u = nullptr, ev_lane_g = nullptr;           // lane form: independent solves (null: none)
  hipFunction_t ev_lane_pos_u = nullptr, ev_lane_pos_g = nullptr;   // lane form of okx_evaluate_batch (null: none)
  int ev_lane_scratch = 0;
  okx::EvalSpec ev_spec{};     // the role points compiled into them
  okx::EvalScalars ev_cfg{};   // the roles' numeric part, a kernel argument
  // a composed axle's evaluated module (okx_program_enable_axle_evaluation): the same kernel slots, specialised to both
  // corners' role points and the roles' points and kinds
  bool ev_axle = false;
  okx::AxleEvalSpec ev_axle_spec{};
  okx::EvalScalars ev_cfg_r{};        // the right corner's numbers
  okx::EvalRoleNum ev_roles[8] = {};  // the roles' numbers
  char ev_note[256] = "";      // why there are none / no lane form

  okx_program() = default;
  okx_program(const okx_program&) = delete;
  okx_program& operator=(const okx_program&) = delete;
  ~okx_program();  // unloads the modules, frees the device buffers (the compile job is okx_program_destroy's)
};

namespace okx {

constexpr int kMaxLdsBytes = 160 * 1024;  // LDS per CU on gfx950

extern thread_local char g_err[512];  // okx_last_error(), per thread
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return okx::fail(OKX_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));    \
  } while (0)

int quad_waves_per_simd();
bool stream_is_capturing(hipStream_t stream);  // true while `stream` records into a HIP graph

// design_pos / row_param / dop_param of the program's device copy, into the arguments of a generated kernel
template <class Args>
inline void set_program_tables(const okx_program* p, Args* a) {
  const char* base = reinterpret_cast<const char*>(p->dev);
  a->design_pos = reinterpret_cast<const double*>(base + offsetof(DevProgram, design_pos));
  a->row_param = reinterpret_cast<const double*>(base + offsetof(DevProgram, row_param));
  a->dop_param = reinterpret_cast<const double*>(base + offsetof(DevProgram, dop_param));
}

int own_head_table(okx_program* p, double lambda0, hipStream_t stream, double** table);
void attach_quad_kernel(okx_program* p, bool cache_only = false, bool* pending = nullptr, const okx_program::JitJob* job = nullptr);
void attach_lane_kernel(okx_program* p, bool cache_only = false, bool* pending = nullptr, const okx_program::JitJob* job = nullptr);
int lane_worst_scratch(const std::string& code, const std::vector<LaneOverride>& overrides, const char* prefix);
void attach_cached_or_compile(okx_program* p);  // okx_program_create: the cached kernels, or a compile job for what is missing
void attach_when_ready(okx_program* p, bool wait, const hipStream_t* stream = nullptr);
void retire_jit_job(okx_program* p);  // okx_program_destroy: join the job, or leave it to the orphan registry
void release_evaluation(okx_program* p);
// Loads an evaluated quad module into the program's ev_* slots (ev_mod, ev_solve_g, ev_pos_u/_g, the optional ev_cold_u);
// *solve_u is the gate the caller publishes last, after its role numbers.
int load_evaluated_module(okx_program* p, const std::string& code, hipFunction_t* solve_u);

// okx_api.hip, for the units beside it
int with_dev_program(const okx_program_desc* desc, const std::function<int(const DevProgram&)>& use);  // a description's DevProgram, handed to `use`
bool geometry_tables_paired(const double* d_geom_pos, const double* d_geom_row_param);
bool steps_per_geometry_fits(long long n_problems, long long spg, bool geometry_tables);
void fill_launch_caps(const okx_program* p, okx_launch_caps* c);  // under the program's shared lock
// okx_metrics.hip: a corner's metric roles against the record's n_out points (`who` opens the message)
int check_corner_roles(const okx_corner_roles* roles, int32_t n_out, const char* who);

}  // namespace okx
