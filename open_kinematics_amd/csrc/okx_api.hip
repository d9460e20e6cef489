// okx_api.hip — the C-ABI of include/okx.h on top of the interpreter kernels: everything that has to see them (kernel
// selection, their launches), the solve path and the program's life cycle.  The program object and the shared helpers are in
// okx_program.hpp (which says what the other units hold), the generated kernels' life cycle (compile job, module loads,
// first-step tables) in okx_attach.cpp, the choice of kernel family, start mode, chain length and grid for a launch in
// okx_launch.cpp.  Every other pass keeps its entry points beside its kernels, in a unit of its own.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "okx_kernels.hip"
#include "okx_packed.hip"
#include "okx_program.hpp"
#include "okx_launch.hpp"

static_assert(okx::kNestedChainLen == okx::kLaneNestSteps, "the planner's nested chain length is the lane kernel's");

namespace {

using okx::fail;
using okx::g_err;
using okx::kMaxLdsBytes;
using okx::attach_when_ready;
using okx::quad_waves_per_simd;
using okx::stream_is_capturing;
using okx::fill_launch_caps;
using okx::geometry_tables_paired;
using okx::steps_per_geometry_fits;
using okx::with_dev_program;

typedef void (*solve_kernel_t)(const okx::DevProgram*, okx::SolveArgs);
typedef void (*packed_kernel_t)(const okx::DevProgram*, okx::SolveArgs, int);

// Every program gets the one-problem-per-wavefront kernel (register LDL^T, template on the
// padded row length) and, when a problem fits 32 lanes, the lane-group packed kernel too.
struct SolveKernels {
  int nreg;
  const void *solve, *tangent;
};
struct PackedKernel {
  int nreg, groups;
  const void* solve;
};
#define OKX_SOLVE_KERNELS(NREG) \
  {NREG, (const void*)(solve_kernel_t)okx::okx_solve_kernel<NREG, false>, (const void*)okx::okx_tangent_kernel<NREG>}
#define OKX_PACKED_KERNEL(NREG, G) {NREG, G, (const void*)(packed_kernel_t)okx::okx_solve_packed_kernel<NREG, G, false>}

void select_solve_kernels(okx_program* p) {
  // by padded row length; the last: 64 ... 126 variables, two wavefronts per problem, LDL^T rows in LDS (okx_kernels.hip
  // ldlt_solve_wide)
  static const SolveKernels kBySize[] = {OKX_SOLVE_KERNELS(15), OKX_SOLVE_KERNELS(18), OKX_SOLVE_KERNELS(21), OKX_SOLVE_KERNELS(24),
                                         OKX_SOLVE_KERNELS(36), OKX_SOLVE_KERNELS(48), OKX_SOLVE_KERNELS(63), OKX_SOLVE_KERNELS(126)};
  const int n = p->host.n, m = p->host.m;
  const SolveKernels* k = kBySize;
  while (k->nreg < n && k->nreg != 126) ++k;
  p->solve_fn = k->solve;
  p->tangent_fn = k->tangent;
  p->nreg = k->nreg;
  p->threads = okx::GroupWidth<126>::value * (n > 63) + okx::kWave * (n <= 63);
  p->eval_fn = n > 63 ? (const void*)okx::okx_eval_kernel<2 * okx::kWave> : (const void*)okx::okx_eval_kernel<okx::kWave>;

  p->groups = 1;
  p->group_width = 64;
  p->packed_fn = nullptr;
  if (n > 24) return;
  const int width = m > p->nreg + 1 ? m : p->nreg + 1;  // the rhs row lives at local lane nreg
  int groups = 64 / width;
  if (groups > 4) groups = 4;
  if (groups < 2) return;
  // the instantiation with the most groups that the width allows.  (The order of the rows is the order of instantiation,
  // hence the layout of the code object: keep it.)
  static const PackedKernel kPacked[] = {OKX_PACKED_KERNEL(15, 3), OKX_PACKED_KERNEL(15, 2), OKX_PACKED_KERNEL(15, 4), OKX_PACKED_KERNEL(18, 3),
                                         OKX_PACKED_KERNEL(18, 2), OKX_PACKED_KERNEL(21, 2), OKX_PACKED_KERNEL(24, 2)};
  for (const PackedKernel& pk : kPacked)
    if (pk.nreg == p->nreg && pk.groups <= groups && pk.groups > p->groups) {
      p->groups = pk.groups;
      p->group_width = width;
      p->packed_fn = pk.solve;
    }
}
#undef OKX_SOLVE_KERNELS
#undef OKX_PACKED_KERNEL

// Resident single-wave workgroups per CU.  The occupancy API assumes 64 KiB of LDS per CU on
// this stack, so the limit is derived here: 512 VGPRs per SIMD lane (8-register granules),
// 160 KiB LDS per CU, 8 waves per SIMD.
int resident_blocks_per_cu(const void* fn, size_t lds_bytes, int threads = okx::kWave) {
  int occ = 32;
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.numRegs > 0) {
    const int alloc = (fa.numRegs + 7) / 8 * 8;
    int per_simd = 512 / alloc;
    if (per_simd > 8) per_simd = 8;
    if (per_simd < 1) per_simd = 1;
    occ = 4 * per_simd;
  }
  occ /= threads > okx::kWave ? threads / okx::kWave : 1;  // workgroups of two wavefronts (n > 63)
  const int by_lds = (int)((160 * 1024) / (lds_bytes ? lds_bytes : 1));
  if (by_lds < occ) occ = by_lds;
  if (occ < 1) occ = 1;
  return occ;
}

int grid_for(const okx_program* p, long long units) {
  long long cap = (long long)p->n_cu * p->blocks_per_cu;
  if (cap < 1) cap = 1;
  return (int)(units < cap ? (units < 1 ? 1 : units) : cap);
}

}  // namespace

// What the other units of the C-ABI use of this one (declared in okx_program.hpp).
namespace okx {

// What okx_quad_source / okx_lane_source / the precompile entry points share: the DevProgram of `desc`, handed to `use`
// (which returns an okx_status and reports its own failures through fail()).
int with_dev_program(const okx_program_desc* desc, const std::function<int(const DevProgram&)>& use) {
  DevProgram* tmp = new (std::nothrow) DevProgram;
  if (!tmp) return fail(OKX_ERR_ALLOC, "out of host memory");
  int rc = build_dev_program(desc, tmp, g_err, (int)sizeof(g_err));
  if (rc == OKX_OK) rc = use(*tmp);
  delete tmp;
  return rc;
}

// The shape of a batch with optional per-geometry tables (every entry point that takes one; each has its own message texts)
bool geometry_tables_paired(const double* d_geom_pos, const double* d_geom_row_param) {
  return (d_geom_pos == nullptr) == (d_geom_row_param == nullptr);
}
bool steps_per_geometry_fits(long long n_problems, long long spg, bool geometry_tables) {
  return !(spg < 0 || (geometry_tables && spg == 0) || (spg > 0 && n_problems % spg != 0));
}

// What the planner reads of a program (under the program's shared lock); the developer switches as the environment has them.
void fill_launch_caps(const okx_program* p, okx_launch_caps* c) {
  c->lane_min_problems = p->lane_min_problems;
  c->n_cu = p->n_cu;
  c->n = p->host.n;
  c->nreg = p->nreg;
  c->n_targets = p->host.n_targets;
  c->blocks_per_cu = p->blocks_per_cu;
  c->packed_blocks_per_cu = p->packed_blocks_per_cu;
  c->groups = p->groups;
  c->has_packed = p->packed_fn != nullptr;
  c->has_quad = p->quad_fn_u != nullptr;
  c->quad_ppw = p->quad_ppw;
  c->quad_waves_per_cu = p->quad_waves_per_cu;
  c->has_head = p->quad_fn_head_u != nullptr;
  c->has_cold = p->quad_fn_cold_u != nullptr;
  c->has_lane = p->lane_fn_u != nullptr;
  c->lane_cold_ok = p->lane_cold_ok;
  c->lane_chain_ok = p->lane_chain_ok;
  c->has_nest = p->lane_nest[0] != nullptr;
  c->has_refine = p->lane_refine[0] != nullptr;
  c->ev_enabled = p->ev_solve_u != nullptr;
  c->ev_lane = p->ev_lane_u != nullptr;
  c->ev_cold = p->ev_cold_u != nullptr;
  c->ev_lane_pos = p->ev_lane_pos_u != nullptr;
  c->line_row = p->line_row;
  c->trace = p->quad_trace != nullptr;
  c->predictor = p->predictor_dev != nullptr;
  const bool dev = std::getenv("OKX_DEV") != nullptr;  // (one look at the environment per launch)
  c->lane_timeline = dev && okx::dev_switch("lane_timeline");
  c->quad_timeline = dev && okx::dev_switch("quad_timeline");
  c->no_cold = dev && okx::dev_switch("no_cold");
  c->evaluate_quad = dev && okx::dev_switch("evaluate_quad");
  c->evaluate_lane = dev && okx::dev_switch("evaluate_lane");
}

}  // namespace okx

extern "C" {

int32_t okx_abi_version(void) { return OKX_ABI_VERSION; }

const char* okx_last_error(void) { return g_err; }

void okx_default_opts(okx_solve_opts* o) {
  if (!o) return;
  o->max_iter = 100;
  o->chain = 0;
  o->steps_per_geometry = 0;
  o->chain_len = 0;
  o->step_tol = 1e-11;
  o->grad_tol = 0.0;
  o->ftol = 1e-10;
  o->lambda0 = 1e-6;
  o->residual_tolerance = 1e-3;
  o->kernel = 0;
  o->confirm_full_pass = 0;
  o->predictor = 0;
  o->shared_first_step = 1;
  o->output = OKX_OUTPUT_RECORDS;
  o->reserved = 0;
}

int32_t okx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int32_t okx_program_create(const okx_program_desc* desc, okx_program** out) {
  if (!out) return fail(OKX_ERR_INVALID, "out is null");
  *out = nullptr;
  std::unique_ptr<okx_program> owner(new (std::nothrow) okx_program);  // (a failed create frees what it had got: ~okx_program)
  okx_program* p = owner.get();
  if (!p) return fail(OKX_ERR_ALLOC, "out of host memory");
  int rc = okx::build_dev_program(desc, &p->host, g_err, (int)sizeof(g_err));
  if (rc != OKX_OK) return rc;
  p->host.lds_doubles = okx::lds_doubles(p->host);
  for (int i = 0; i < p->host.n_crows; ++i) p->line_row = p->line_row || p->host.row_type[i] == OKX_ROW_POINT_ON_LINE;
  select_solve_kernels(p);
  p->lds_bytes = sizeof(double) * (size_t)p->host.lds_doubles;
  p->solve_lds_bytes = p->lds_bytes;
  p->packed_lds_bytes = p->packed_fn ? sizeof(double) * (size_t)okx::packed_lds_doubles(p->host, p->groups) : 0;
  if (p->packed_lds_bytes > 160 * 1024) p->packed_fn = nullptr;
  if (p->lds_bytes > 160 * 1024) return fail(OKX_ERR_LIMIT, "problem needs %zu bytes of LDS (max 163840)", p->lds_bytes);
  hipError_t e = hipGetDevice(&p->device);
  if (e != hipSuccess) return fail(OKX_ERR_DEVICE, "hipGetDevice failed: %s (no GPU?)", hipGetErrorString(e));
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, p->device);
  if (e != hipSuccess) return fail(OKX_ERR_DEVICE, "hipGetDeviceProperties failed: %s", hipGetErrorString(e));
  p->n_cu = prop.multiProcessorCount;
  e = hipMalloc((void**)&p->dev, sizeof(okx::DevProgram));
  if (e != hipSuccess) {
    p->dev = nullptr;
    return fail(OKX_ERR_DEVICE, "hipMalloc failed: %s", hipGetErrorString(e));
  }
  e = hipMemcpy(p->dev, &p->host, sizeof(okx::DevProgram), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(OKX_ERR_DEVICE, "hipMemcpy failed: %s", hipGetErrorString(e));
  // >64 KiB of dynamic LDS needs the opt-in attribute.  The kernels are shared by every program of the
  // process, so the limit is raised to the hardware maximum once per kernel (a per-program size would let a
  // later, smaller program lower it under an earlier one's feet).
  for (const void* fn : {p->solve_fn, p->eval_fn, (const void*)okx::okx_rebind_kernel,
                         p->packed_fn, p->tangent_fn}) {
    if (!fn) continue;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes);
    if (e != hipSuccess)
      return fail(OKX_ERR_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed: %s", hipGetErrorString(e));
  }
  p->blocks_per_cu = resident_blocks_per_cu(p->solve_fn, p->solve_lds_bytes, p->threads);
  p->packed_blocks_per_cu = p->packed_fn ? resident_blocks_per_cu(p->packed_fn, p->packed_lds_bytes) : 0;
  okx::attach_cached_or_compile(p);
  *out = owner.release();
  return OKX_OK;
}

int32_t okx_program_ready(okx_program* p, int32_t wait) {
  if (!p) return fail(OKX_ERR_INVALID, "null program");
  attach_when_ready(p, wait != 0);
  return p->jit.load(std::memory_order_acquire) ? 0 : 1;
}

void okx_program_destroy(okx_program* p) {
  if (!p) return;
  okx::retire_jit_job(p);
  delete p;
}

const char* okx_program_kernel(const okx_program* p) {
  if (!p) return "";
  return p->quad_fn_u ? "quad" : "wave";
}

const char* okx_program_kernel_note(const okx_program* p) { return p ? p->quad_note : ""; }

/* 1 when chain heads of this program's own geometry take their first step from the shared first-step table
   (okx_solve_opts.shared_first_step with a generated head kernel): their okx_info.nfev then omits that evaluation. */
int32_t okx_program_shares_first_step(const okx_program* p) { return p && p->quad_fn_head_u ? 1 : 0; }
int32_t okx_program_has_cold_body(const okx_program* p) { return p && p->quad_fn_cold_u && p->quad_fn_head_u ? 1 : 0; }

/* Why the program has no lane kernel (empty string: it has one), and the batch size from which auto selection uses it. */
const char* okx_program_lane_note(const okx_program* p) { return p ? p->lane_note : ""; }
int64_t okx_program_lane_threshold(const okx_program* p) { return p && p->lane_fn_u ? p->lane_min_problems : -1; }
/* bit0: auto selection uses the lane kernel's independent-solve body, bit1: its chain body (0: neither / no lane kernel) */
int32_t okx_program_lane_bodies(const okx_program* p) {
  return p && p->lane_fn_u ? (p->lane_cold_ok ? 1 : 0) | (p->lane_chain_ok ? 2 : 0) : 0;
}

/* Generated source of a program's kernel of one family into the caller's buffer: the number of bytes the full text needs
   (including the terminator) or a negative okx_status. */
static int64_t generated_source(const okx_program_desc* desc, char* buf, int64_t buflen, const char* family,
                                const std::function<bool(const okx::DevProgram&, std::string*, std::string*)>& generate) {
  std::string src;
  const int rc = with_dev_program(desc, [&](const okx::DevProgram& program) {
    std::string why;
    return generate(program, &src, &why) ? (int)OKX_OK : fail(OKX_ERR_LIMIT, "no %s kernel for this program: %s", family, why.c_str());
  });
  if (rc != OKX_OK) return rc;
  if (buf && buflen > 0) {
    const size_t ncopy = src.size() < (size_t)buflen - 1 ? src.size() : (size_t)buflen - 1;
    std::memcpy(buf, src.data(), ncopy);
    buf[ncopy] = 0;
  }
  return (int64_t)src.size() + 1;
}

/* Generated source of the lane kernel for a program (no device needed); same contract as okx_quad_source. */
int64_t okx_lane_source(const okx_program_desc* desc, char* buf, int64_t buflen) {
  return generated_source(desc, buf, buflen, "lane", [](const okx::DevProgram& program, std::string* src, std::string* why) {
    return okx::lane_generate(program, src, why);
  });
}

/* Generated source of the quad kernel for a program (no device needed).  Returns the number of
   bytes the full text needs (including the terminator) or a negative okx_status. */
int64_t okx_quad_source(const okx_program_desc* desc, char* buf, int64_t buflen) {
  return generated_source(desc, buf, buflen, "quad", [](const okx::DevProgram& program, std::string* src, std::string* why) {
    return okx::quad_generate(program, quad_waves_per_simd(), src, why);
  });
}

/* Generates and compiles the quad kernel of a program into the on-disk cache (no device needed):
   what __graft_entry__.build() calls for the BASELINE topologies. */
int32_t okx_precompile(const okx_program_desc* desc) {
  return with_dev_program(desc, [](const okx::DevProgram& program) {
    std::string src, why, code;
    if (!okx::quad_build(program, quad_waves_per_simd(), &src, &code, &why))
      return fail(why.compare(0, 14, "compile failed") == 0 ? OKX_ERR_DEVICE : OKX_ERR_LIMIT, "no quad kernel for this program: %s", why.c_str());
    if (program.n_free <= okx::kQuadMaxFree) {
      // the lane kernel of the same program (programs it does not fit simply have none)
      std::string lsrc, lwhy, lcode;
      std::vector<okx::LaneOverride> overrides;  // (asked for so that the per-kernel choice is made and remembered)
      if (okx::lane_generate(program, &lsrc, &lwhy, 0) && !okx::lane_build(program, &lsrc, &lcode, &lwhy, false, nullptr, 0, false, &overrides))
        return fail(OKX_ERR_DEVICE, "lane kernel: %s", lwhy.c_str());
    }
    return (int)OKX_OK;
  });
}

/* Scratch (private segment) bytes of the solve kernels okx_precompile / okx_program_create would use for this program:
   0 means the register allocation holds everything (what every BASELINE program is expected to report). */
int32_t okx_debug_kernel_scratch(const okx_program_desc* desc, int32_t* scratch_bytes) {
  if (!scratch_bytes) return fail(OKX_ERR_INVALID, "null output pointer");
  return with_dev_program(desc, [&](const okx::DevProgram& program) {
    std::string src, why, code;
    if (!okx::quad_build(program, quad_waves_per_simd(), &src, &code, &why))
      return fail(OKX_ERR_LIMIT, "no quad kernel for this program: %s", why.c_str());
    *scratch_bytes = okx::quad_code_scratch_bytes(code, "okx_quad_solve");
    return (int)OKX_OK;
  });
}

/* The lane kernel of a program as okx_precompile / okx_program_create would build it: scratch bytes of its independent-solve
   and chain bodies and the emission variant lane_build kept (out3; no device needed). */
int32_t okx_debug_lane_scratch(const okx_program_desc* desc, int32_t* out3) {
  if (!out3) return fail(OKX_ERR_INVALID, "null output pointer");
  return with_dev_program(desc, [&](const okx::DevProgram& program) {
    std::string src, why, code;
    int variant = -1;
    std::vector<okx::LaneOverride> overrides;
    if (!okx::lane_build(program, &src, &code, &why, false, &variant, 0, false, &overrides))
      return fail(OKX_ERR_LIMIT, "no lane kernel for this program: %s", why.c_str());
    out3[0] = okx::lane_worst_scratch(code, overrides, "okx_lane_solve");
    out3[1] = okx::lane_worst_scratch(code, overrides, "okx_lane_chain");
    out3[2] = variant;
    return (int)OKX_OK;
  });
}

}  // extern "C"

namespace {

// One launch of okx_solve_batch / okx_solve_evaluated_batch (`evaluated`: the launch runs the program's evaluated kernels,
// whose epilogue writes d_tangents / d_eval).
struct SolveCall {
  okx_program* p;
  const okx_solve_opts* opts;
  int64_t n_problems;
  const double *d_targets, *d_geom_pos, *d_geom_row_param;
  double* d_out_pos;
  okx_info* d_info;
  hipStream_t stream;
  bool evaluated;
  double *d_tangents, *d_eval;
};

// which of its arrays a launch passes (okx_plan_launch: what a launch of the asked shape would pass)
struct LaunchArrays {
  bool targets, geom_pos, geom_row_param, out_pos, info, tan_or_eval;
};

// (an evaluated launch's first check, ahead of its arguments: the planner takes the evaluated kernels as given)
int32_t need_evaluation(bool enabled, const char* ev_note) {
  if (enabled) return OKX_OK;
  return fail(OKX_ERR_INVALID, "evaluated solves need okx_program_enable_evaluation first%s%s", ev_note[0] ? ": " : "", ev_note);
}

// The steps_per_geometry checks of a launch, with its messages (okx_plan_launch and okx_debug_plan_launch: the same).
int32_t check_launch_spans(long long n_problems, long long spg, bool geometry_tables) {
  if (!steps_per_geometry_fits(n_problems, spg, false)) return fail(OKX_ERR_INVALID, "n_problems must be a multiple of steps_per_geometry");
  if (geometry_tables && spg == 0) return fail(OKX_ERR_INVALID, "a geometry table needs steps_per_geometry > 0");
  return OKX_OK;
}

// Argument checks of a launch, the first failing one wins; under the program's shared lock.  OKX_OK with n_problems == 0:
// nothing to do.
int32_t validate_launch(const okx_program* p, const okx_solve_opts* opts, int64_t n_problems, bool evaluated, const LaunchArrays& has) {
  if (evaluated) {
    if (const int32_t rc = need_evaluation(p->ev_solve_u != nullptr, p->ev_note)) return rc;
    if (!has.tan_or_eval) return fail(OKX_ERR_INVALID, "an evaluated solve needs d_tangents or d_eval");
  }
  if (n_problems < 0) return fail(OKX_ERR_INVALID, "negative problem count");
  if (n_problems == 0) return OKX_OK;
  if (opts->output < OKX_OUTPUT_RECORDS || opts->output > OKX_OUTPUT_NONE) return fail(OKX_ERR_INVALID, "unknown output mode");
  if ((!has.out_pos && opts->output != OKX_OUTPUT_NONE) || !has.info) return fail(OKX_ERR_INVALID, "null output pointer");
  if (p->host.n_targets > 0 && !has.targets) return fail(OKX_ERR_INVALID, "null targets");
  if (has.geom_pos != has.geom_row_param)
    return fail(OKX_ERR_INVALID, "geometry positions and row parameters must be given together");
  if (const int32_t rc = check_launch_spans(n_problems, opts->steps_per_geometry, has.geom_pos)) return rc;
  if (opts->max_iter < 1) return fail(OKX_ERR_INVALID, "max_iter must be >= 1");
  if (!(opts->lambda0 >= 0.0) || !(opts->lambda0 < 1e300)) return fail(OKX_ERR_INVALID, "lambda0 must be finite and >= 0");
  return OKX_OK;
}

// The first-step table of a launch into q->head: the own geometry's (found or filled, okx::own_head_table) or the per-geometry
// scratch of the program, filled by okx_quad_head_g ahead of the solve.  Null: the chain heads run their own first pass.
int32_t find_head_table(const SolveCall& c, okx::QuadArgs* q) {
  okx_program* p = c.p;
  if (!c.d_geom_pos) {
    double* table = nullptr;  // own geometry: once per lambda0 (the default's at program creation), then cached
    const int rc = okx::own_head_table(p, c.opts->lambda0, c.stream, &table);
    q->head = table;  // (null: no table for this launch - see own_head_table)
    return rc;
  }
  const long long spg = c.opts->steps_per_geometry;
  // (one table row costs about 1.3 passes of one quad: with fewer than four steps per geometry, or a table beyond
  //  256 MiB, the heads run their own first pass)
  if (!(spg >= 4 && (c.n_problems / spg) * (long long)p->head_stride * 8 <= (256LL << 20))) return OKX_OK;
  const long long n_geom = c.n_problems / spg;
  if (n_geom > p->head_geom_cap) {
    // grow-only scratch, replaced in stream order: launches of this program with geometry tables are stream-ordered
    // (okx.h), so the old table's readers are ahead of the free on this stream - no device-wide synchronisation.
    // Never inside a stream capture (the allocation would become a node of the graph while the pointer is cached
    // here): a captured launch that finds the scratch too small runs without the shared first step - warm the launch
    // up once outside the capture.
    if (stream_is_capturing(c.stream)) return OKX_OK;
    if (p->head_geom_dev) {
      double* old = p->head_geom_dev;
      p->head_geom_dev = nullptr;
      p->head_geom_cap = 0;
      HIP_TRY(hipFreeAsync(old, c.stream));
    }
    const size_t bytes = sizeof(double) * (size_t)n_geom * (size_t)p->head_stride;
    double* fresh = nullptr;
    HIP_TRY(hipMallocAsync((void**)&fresh, bytes, c.stream));
    p->head_geom_dev = fresh;
    p->head_geom_cap = n_geom;
  }
  okx::QuadHeadArgs h;
  h.geom_pos = c.d_geom_pos;
  h.geom_row_param = c.d_geom_row_param;
  h.lambda0 = c.opts->lambda0;
  h.design_pos = q->design_pos;
  h.row_param = q->row_param;
  h.dop_param = q->dop_param;
  h.head = p->head_geom_dev;
  h.n_geometries = n_geom;
  void* hargs[] = {(void*)&h};
  const long long head_waves = (n_geom + p->quad_ppw - 1) / p->quad_ppw;
  const long long head_cap = (long long)p->n_cu * p->quad_waves_per_cu;
  HIP_TRY(hipModuleLaunchKernel(p->quad_fn_head_g, (int)(head_waves < head_cap ? head_waves : head_cap), 1, 1, okx::kWave, 1, 1,
                                0, c.stream, hargs, nullptr));
  q->head = p->head_geom_dev;
  return OKX_OK;
}

// Arguments of the generated kernels (quad and lane family) for this launch, its first-step table included.
int32_t generated_args(const SolveCall& c, const okx::LaunchPlan& plan, okx::QuadArgs* q, okx::QuadEvArgs* qe) {
  const okx_program* p = c.p;
  const okx_solve_opts* opts = c.opts;
  q->targets = c.d_targets;
  q->geom_pos = c.d_geom_pos;
  q->geom_row_param = c.d_geom_row_param;
  q->out_pos = c.d_out_pos;
  q->info = c.d_info;
  q->n_problems = c.n_problems;
  q->steps_per_geometry = opts->steps_per_geometry;
  q->chain_len = plan.chain_len;
  q->max_iter = opts->max_iter;
  q->confirm = plan.confirm;
  q->step_tol = opts->step_tol;
  q->grad_tol = opts->grad_tol;
  q->ftol = opts->ftol;
  q->lambda0 = opts->lambda0;
  q->residual_tolerance = opts->residual_tolerance;
  okx::set_program_tables(p, q);
  q->trace = p->quad_trace;
  q->trace_problem = p->quad_trace_problem;
  q->predictor = (opts->predictor != 0 && !c.d_geom_pos) ? p->predictor_dev : nullptr;
  q->predictor_mode = opts->predictor;
  q->predictor_len = p->predictor_len;
  q->head = nullptr;
  q->out_mode = opts->output;
  if (plan.shared_first_step)
    if (const int32_t rc = find_head_table(c, q)) return rc;
  // evaluated launches: the same arguments, then the epilogue's outputs and the roles' numbers
  qe->tan = c.d_tangents;
  qe->ev = c.d_eval;
  qe->cfg = p->ev_cfg;
  qe->cfg_r = p->ev_cfg_r;
  std::memcpy(qe->roles, p->ev_roles, sizeof(qe->roles));
  return OKX_OK;
}

int32_t launch_lane(const SolveCall& c, const okx_launch_caps& caps, const okx::LaunchPlan& plan) {
  const okx_program* p = c.p;
  okx::QuadArgs q;
  okx::QuadEvArgs qe;
  if (const int32_t rc = generated_args(c, plan, &q, &qe)) return rc;
  void* kargs[] = {c.evaluated ? (void*)&qe : (void*)&q};
  const bool cold = plan.chain_len == 1, compact = c.opts->output != OKX_OUTPUT_RECORDS;
  const int geom = c.d_geom_pos ? 1 : 0;
  hipFunction_t fn = cold ? (geom ? p->lane_fn_g : p->lane_fn_u) : (geom ? p->lane_chain_g : p->lane_chain_u);
  if (compact) fn = p->lane_compact[(cold ? 0 : 2) + geom];
  if (c.evaluated) fn = geom ? p->ev_lane_g : p->ev_lane_u;
  void* ring = nullptr;
  if (plan.start == okx::kStartNested) {
    fn = p->lane_nest[(compact ? 2 : 0) + geom];
    HIP_TRY(hipMallocAsync(&ring, sizeof(double) * (size_t)okx::lane_nest_doubles(p->host.n) * (size_t)plan.grid, c.stream));
    q.predictor = static_cast<const double*>(ring);
  } else if (!cold && okx::lane_chain_is_flat(p->host.n)) {
    // what a flat chain body carries from step to step (okx_quad.hpp lane_chain_is_flat): scratch of this launch,
    // allocated and freed in stream order (legal under stream capture, no device-wide synchronisation)
    HIP_TRY(hipMallocAsync(&ring, sizeof(double) * (size_t)okx::lane_flat_chain_doubles(p->host.n) * (size_t)plan.grid, c.stream));
    q.predictor = static_cast<const double*>(ring);
  }
  if (plan.start == okx::kStartRefined) {
    // four launches on the stream: the coarse steps (offset 0), then offsets 1, 2, 3 from their interpolant
    const int variant = (compact ? 2 : 0) + geom;
    for (int off = 0; off < 4; ++off) {
      q.chain_len = off;  // (the strided bodies read their offset here)
      HIP_TRY(hipModuleLaunchKernel(p->lane_refine[(off ? 4 : 0) + variant], okx::lane_refine_grid(caps, plan, c.n_problems, off), 1, 1,
                                    okx::kWave, 1, 1, 0, c.stream, kargs, nullptr));
    }
    return OKX_OK;
  }
  qe.q = q;
  HIP_TRY(hipModuleLaunchKernel(fn, plan.grid, 1, 1, okx::kWave, 1, 1, 0, c.stream, kargs, nullptr));
  if (ring) HIP_TRY(hipFreeAsync(ring, c.stream));
  return OKX_OK;
}

int32_t launch_quad(const SolveCall& c, const okx::LaunchPlan& plan) {
  const okx_program* p = c.p;
  okx::QuadArgs q;
  okx::QuadEvArgs qe;
  if (const int32_t rc = generated_args(c, plan, &q, &qe)) return rc;
  void* kargs[] = {c.evaluated ? (void*)&qe : (void*)&q};
  const bool cold = plan.cold_if_table && q.head != nullptr;  // (the table's availability is a launch-time fact: own_head_table)
  hipFunction_t fn;
  if (c.evaluated) fn = cold ? p->ev_cold_u : c.d_geom_pos ? p->ev_solve_g : p->ev_solve_u;
  else fn = cold ? p->quad_fn_cold_u : c.d_geom_pos ? p->quad_fn_g : p->quad_fn_u;
  qe.q = q;
  HIP_TRY(hipModuleLaunchKernel(fn, plan.grid, 1, 1, okx::kWave, 1, 1, 0, c.stream, kargs, nullptr));
  return OKX_OK;
}

// Arguments of the interpreter kernels for independent confirmed solves on the program's own geometry: a launch sets what
// differs (okx_debug_phase_profile: nothing but its counters).
okx::SolveArgs interpreter_args(const okx_solve_opts* opts, int64_t n_problems, const double* d_targets, double* d_out_pos, okx_info* d_info) {
  okx::SolveArgs a{};  // (no geometry tables, steps_per_geometry 0, no phase counters)
  a.targets = d_targets;
  a.out_pos = d_out_pos;
  a.info = d_info;
  a.n_problems = n_problems;
  a.max_iter = opts->max_iter;
  a.confirm = 1;
  a.chain_len = 1;
  a.step_tol = opts->step_tol;
  a.grad_tol = opts->grad_tol;
  a.ftol = opts->ftol;
  a.lambda0 = opts->lambda0;
  a.residual_tolerance = opts->residual_tolerance;
  return a;
}

// the interpreter kernels: one problem per wavefront, or the lane-group packed kernel
int32_t launch_interpreter(const SolveCall& c, const okx::LaunchPlan& plan) {
  const okx_program* p = c.p;
  const okx_solve_opts* opts = c.opts;
  if (opts->output != OKX_OUTPUT_RECORDS)
    return fail(OKX_ERR_INVALID, "output mode %d needs a generated kernel (this launch runs the interpreter: %s)", opts->output,
                p->quad_note[0] ? p->quad_note : "kernel option");
  okx::SolveArgs a = interpreter_args(opts, c.n_problems, c.d_targets, c.d_out_pos, c.d_info);
  a.geom_pos = c.d_geom_pos;
  a.geom_row_param = c.d_geom_row_param;
  a.steps_per_geometry = opts->steps_per_geometry;
  a.confirm = plan.confirm;
  a.chain_len = plan.chain_len;
  const okx::DevProgram* dev = p->dev;
  if (plan.family == okx::kFamilyPacked) {
    int width = p->group_width;
    void* kargs[] = {(void*)&dev, (void*)&a, (void*)&width};
    HIP_TRY(hipLaunchKernel(p->packed_fn, dim3(plan.grid), dim3(okx::kWave), kargs, p->packed_lds_bytes, c.stream));
    return OKX_OK;
  }
  void* kargs[] = {(void*)&dev, (void*)&a};
  HIP_TRY(hipLaunchKernel(p->solve_fn, dim3(plan.grid), dim3(p->threads), kargs, p->lds_bytes, c.stream));
  return OKX_OK;
}

// validate, read the program's capabilities, plan, launch
int32_t solve_impl(const SolveCall& c) {
  okx_program* p = c.p;
  if (!p || !c.opts) return fail(OKX_ERR_INVALID, "null program or options");
  attach_when_ready(p, false, &c.stream);
  std::shared_lock<std::shared_mutex> kernels(p->kern_mutex);
  const LaunchArrays has = {c.d_targets != nullptr, c.d_geom_pos != nullptr, c.d_geom_row_param != nullptr, c.d_out_pos != nullptr,
                            c.d_info != nullptr, c.d_tangents || c.d_eval};
  const int32_t rc = validate_launch(p, c.opts, c.n_problems, c.evaluated, has);
  if (rc != OKX_OK || c.n_problems == 0) return rc;
  okx_launch_caps caps;
  fill_launch_caps(p, &caps);
  okx::LaunchPlan plan;
  if (okx::plan_launch(caps, okx::launch_request(*c.opts, c.n_problems, has.geom_pos, c.evaluated), p->quad_note, p->lane_note, p->ev_note, &plan))
    return fail(plan.status, "%s", plan.message);
  if (plan.family == okx::kFamilyLane) return launch_lane(c, caps, plan);
  if (plan.family == okx::kFamilyQuad) return launch_quad(c, plan);
  return launch_interpreter(c, plan);
}

}  // namespace

extern "C" {

int32_t okx_solve_batch(okx_program* p, const okx_solve_opts* opts, int64_t n_problems,
                        const double* d_targets, const double* d_geom_pos,
                        const double* d_geom_row_param, double* d_out_pos, okx_info* d_info,
                        void* stream) {
  return solve_impl({p, opts, n_problems, d_targets, d_geom_pos, d_geom_row_param, d_out_pos, d_info, (hipStream_t)stream, false, nullptr, nullptr});
}

int32_t okx_solve_evaluated_batch(okx_program* p, const okx_solve_opts* opts, int64_t n_problems,
                                  const double* d_targets, const double* d_geom_pos, const double* d_geom_row_param,
                                  double* d_out_pos, okx_info* d_info, double* d_tangents, double* d_eval, void* stream) {
  return solve_impl({p, opts, n_problems, d_targets, d_geom_pos, d_geom_row_param, d_out_pos, d_info, (hipStream_t)stream, true, d_tangents, d_eval});
}

static void report_plan(const okx::LaunchPlan& plan, int32_t* family, int32_t* chain_len) {
  *family = plan.family;
  *chain_len = plan.start == okx::kStartNested ? -1 : (int32_t)(plan.chain_len > 0x7fffffffll ? 0x7fffffffll : plan.chain_len);
}

int32_t okx_plan_launch(okx_program* p, const okx_solve_opts* opts, int64_t n_problems, int32_t geometry_tables, int32_t evaluated,
                        int32_t* out2) {
  if (!out2) return fail(OKX_ERR_INVALID, "null output pointer");
  out2[0] = out2[1] = 0;
  if (n_problems <= 0) return fail(OKX_ERR_INVALID, "a launch plan needs a positive problem count");
  if (!p || !opts) return fail(OKX_ERR_INVALID, "null program or options");
  const hipStream_t no_stream = nullptr;
  attach_when_ready(p, false, &no_stream);
  std::shared_lock<std::shared_mutex> kernels(p->kern_mutex);
  const bool geom = geometry_tables != 0;
  if (const int32_t rc = validate_launch(p, opts, n_problems, evaluated != 0, {true, geom, geom, true, true, true})) return rc;
  okx_launch_caps caps;
  fill_launch_caps(p, &caps);
  okx::LaunchPlan plan;
  if (okx::plan_launch(caps, okx::launch_request(*opts, n_problems, geom, evaluated != 0), p->quad_note, p->lane_note, p->ev_note, &plan))
    return fail(plan.status, "%s", plan.message);
  report_plan(plan, &out2[0], &out2[1]);
  return OKX_OK;
}

/* Test hooks (okx_debug.h): the planner on caller-made capabilities, and the capabilities the launch path fills itself. */
static thread_local char g_plan_notes[3][64];  // what okx_debug_plan_launch passes for a program's quad_note, lane_note, ev_note

void okx_debug_plan_notes(const char* quad_note, const char* lane_note, const char* ev_note) {
  const char* notes[3] = {quad_note, lane_note, ev_note};
  for (int k = 0; k < 3; ++k) std::snprintf(g_plan_notes[k], sizeof(g_plan_notes[k]), "%s", notes[k] ? notes[k] : "");
}

int32_t okx_debug_plan_launch(const okx_launch_caps* caps, const okx_solve_opts* opts, int64_t n_problems, int32_t geometry_tables,
                              int32_t evaluated, int32_t* out6) {
  if (!caps || !opts || !out6) return fail(OKX_ERR_INVALID, "null pointer");
  for (int k = 0; k < 6; ++k) out6[k] = 0;
  if (n_problems <= 0) return fail(OKX_ERR_INVALID, "a launch plan needs a positive problem count");
  if (evaluated)
    if (const int32_t rc = need_evaluation(caps->ev_enabled != 0, g_plan_notes[2])) return rc;
  if (const int32_t rc = check_launch_spans(n_problems, opts->steps_per_geometry, geometry_tables != 0)) return rc;
  if (caps->n_cu < 1 || (caps->has_quad && (caps->quad_ppw < 1 || caps->quad_waves_per_cu < 1)) || (caps->has_packed && caps->groups < 1))
    return fail(OKX_ERR_INVALID, "capabilities name a kernel without its launch sizes");
  okx::LaunchPlan plan;
  if (okx::plan_launch(*caps, okx::launch_request(*opts, n_problems, geometry_tables != 0, evaluated != 0), g_plan_notes[0], g_plan_notes[1], g_plan_notes[2], &plan))
    return fail(plan.status, "%s", plan.message);
  report_plan(plan, &out6[0], &out6[1]);
  out6[2] = plan.start;
  out6[3] = plan.auto_cold ? 1 : 0;
  out6[4] = plan.confirm;
  out6[5] = plan.grid;
  return OKX_OK;
}

int32_t okx_debug_plan_evaluate(const okx_launch_caps* caps, int64_t n_problems, int64_t steps_per_geometry, int32_t* out2) {
  if (!caps || !out2) return fail(OKX_ERR_INVALID, "null pointer");
  if (n_problems <= 0 || steps_per_geometry < 0 || (steps_per_geometry > 0 && n_problems % steps_per_geometry != 0))
    return fail(OKX_ERR_INVALID, "bad steps_per_geometry");
  long long units = 0;
  out2[0] = okx::evaluate_on_lane(*caps, n_problems, steps_per_geometry, &units) ? 1 : 0;
  out2[1] = (int32_t)(units > 0x7fffffffll ? 0x7fffffffll : units);
  return OKX_OK;
}

int32_t okx_debug_program_caps(okx_program* p, okx_launch_caps* caps) {
  if (!p || !caps) return fail(OKX_ERR_INVALID, "null pointer");
  attach_when_ready(p, false);
  std::shared_lock<std::shared_mutex> kernels(p->kern_mutex);
  fill_launch_caps(p, caps);
  return OKX_OK;
}

/* The interpreter's evaluation kernel at d_x: residuals, and the Jacobian (okx_eval_batch) or the normal equations
   (okx_debug_normal_equations). */
static int32_t launch_eval(okx_program* p, okx::EvalArgs a, void* stream) {
  const okx::DevProgram* dev = p->dev;
  void* kargs[] = {(void*)&dev, (void*)&a};
  HIP_TRY(hipLaunchKernel(p->eval_fn, dim3(grid_for(p, a.n_problems)), dim3(p->threads), kargs, p->lds_bytes,
                          (hipStream_t)stream));
  return OKX_OK;
}

int32_t okx_eval_batch(okx_program* p, int64_t n_problems, const double* d_x,
                       const double* d_targets, double* d_r, double* d_jac, void* stream) {
  if (!p) return fail(OKX_ERR_INVALID, "null program");
  if (n_problems <= 0) return n_problems == 0 ? OKX_OK : fail(OKX_ERR_INVALID, "negative count");
  if (!d_x || !d_r) return fail(OKX_ERR_INVALID, "null pointer");
  return launch_eval(p, {d_x, d_targets, d_r, d_jac, nullptr, nullptr, n_problems}, stream);
}

/* Test hook (not part of the reference boundary): J^T J and J^T r as the solver forms them. */
int32_t okx_debug_normal_equations(okx_program* p, int64_t n_problems, const double* d_x,
                                   const double* d_targets, double* d_r, double* d_ata,
                                   double* d_atr, void* stream) {
  if (!p || !d_x || !d_r) return fail(OKX_ERR_INVALID, "null pointer");
  if (n_problems <= 0) return OKX_OK;
  return launch_eval(p, {d_x, d_targets, d_r, nullptr, d_ata, d_atr, n_problems}, stream);
}

int32_t okx_rebind_design(okx_program* p, int64_t n_geometries, const double* d_hardpoints,
                          double* d_geom_pos, double* d_geom_row_param, void* stream) {
  if (!p) return fail(OKX_ERR_INVALID, "null program");
  if (n_geometries <= 0) return n_geometries == 0 ? OKX_OK : fail(OKX_ERR_INVALID, "negative count");
  if (!d_hardpoints || !d_geom_pos || !d_geom_row_param) return fail(OKX_ERR_INVALID, "null pointer");
  okx::RebindArgs a;
  a.hardpoints = d_hardpoints;
  a.geom_pos = d_geom_pos;
  a.geom_row_param = d_geom_row_param;
  a.n_geometries = n_geometries;
  hipLaunchKernelGGL(okx::okx_rebind_kernel, dim3(grid_for(p, n_geometries)), dim3(okx::kWave),
                     p->lds_bytes, (hipStream_t)stream, (const okx::DevProgram*)p->dev, a);
  HIP_TRY(hipGetLastError());
  return OKX_OK;
}

int32_t okx_expand_positions_batch(okx_program* p, int64_t n_problems, int64_t steps_per_geometry, const double* d_free,
                                   const double* d_geom_pos, double* d_out_pos, void* stream) {
  if (!p) return fail(OKX_ERR_INVALID, "null program");
  {
    const hipStream_t launch_stream = (hipStream_t)stream;
    attach_when_ready(p, false, &launch_stream);
  }
  std::shared_lock<std::shared_mutex> kernels(p->kern_mutex);
  if (n_problems < 0) return fail(OKX_ERR_INVALID, "negative problem count");
  if (n_problems == 0) return OKX_OK;
  if (!d_free || !d_out_pos) return fail(OKX_ERR_INVALID, "null pointer");
  if (!steps_per_geometry_fits(n_problems, steps_per_geometry, d_geom_pos != nullptr)) return fail(OKX_ERR_INVALID, "bad steps_per_geometry");
  if (p->quad_fn_expand) {  // generated form: 16 states per wavefront, coalesced records
    okx::QuadExpandArgs q;
    q.free = d_free;
    q.geom_pos = d_geom_pos;
    q.out_pos = d_out_pos;
    q.n_problems = n_problems;
    q.steps_per_geometry = steps_per_geometry > 0 ? steps_per_geometry : n_problems;
    okx::set_program_tables(p, &q);
    const long long waves = (n_problems + p->quad_ppw - 1) / p->quad_ppw;
    // (pair mode: a persistent grid - the wavefront reads its fixed points once and walks its wave units)
    const long long grid_cap = p->quad_ppw == 8 ? (long long)p->n_cu * 32 : 65536;
    void* kargs[] = {(void*)&q};
    HIP_TRY(hipModuleLaunchKernel(p->quad_fn_expand, (int)(waves < grid_cap ? waves : grid_cap), 1, 1, okx::kWave, 1, 1, 0,
                                  (hipStream_t)stream, kargs, nullptr));
    return OKX_OK;
  }
  okx::ExpandArgs a;
  a.free = d_free;
  a.geom_pos = d_geom_pos;
  a.out_pos = d_out_pos;
  a.n_problems = n_problems;
  a.steps_per_geometry = steps_per_geometry > 0 ? steps_per_geometry : n_problems;
  const long long blocks = (n_problems + okx::kExpandThreads - 1) / okx::kExpandThreads;
  if (blocks > 0x7fffffffll) return fail(OKX_ERR_INVALID, "too many problems for one launch");
  // derived positions [3 n_derived][64] and the point -> source table
  const size_t expand_lds = sizeof(double) * 3 * p->host.n_derived * okx::kExpandThreads + sizeof(int) * p->host.n_points;
  hipLaunchKernelGGL(okx::okx_expand_kernel, dim3((unsigned)blocks), dim3(okx::kExpandThreads), expand_lds, (hipStream_t)stream,
                     (const okx::DevProgram*)p->dev, a);
  HIP_TRY(hipGetLastError());
  return OKX_OK;
}

int32_t okx_tangent_batch(okx_program* p, int64_t n_problems, int64_t steps_per_geometry, const double* d_pos,
                          const double* d_geom_pos, const double* d_geom_row_param, double* d_tangents,
                          okx_tangent_info* d_tinfo, void* stream) {
  if (!p) return fail(OKX_ERR_INVALID, "null program");
  {
    const hipStream_t launch_stream = (hipStream_t)stream;
    attach_when_ready(p, false, &launch_stream);
  }
  std::shared_lock<std::shared_mutex> kernels(p->kern_mutex);
  if (n_problems < 0) return fail(OKX_ERR_INVALID, "negative problem count");
  if (n_problems == 0) return OKX_OK;
  if (!d_pos || !d_tangents || !d_tinfo) return fail(OKX_ERR_INVALID, "null pointer");
  if (!geometry_tables_paired(d_geom_pos, d_geom_row_param))
    return fail(OKX_ERR_INVALID, "geometry positions and row parameters must be given together");
  if (!steps_per_geometry_fits(n_problems, steps_per_geometry, d_geom_pos != nullptr)) return fail(OKX_ERR_INVALID, "bad steps_per_geometry");
  if (p->host.n_targets == 0) return OKX_OK;
  if (!p->quad_fn_tan_u || okx::dev_switch("tangent_generic")) {  // (tests: the interpreter's tangent kernel on a program with a generated one)
    // generic interpreter form: one wavefront per state (programs without a quad kernel)
    okx::TangentArgs t;
    t.pos = d_pos;
    t.geom_pos = d_geom_pos;
    t.geom_row_param = d_geom_row_param;
    t.tan = d_tangents;
    t.tinfo = d_tinfo;
    t.n_problems = n_problems;
    t.steps_per_geometry = steps_per_geometry;
    for (int k = 0; k < p->host.n_free; ++k) {
      t.free_out[k] = -1;
      for (int o = 0; o < p->host.n_out; ++o)
        if (p->host.out_point[o] == p->host.free_point[k]) t.free_out[k] = o;
      if (t.free_out[k] < 0)
        return fail(OKX_ERR_INVALID, "tangents need every free point among the output points (point %d is not)",
                    p->host.free_point[k]);
    }
    const size_t lds = p->lds_bytes + sizeof(double) * 3 * (size_t)p->host.n_points;
    if (lds > 160 * 1024) return fail(OKX_ERR_LIMIT, "tangent kernel needs %zu bytes of LDS", lds);
    const okx::DevProgram* dev = p->dev;
    void* kargs[] = {(void*)&dev, (void*)&t};
    HIP_TRY(hipLaunchKernel(p->tangent_fn, dim3(grid_for(p, n_problems)), dim3(p->threads), kargs, lds,
                            (hipStream_t)stream));
    return OKX_OK;
  }
  okx::QuadTanArgs q;
  q.pos = d_pos;
  q.geom_pos = d_geom_pos;
  q.geom_row_param = d_geom_row_param;
  q.tan = d_tangents;
  q.tinfo = d_tinfo;
  q.n_problems = n_problems;
  q.steps_per_geometry = steps_per_geometry;
  okx::set_program_tables(p, &q);
  const long long waves = (n_problems + p->quad_ppw - 1) / p->quad_ppw;
  const long long cap = (long long)p->n_cu * p->quad_waves_per_cu;
  void* kargs[] = {(void*)&q};
  HIP_TRY(hipModuleLaunchKernel(d_geom_pos ? p->quad_fn_tan_g : p->quad_fn_tan_u, (int)(waves < cap ? waves : cap), 1, 1,
                                okx::kWave, 1, 1, 0, (hipStream_t)stream, kargs, nullptr));
  return OKX_OK;
}

/* Diagnostic (okx_debug.h): record the LM passes of ONE problem of this program's subsequent quad-kernel
   solves into d_trace [256][8] = (mode, trial cost, accepted cost, lambda, step, gain ratio, accepted, done);
   pass a null pointer to switch it off. */
int32_t okx_debug_quad_trace(okx_program* p, double* d_trace, int64_t problem) {
  if (!p) return fail(OKX_ERR_INVALID, "null program");
  p->quad_trace = d_trace;
  p->quad_trace_problem = d_trace ? problem : -1;
  return OKX_OK;
}

/* okx_debug_quad_eval / okx_debug_lane_eval: the parity kernel of the quad or the lane family, 16 or 64 problems per
   wavefront, at most 4096 or 1024 workgroups. */
static int32_t debug_generated_eval(okx_program* p, bool lane, int64_t n_problems, const double* d_x, const double* d_targets, double lambda,
                                    double* d_r, double* d_ata, double* d_atr, double* d_dx, void* stream) {
  if (!p || !d_x || !d_r || !d_ata || !d_atr || !d_dx) return fail(OKX_ERR_INVALID, "null pointer");
  attach_when_ready(p, false);
  std::shared_lock<std::shared_mutex> kernels(p->kern_mutex);
  const hipFunction_t fn = lane ? p->lane_fn_eval : p->quad_fn_eval;
  if (!fn) return fail(OKX_ERR_INVALID, "no %s kernel: %s", lane ? "lane" : "quad", lane ? p->lane_note : p->quad_note);
  if (n_problems <= 0) return OKX_OK;
  const int per_wave = lane ? 64 : 16, max_grid = lane ? 1024 : 4096;
  okx::QuadEvalArgs q = {d_x, d_targets, d_r, d_ata, d_atr, d_dx, lambda, n_problems};
  okx::set_program_tables(p, &q);
  const long long waves = (n_problems + per_wave - 1) / per_wave;
  void* kargs[] = {(void*)&q};
  HIP_TRY(hipModuleLaunchKernel(fn, (int)(waves < max_grid ? waves : max_grid), 1, 1, okx::kWave, 1, 1, 0,
                                (hipStream_t)stream, kargs, nullptr));
  return OKX_OK;
}

/* Test hook: what the quad kernel's straight-line code computes at given free vectors d_x [B][n]:
   d_r [B][m], d_ata [B][n][n] (each structurally non-zero off-diagonal block is written ONCE, on one side of the
   diagonal, and the diagonal blocks in full: clear the
   buffer first), d_atr [B][n] and the damped step d_dx [B][n] = -(J^T J + lambda I)^-1 J^T r from
   its LDL^T (NaN when a pivot is not positive). */
int32_t okx_debug_quad_eval(okx_program* p, int64_t n_problems, const double* d_x, const double* d_targets,
                            double lambda, double* d_r, double* d_ata, double* d_atr, double* d_dx,
                            void* stream) {
  return debug_generated_eval(p, false, n_problems, d_x, d_targets, lambda, d_r, d_ata, d_atr, d_dx, stream);
}

/* Test hook: okx_debug_quad_eval's quantities as the LANE kernel's straight-line code computes them. */
int32_t okx_debug_lane_eval(okx_program* p, int64_t n_problems, const double* d_x, const double* d_targets,
                            double lambda, double* d_r, double* d_ata, double* d_atr, double* d_dx,
                            void* stream) {
  return debug_generated_eval(p, true, n_problems, d_x, d_targets, lambda, d_r, d_ata, d_atr, d_dx, stream);
}

/* Diagnostic (not part of the reference boundary): same as okx_solve_batch for an n = 18
   program, but runs the stamped kernel instantiation and returns per-phase cycle sums of
   workgroup 0 in d_phase_cycles[12]: 0 staging, 1 problem setup, 2 x->pos + derived points,
   3 rows, 4 reductions + LM logic, 5 normal equations, 6 factorisation, 7 substitutions,
   8 output. */
int32_t okx_debug_phase_profile(okx_program* p, const okx_solve_opts* opts, int64_t n_problems,
                                const double* d_targets, double* d_out_pos, okx_info* d_info,
                                unsigned long long* d_phase_cycles, void* stream) {
  if (!p || !opts || p->nreg != 18) return fail(OKX_ERR_INVALID, "phase profile needs an n = 18 program");
  okx::SolveArgs a = interpreter_args(opts, n_problems, d_targets, d_out_pos, d_info);
  a.phase_cycles = d_phase_cycles;
  const okx::DevProgram* dev = p->dev;
  if (p->groups == 3 && opts->kernel == 2) {
    int width = p->group_width;
    void* kargs[] = {(void*)&dev, (void*)&a, (void*)&width};
    packed_kernel_t fn = okx::okx_solve_packed_kernel<18, 3, true>;
    HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes));
    HIP_TRY(hipLaunchKernel((const void*)fn, dim3(grid_for(p, (n_problems + 2) / 3)), dim3(okx::kWave),
                            kargs, p->packed_lds_bytes, (hipStream_t)stream));
    return OKX_OK;
  }
  void* kargs[] = {(void*)&dev, (void*)&a};
  solve_kernel_t fn = okx::okx_solve_kernel<18, true>;
  HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes));
  HIP_TRY(hipLaunchKernel((const void*)fn, dim3(grid_for(p, n_problems)), dim3(okx::kWave), kargs,
                          p->lds_bytes, (hipStream_t)stream));
  return OKX_OK;
}

/* Plan introspection for CPU-side tests: fills counts without touching a device. */
int32_t okx_debug_plan_stats(const okx_program_desc* desc, int32_t* out8) {
  return with_dev_program(desc, [&](const okx::DevProgram& program) {
    if (!out8) return (int)OKX_OK;
    out8[0] = program.n;
    out8[1] = program.m;
    out8[2] = program.n_pairs;
    out8[3] = program.pair_start[program.n_pairs];
    out8[4] = program.n_active;
    out8[5] = program.js_stride;
    out8[6] = program.lda;
    out8[7] = okx::lds_doubles(program) * 8;
    return (int)OKX_OK;
  });
}

}  // extern "C"
