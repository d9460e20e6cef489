// okx_attach.cpp — the generated kernels of a program: the compile job, the switch-over, module loads, first-step tables.
// Host code on the HIP runtime API only (no kernel is named here): built as plain C++, like okx_jit.cpp.
#include "okx_program.hpp"

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <new>

namespace okx {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int quad_waves_per_simd() {
  // (developer switch quad_two_waves: __launch_bounds__(64, 2), i.e. at most 256 registers per lane - what a second resident
  //  wavefront per SIMD would need; profiles/r05/EXPERIMENTS.md section 4 has what the compiler makes of it)
  return okx::dev_switch("quad_two_waves") ? 2 : 1;
}

// The first-step table of the program's own geometry for `lambda0`: found, or filled by one wavefront of okx_quad_head_u
// on `stream` (a new buffer per lambda0: an older table may still be read by launches in flight).  A launch on another
// stream than the one that filled the table waits for the fill's event.
constexpr size_t kMaxHeadTables = 16;  // distinct lambda0 values with a table of their own per program

// true while `stream` records into a HIP graph: nothing may be allocated, filled or waited for on its behalf then
bool stream_is_capturing(hipStream_t stream) {
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &status) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return status != hipStreamCaptureStatusNone;
}

// *table = nullptr with OKX_OK: no table for this launch (the chain heads take their own first pass): a launch that is
// being captured into a graph and finds no table of its lambda0 yet, or a program whose table list is full.
int own_head_table(okx_program* p, double lambda0, hipStream_t stream, double** table) {
  *table = nullptr;
  std::lock_guard<std::mutex> lock(p->head_mutex);
  const bool capturing = stream_is_capturing(stream);
  for (okx_program::HeadTable& t : p->head_tables)
    if (t.lambda0 == lambda0) {
      // (always ordered behind the fill: an event that has completed costs nothing, and a stream handle can be reused.
      //  Under capture the wait would become a graph dependency on an event outside the graph: the table of a captured
      //  launch must have been filled before the capture began - okx_program_create fills the default's synchronously.)
      if (!capturing) HIP_TRY(hipStreamWaitEvent(stream, t.ready, 0));
      *table = t.dev;
      return OKX_OK;
    }
  if (capturing || p->head_tables.size() >= kMaxHeadTables) return OKX_OK;
  okx_program::HeadTable t;
  t.lambda0 = lambda0;
  t.filled_on = stream;
  HIP_TRY(hipMalloc((void**)&t.dev, sizeof(double) * ((size_t)p->head_stride + 2)));  // (+ pad: the cold body reads the table in 16-byte pieces)
  if (hipEventCreateWithFlags(&t.ready, hipEventDisableTiming) != hipSuccess) {
    (void)hipFree(t.dev);
    return fail(OKX_ERR_DEVICE, "hipEventCreate failed");
  }
  okx::QuadHeadArgs h;
  h.geom_pos = nullptr;
  h.geom_row_param = nullptr;
  h.head = t.dev;
  h.n_geometries = 1;
  h.lambda0 = lambda0;
  set_program_tables(p, &h);
  void* hargs[] = {(void*)&h};
  hipError_t e = hipModuleLaunchKernel(p->quad_fn_head_u, 1, 1, 1, okx::kWave, 1, 1, 0, stream, hargs, nullptr);
  if (e == hipSuccess) e = hipEventRecord(t.ready, stream);
  if (e != hipSuccess) {
    (void)hipEventDestroy(t.ready);
    (void)hipFree(t.dev);
    return fail(OKX_ERR_DEVICE, "first-step table: %s", hipGetErrorString(e));
  }
  p->head_tables.push_back(t);
  *table = t.dev;
  return OKX_OK;
}

// Generate, compile (or fetch from the cache) and load the kernel specialised to this program.
// Failure is not an error of okx_program_create: the generic kernels stay in charge and
// okx_program_kernel_note() says why.
// `cache_only`: only what the kernel cache already holds (okx_program_create); a miss sets *pending and leaves the
// interpreter kernels in charge until the compile job has filled the cache.
// `job`: the compile job's results (switch-over): the code object comes from memory, the compiler is never run here.
void attach_quad_kernel(okx_program* p, bool cache_only, bool* pending, const okx_program::JitJob* job) {
  p->quad_mod = nullptr;
  p->quad_fn_u = p->quad_fn_g = nullptr;
  p->quad_fn_cold_u = nullptr;
  p->quad_fn_eval = nullptr;
  p->quad_fn_expand = nullptr;
  p->quad_fn_tan_u = p->quad_fn_tan_g = nullptr;
  p->quad_waves_per_cu = 0;
  p->quad_ppw = p->host.n_free > okx::kQuadMaxFree ? 8 : 16;
  p->quad_note[0] = 0;
  if (okx::dev_switch("no_quad")) {  // (tests: the interpreter kernels on a program that has generated ones)
    std::snprintf(p->quad_note, sizeof(p->quad_note), "disabled by OKX_DEV=no_quad");
    return;
  }
  std::string src, why, code;
  if (job) {
    if (!job->quad_ok) {
      std::snprintf(p->quad_note, sizeof(p->quad_note), "not generated: %.200s", job->quad_why.c_str());
      if (getenv("OKX_VERBOSE")) std::fprintf(stderr, "okx: quad kernel: %s\n", job->quad_why.c_str());
      return;
    }
    code = job->quad_code;
  } else if (!okx::quad_build(p->host, quad_waves_per_simd(), &src, &code, &why, false, cache_only)) {
    if (cache_only && why == okx::kNotCached) {
      if (pending) *pending = true;
      std::snprintf(p->quad_note, sizeof(p->quad_note), "being compiled (the interpreter kernels serve the program until then)");
      return;
    }
    std::snprintf(p->quad_note, sizeof(p->quad_note), "not generated: %.200s", why.c_str());
    if (getenv("OKX_VERBOSE")) std::fprintf(stderr, "okx: quad kernel: %s\n", why.c_str());
    return;
  }
  hipModule_t mod = nullptr;
  hipError_t e = hipModuleLoadData(&mod, code.data());
  if (e != hipSuccess && !job) {
    // a damaged cache entry (truncated file, other toolchain): rebuild it once
    (void)hipGetLastError();
    if (okx::quad_build(p->host, quad_waves_per_simd(), &src, &code, &why, true)) e = hipModuleLoadData(&mod, code.data());
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    std::snprintf(p->quad_note, sizeof(p->quad_note), "hipModuleLoadData: %s", hipGetErrorString(e));
    return;
  }
  hipFunction_t fu = nullptr, fg = nullptr;
  if (hipModuleGetFunction(&fu, mod, "okx_quad_solve_u") != hipSuccess ||
      hipModuleGetFunction(&fg, mod, "okx_quad_solve_g") != hipSuccess) {
    (void)hipModuleUnload(mod);
    std::snprintf(p->quad_note, sizeof(p->quad_note), "kernel symbols missing in the code object");
    return;
  }
  int regs = 0;
  int per_simd = quad_waves_per_simd();
  if (hipFuncGetAttribute(&regs, HIP_FUNC_ATTRIBUTE_NUM_REGS, fg) == hipSuccess && regs > 0) {
    const int alloc = (regs + 7) / 8 * 8;
    per_simd = 512 / alloc;
    if (per_simd > 8) per_simd = 8;
    if (per_simd < 1) per_simd = 1;
  }
  p->quad_mod = mod;
  p->quad_fn_g = fg;
  if (hipModuleGetFunction(&p->quad_fn_eval, mod, "okx_quad_eval") != hipSuccess) p->quad_fn_eval = nullptr;
  if (hipModuleGetFunction(&p->quad_fn_expand, mod, "okx_quad_expand") != hipSuccess) p->quad_fn_expand = nullptr;
  if (hipModuleGetFunction(&p->quad_fn_tan_u, mod, "okx_quad_tangent_u") != hipSuccess ||
      hipModuleGetFunction(&p->quad_fn_tan_g, mod, "okx_quad_tangent_g") != hipSuccess)
    p->quad_fn_tan_u = p->quad_fn_tan_g = nullptr;
  p->quad_fn_head_u = p->quad_fn_head_g = nullptr;
  if (hipModuleGetFunction(&p->quad_fn_cold_u, mod, "okx_quad_cold_u") != hipSuccess) p->quad_fn_cold_u = nullptr;
  p->head_stride = okx::quad_head_stride(p->host);
  if (!(p->head_stride > 0 && hipModuleGetFunction(&p->quad_fn_head_u, mod, "okx_quad_head_u") == hipSuccess &&
        hipModuleGetFunction(&p->quad_fn_head_g, mod, "okx_quad_head_g") == hipSuccess))
    p->quad_fn_head_u = p->quad_fn_head_g = nullptr;
  (void)hipGetLastError();  // optional kernels absent from a module must not leave a sticky error behind
  p->quad_waves_per_cu = 4 * per_simd;
  // The first-step table of the program's own geometry for the default damping belongs to the program's set-up, like the
  // kernel itself: filled here (one wavefront, ~10 us) on a private non-blocking stream that is waited for before this
  // returns - no solve launch ever pays for it, a later stream capture finds it complete, and nothing is ordered against
  // the legacy stream (a synchronise there would serialise every blocking stream of the process).
  if (p->quad_fn_head_u) {
    okx_solve_opts o;
    okx_default_opts(&o);
    double* unused = nullptr;
    hipStream_t fill = nullptr;
    bool ok = hipStreamCreateWithFlags(&fill, hipStreamNonBlocking) == hipSuccess;
    ok = ok && own_head_table(p, o.lambda0, fill, &unused) == OKX_OK && hipStreamSynchronize(fill) == hipSuccess;
    if (fill) (void)hipStreamDestroy(fill);
    if (!ok) {
      (void)hipGetLastError();
      p->quad_fn_head_u = p->quad_fn_head_g = nullptr;
    }
  }
  // the gate every launch path tests, published last (a program may be switched over while it is in use)
  std::atomic_thread_fence(std::memory_order_release);
  p->quad_fn_u = fu;
}

// The lane kernel of a program that has a quad kernel (same policy: failure only means the quad kernel serves every
// batch size; okx_program_lane_note() says why).
// Largest scratch among the four kernels `prefix`_u / _u_c / _g / _g_c as they will be launched: a kernel that spills less in
// another emission variant's module is taken from there (okx::LaneOverride).
int lane_worst_scratch(const std::string& code, const std::vector<okx::LaneOverride>& overrides, const char* prefix) {
  int worst = -1;
  for (const char* tail : {"_u", "_u_c", "_g", "_g_c"}) {
    const std::string kernel = std::string(prefix) + tail;
    int sc = okx::quad_code_kernel_scratch_bytes(code, kernel.c_str());
    for (const okx::LaneOverride& o : overrides)
      if (o.kernel == kernel && o.scratch >= 0) sc = o.scratch;
    if (sc > worst) worst = sc;
  }
  return worst;
}

// The lane module's optional start modes: the nested one and the coarse-to-fine one (null slots: none).
static void attach_lane_start_modes(okx_program* p, hipModule_t mod, const std::string& code) {
  // the nested start mode (chain_len = -1 on large sweeps): kept while it does not spill more than the independent-solve body may
  static const char* const kNest[4] = {"okx_lane_nest_u", "okx_lane_nest_g", "okx_lane_nest_u_c", "okx_lane_nest_g_c"};
  p->lane_nest_scratch = okx::quad_code_scratch_bytes(code, "okx_lane_nest");
  for (int k = 0; k < 4; ++k)
    if (hipModuleGetFunction(&p->lane_nest[k], mod, kNest[k]) != hipSuccess) {
      (void)hipGetLastError();
      p->lane_nest[k] = nullptr;
    }
  if (p->lane_nest_scratch < 0 || p->lane_nest_scratch > (okx::dev_switch("lane_timeline") ? 1 << 20 : 256) || !p->lane_nest[0] || !p->lane_nest[1] || !p->lane_nest[2] || !p->lane_nest[3])
    p->lane_nest[0] = p->lane_nest[1] = p->lane_nest[2] = p->lane_nest[3] = nullptr;
  {  // coarse-to-fine start: present only in modules generated with the developer switch
    static const char* const kRefine[8] = {"okx_lane_refc_u", "okx_lane_refc_g", "okx_lane_refc_u_c", "okx_lane_refc_g_c",
                                           "okx_lane_refw_u", "okx_lane_refw_g", "okx_lane_refw_u_c", "okx_lane_refw_g_c"};
    bool all = true;
    for (int k = 0; k < 8; ++k)
      if (hipModuleGetFunction(&p->lane_refine[k], mod, kRefine[k]) != hipSuccess) {
        (void)hipGetLastError();
        all = false;
      }
    const int refine_scratch = all ? okx::quad_code_scratch_bytes(code, "okx_lane_ref") : -1;
    if (!all || refine_scratch < 0 || refine_scratch > 512)
      for (int k = 0; k < 8; ++k) p->lane_refine[k] = nullptr;
  }
}

void attach_lane_kernel(okx_program* p, bool cache_only, bool* pending, const okx_program::JitJob* job) {
  p->lane_mod = nullptr;
  p->lane_fn_u = p->lane_fn_g = p->lane_fn_eval = nullptr;
  p->lane_chain_u = p->lane_chain_g = nullptr;
  p->lane_nest[0] = p->lane_nest[1] = p->lane_nest[2] = p->lane_nest[3] = nullptr;
  p->lane_note[0] = 0;
  // The quad kernel runs 16 problems per wavefront, one wavefront per SIMD: up to n_cu * 4 * 16 problems (16384) are ONE
  // round of it (~21 us for the double wishbone).  One problem more is a second round (~38 us), while the lane kernel
  // takes 25 ... 29 us for anything up to n_cu * 4 * 64 problems (profiles/r03/EXPERIMENTS.md): auto selection switches there.
  p->lane_min_problems = (long long)p->n_cu * 4 * 16 + 1;
  if (!p->quad_fn_u || p->quad_ppw != 16) {
    std::snprintf(p->lane_note, sizeof(p->lane_note), "no single-mode quad kernel to share first-step tables with");
    return;
  }
  if (okx::dev_switch("no_lane")) {
    std::snprintf(p->lane_note, sizeof(p->lane_note), "disabled by OKX_DEV=no_lane");
    return;
  }
  std::string src, why, code;
  std::vector<okx::LaneOverride> overrides;
  if (job) {
    if (!job->lane_ok) {
      std::snprintf(p->lane_note, sizeof(p->lane_note), "not generated: %.200s", job->lane_why.c_str());
      return;
    }
    code = job->lane_code;
    overrides = job->lane_overrides;
  } else if (!okx::lane_build(p->host, &src, &code, &why, false, nullptr, 256, cache_only, &overrides)) {
    if (cache_only && why == okx::kNotCached) {
      if (pending) *pending = true;
      std::snprintf(p->lane_note, sizeof(p->lane_note), "being compiled");
      return;
    }
    std::snprintf(p->lane_note, sizeof(p->lane_note), "not generated: %.200s", why.c_str());
    return;
  }
  // A body that spills is only worth having while the spill is small.  Measured on MI355X: the double wishbone's
  // independent-solve body (104 - 192 B of scratch) is still 1.8x the quad kernel on 4096 geometries x 256 steps, its
  // looping chain body (668 B) was 8 % slower than the quad kernel's chains; MacPherson (0 B) wins both ways.
  p->lane_cold_scratch = lane_worst_scratch(code, overrides, "okx_lane_solve");
  p->lane_chain_scratch = lane_worst_scratch(code, overrides, "okx_lane_chain");
  p->lane_cold_ok = p->lane_cold_scratch >= 0 && p->lane_cold_scratch <= 256;
  // ... and a flat chain body (okx_quad.hpp lane_chain_is_flat: the double wishbone; 0 B of scratch) is correct but does not
  // pay: each chain step repeats the independent solve's prologue and its records leave lane by lane, so 4096 x 256 in
  // chains of 4 takes 0.62 ms against 0.51 ms of independent solves, and a 1048576-step sweep of one geometry 0.47
  // against 0.43 ms although its evaluations drop from 2.97 to 1.53 (tools/lane_chain_modes.py, lane_chain_own.py).
  // Auto selection keeps resolving chain_len = -1 to independent solves there; kernel = 4 with chains runs it.
  p->lane_chain_ok = p->lane_chain_scratch == 0 && !okx::lane_chain_is_flat(p->host.n);
  if (!p->lane_cold_ok && !p->lane_chain_ok) {
    std::snprintf(p->lane_note, sizeof(p->lane_note), "the lane kernel of this program spills (%d / %d B of scratch): not used",
                  p->lane_cold_scratch, p->lane_chain_scratch);
    return;
  }
  hipModule_t mod = nullptr;
  hipError_t e = hipModuleLoadData(&mod, code.data());
  if (e != hipSuccess && !cache_only && !job) {
    (void)hipGetLastError();
    if (okx::lane_build(p->host, &src, &code, &why, true, nullptr, 256)) e = hipModuleLoadData(&mod, code.data());
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    std::snprintf(p->lane_note, sizeof(p->lane_note), "hipModuleLoadData: %s", hipGetErrorString(e));
    return;
  }
  hipFunction_t lane_u = nullptr;
  if (hipModuleGetFunction(&lane_u, mod, "okx_lane_solve_u") != hipSuccess ||
      hipModuleGetFunction(&p->lane_fn_g, mod, "okx_lane_solve_g") != hipSuccess ||
      hipModuleGetFunction(&p->lane_chain_u, mod, "okx_lane_chain_u") != hipSuccess ||
      hipModuleGetFunction(&p->lane_chain_g, mod, "okx_lane_chain_g") != hipSuccess ||
      hipModuleGetFunction(&p->lane_compact[0], mod, "okx_lane_solve_u_c") != hipSuccess ||
      hipModuleGetFunction(&p->lane_compact[1], mod, "okx_lane_solve_g_c") != hipSuccess ||
      hipModuleGetFunction(&p->lane_compact[2], mod, "okx_lane_chain_u_c") != hipSuccess ||
      hipModuleGetFunction(&p->lane_compact[3], mod, "okx_lane_chain_g_c") != hipSuccess ||
      hipModuleGetFunction(&p->lane_fn_eval, mod, "okx_lane_eval") != hipSuccess) {
    (void)hipGetLastError();
    (void)hipModuleUnload(mod);
    p->lane_fn_u = p->lane_fn_g = p->lane_fn_eval = nullptr;
    p->lane_chain_u = p->lane_chain_g = nullptr;
    std::snprintf(p->lane_note, sizeof(p->lane_note), "kernel symbols missing in the code object");
    return;
  }
  for (const okx::LaneOverride& o : overrides) {
    hipFunction_t* slot = o.kernel == "okx_lane_solve_u" ? &lane_u : o.kernel == "okx_lane_solve_g" ? &p->lane_fn_g :
                          o.kernel == "okx_lane_chain_u" ? &p->lane_chain_u : o.kernel == "okx_lane_chain_g" ? &p->lane_chain_g :
                          o.kernel == "okx_lane_solve_u_c" ? &p->lane_compact[0] : o.kernel == "okx_lane_solve_g_c" ? &p->lane_compact[1] :
                          o.kernel == "okx_lane_chain_u_c" ? &p->lane_compact[2] : o.kernel == "okx_lane_chain_g_c" ? &p->lane_compact[3] : nullptr;
    hipModule_t extra = nullptr;
    hipFunction_t fn = nullptr;
    if (!slot || hipModuleLoadData(&extra, o.code.data()) != hipSuccess) {
      (void)hipGetLastError();
      continue;  // (the kept module's kernel stays)
    }
    if (hipModuleGetFunction(&fn, extra, o.kernel.c_str()) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipModuleUnload(extra);
      continue;
    }
    p->lane_extra_mods.push_back(extra);
    *slot = fn;
  }
  attach_lane_start_modes(p, mod, code);
  p->lane_mod = mod;
  std::atomic_thread_fence(std::memory_order_release);
  p->lane_fn_u = lane_u;  // the gate of the lane kernel's launch path, published last
}

// The compile job of a program whose kernels were not in the cache: compiles what was missing (same calls, same policy as
// the attach functions), keeps the results in the job and - through quad_compile - in the cache.  Touches nothing but
// the job.  No device call on this thread.
static void jit_job(okx_program::JitJob* job) {
  std::string src;
  if (job->want_quad) job->quad_ok = okx::quad_build(job->host, quad_waves_per_simd(), &src, &job->quad_code, &job->quad_why);
  job->quad_ready.store(1, std::memory_order_release);  // (a launch may switch over to the quad kernels now: two stages)
  if (job->want_lane && (job->quad_ok || !job->want_quad) && job->host.n_free <= okx::kQuadMaxFree && !okx::dev_switch("no_lane")) {
    std::string lsrc;
    job->lane_ok = okx::lane_build(job->host, &lsrc, &job->lane_code, &job->lane_why, false, nullptr, 256, false, &job->lane_overrides);
  } else if (job->want_lane) {
    job->lane_why = "no quad kernel to share first-step tables with";
  }
  job->finished.store(1, std::memory_order_release);
}

// Jobs of programs that were destroyed while their compiler was still running: joined (and freed) by a later destroy that
// finds them finished, or at process exit - a short script that drops its program early still leaves a filled cache behind,
// at the price of waiting for the compiler when it exits.
static std::mutex g_orphan_mutex;
static std::vector<okx_program::JitJob*> g_orphans;
static void reap_orphans(bool wait) {
  std::lock_guard<std::mutex> lock(g_orphan_mutex);
  for (size_t k = 0; k < g_orphans.size();) {
    okx_program::JitJob* job = g_orphans[k];
    if (!wait && !job->finished.load(std::memory_order_acquire)) {
      ++k;
      continue;
    }
    job->thread.join();
    delete job;
    g_orphans.erase(g_orphans.begin() + (long)k);
  }
}
static void reap_orphans_at_exit() { reap_orphans(true); }

// Switches a program over to its generated kernels once the compile job is done (`wait`: block until it is).  Called at
// the top of every entry point that launches; costs one atomic load when nothing is pending.  Never while the caller's
// stream records a graph (`stream` non-null: the launch's stream) - module loads and allocations are illegal inside a
// capture; the interpreter serves that launch and a later one switches over.
void attach_when_ready(okx_program* p, bool wait, const hipStream_t* stream) {
  okx_program::JitJob* job = p->jit.load(std::memory_order_acquire);
  if (!job) return;
  const bool all_done = wait || job->finished.load(std::memory_order_acquire);
  // first stage: the quad module alone is ready (the lane module's variants take another minute) - switch over to it now,
  // it serves every batch size until the lane kernels arrive
  const bool quad_stage = !all_done && job->want_quad && job->want_lane && job->quad_ready.load(std::memory_order_acquire) && !job->quad_attached.load(std::memory_order_acquire);
  if (!all_done && !quad_stage) return;
  if (!wait && stream && stream_is_capturing(*stream)) return;
  std::lock_guard<std::mutex> lock(p->jit_mutex);
  job = p->jit.load(std::memory_order_acquire);
  if (!job) return;  // another caller got here first
  if (!all_done) {
    if (job->quad_attached.load(std::memory_order_acquire)) return;  // (another caller did the first stage meanwhile)
    int current = p->device;
    (void)hipGetDevice(&current);
    if (current != p->device) (void)hipSetDevice(p->device);
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    const bool exchanged = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;
    {
      std::unique_lock<std::shared_mutex> kernels(p->kern_mutex);
      attach_quad_kernel(p, false, nullptr, job);   // (reads job->quad_code / quad_why only: written before quad_ready)
      job->quad_attached.store(1, std::memory_order_release);
    }
    if (exchanged) (void)hipThreadExchangeStreamCaptureMode(&mode);
    (void)hipGetLastError();
    if (current != p->device) (void)hipSetDevice(current);
    return;
  }
  job->thread.join();
  int current = p->device;
  (void)hipGetDevice(&current);
  if (current != p->device) (void)hipSetDevice(p->device);
  // (another thread of the process may be capturing in global mode - torch's default: this thread's module loads and
  //  allocations must not invalidate that capture)
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  const bool exchanged = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;
  {
    std::unique_lock<std::shared_mutex> kernels(p->kern_mutex);  // launches in progress finish first, later ones see the new set
    if (job->want_quad && !job->quad_attached.load(std::memory_order_acquire)) attach_quad_kernel(p, false, nullptr, job);
    if (job->want_lane) attach_lane_kernel(p, false, nullptr, job);
  }
  if (exchanged) (void)hipThreadExchangeStreamCaptureMode(&mode);
  (void)hipGetLastError();
  if (current != p->device) (void)hipSetDevice(current);
  p->jit.store(nullptr, std::memory_order_release);
  delete job;
}
// Generated kernels at okx_program_create: loaded when the kernel cache has them (the usual case: a build step and
// okx_precompile fill it).  Otherwise a host thread compiles them (10 ... 80 s per module) while the create call returns at
// once and the interpreter kernels solve; the first launch after the job is done switches the program over.
void attach_cached_or_compile(okx_program* p) {
  bool pending_quad = false, pending_lane = false;
  attach_quad_kernel(p, true, &pending_quad);
  if (!pending_quad) attach_lane_kernel(p, true, &pending_lane);
  if (!pending_quad && !pending_lane) return;
  okx_program::JitJob* job = new (std::nothrow) okx_program::JitJob;
  if (job) {
    job->host = p->host;
    job->want_quad = pending_quad;
    job->want_lane = true;  // (a pending quad kernel means the lane kernel, which shares its tables, was not looked at yet)
    try {
      job->thread = std::thread(jit_job, job);
      p->jit.store(job, std::memory_order_release);
    } catch (...) {  // no thread to be had: compile here, as before
      delete job;
      job = nullptr;
    }
  }
  if (!job) {
    if (pending_quad) attach_quad_kernel(p);
    attach_lane_kernel(p);
  }
}

// okx_program_destroy: a compile job still pending owns what it works on, so the program goes now and the job is joined when
// it has finished (by a later destroy, or at exit: it still fills the cache for the next program) - never a wait of minutes here
void retire_jit_job(okx_program* p) {
  if (okx_program::JitJob* job = p->jit.exchange(nullptr)) {
    if (job->finished.load(std::memory_order_acquire)) {
      job->thread.join();
      delete job;
    } else {
      std::lock_guard<std::mutex> lock(g_orphan_mutex);
      static bool registered = false;
      if (!registered) {
        registered = true;
        std::atexit(reap_orphans_at_exit);
      }
      g_orphans.push_back(job);
    }
  }
  reap_orphans(false);
}

void release_evaluation(okx_program* p) {
  if (p->ev_mod) (void)hipModuleUnload(p->ev_mod);
  if (p->ev_lane_mod) (void)hipModuleUnload(p->ev_lane_mod);
  p->ev_mod = p->ev_lane_mod = nullptr;
  p->ev_solve_u = p->ev_solve_g = p->ev_cold_u = p->ev_pos_u = p->ev_pos_g = nullptr;
  p->ev_lane_u = p->ev_lane_g = nullptr;
  p->ev_lane_pos_u = p->ev_lane_pos_g = nullptr;
}

int load_evaluated_module(okx_program* p, const std::string& code, hipFunction_t* solve_u) {
  if (p->ev_mod) {
    HIP_TRY(hipDeviceSynchronize());  // launches in flight may still run the modules about to be replaced
    release_evaluation(p);
  }
  p->ev_note[0] = 0;
  hipModule_t mod = nullptr;
  if (hipModuleLoadData(&mod, code.data()) != hipSuccess) {
    (void)hipGetLastError();
    return fail(OKX_ERR_DEVICE, "hipModuleLoadData failed for the evaluated module");
  }
  if (hipModuleGetFunction(solve_u, mod, "okx_quad_evsolve_u") != hipSuccess ||
      hipModuleGetFunction(&p->ev_solve_g, mod, "okx_quad_evsolve_g") != hipSuccess ||
      hipModuleGetFunction(&p->ev_pos_u, mod, "okx_quad_evaluate_u") != hipSuccess ||
      hipModuleGetFunction(&p->ev_pos_g, mod, "okx_quad_evaluate_g") != hipSuccess) {
    (void)hipGetLastError();
    (void)hipModuleUnload(mod);
    p->ev_solve_g = p->ev_pos_u = p->ev_pos_g = nullptr;
    return fail(OKX_ERR_DEVICE, "kernel symbols missing in the evaluated module");
  }
  if (hipModuleGetFunction(&p->ev_cold_u, mod, "okx_quad_evcold_u") != hipSuccess) {
    (void)hipGetLastError();
    p->ev_cold_u = nullptr;
  }
  p->ev_mod = mod;
  return OKX_OK;
}

}  // namespace okx

okx_program::~okx_program() {
  if (ev_mod) (void)hipModuleUnload(ev_mod);
  if (ev_lane_mod) (void)hipModuleUnload(ev_lane_mod);
  if (quad_mod) (void)hipModuleUnload(quad_mod);
  if (lane_mod) (void)hipModuleUnload(lane_mod);
  for (hipModule_t m : lane_extra_mods) (void)hipModuleUnload(m);
  if (predictor_dev) (void)hipFree(predictor_dev);
  for (HeadTable& t : head_tables) {
    (void)hipEventDestroy(t.ready);
    (void)hipFree(t.dev);
  }
  if (head_geom_dev) (void)hipFree(head_geom_dev);
  if (diag_scratch) (void)hipFree(diag_scratch);
  if (dev) (void)hipFree(dev);
}
