// okx_predictor.cpp — the chain-head predictor of a program (okx_program_fit_predictor, include/okx.h): a tensor Chebyshev
// fit over a target box.  Host code: its node solve is the public okx_solve_batch.
#include "okx_program.hpp"

#include <cmath>
#include <functional>
#include <vector>

using okx::attach_when_ready;
using okx::fail;

extern "C" {

int32_t okx_program_has_predictor(const okx_program* p) { return p && p->predictor_dev ? 1 : 0; }

/* The node solve of okx_program_fit_predictor: the program at `targets` (info->size() cold starts on the quad kernel,
   synchronous), records and info back on the host. */
static int32_t solve_predictor_nodes(okx_program* p, const std::vector<double>& targets, std::vector<double>* out, std::vector<okx_info>* info,
                                     void* stream) {
  const long long S = (long long)info->size();
  // one scratch allocation for the node solve: targets | positions | info records
  const size_t bytes_t = targets.size() * sizeof(double), bytes_out = out->size() * sizeof(double);
  const size_t bytes_info = (size_t)S * sizeof(okx_info);
  char* d_scratch = nullptr;
  HIP_TRY(hipMalloc((void**)&d_scratch, bytes_t + bytes_out + bytes_info));
  double* d_t = reinterpret_cast<double*>(d_scratch);
  double* d_out = reinterpret_cast<double*>(d_scratch + bytes_t);
  okx_info* d_info = reinterpret_cast<okx_info*>(d_scratch + bytes_t + bytes_out);
  int32_t rc = OKX_OK;
  okx_solve_opts o;
  okx_default_opts(&o);
  o.chain_len = 1;
  o.kernel = 3;
  o.confirm_full_pass = 1;  // end on a computed correction: the fit wants every digit
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(d_t, targets.data(), bytes_t, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = fail(OKX_ERR_DEVICE, "copy failed");
  if (rc == OKX_OK) rc = okx_solve_batch(p, &o, S, d_t, nullptr, nullptr, d_out, d_info, stream);
  if (rc == OKX_OK &&
      (hipMemcpyAsync(out->data(), d_out, bytes_out, hipMemcpyDeviceToHost, st) != hipSuccess ||
       hipMemcpyAsync(info->data(), d_info, bytes_info, hipMemcpyDeviceToHost, st) != hipSuccess ||
       hipStreamSynchronize(st) != hipSuccess))
    rc = fail(OKX_ERR_DEVICE, "node solve failed: %s", hipGetErrorString(hipGetLastError()));
  (void)hipFree(d_scratch);
  return rc;
}

/* Fits the chain-head predictor of a program with a quad kernel over the target box [lo, hi] (absolute
   target values, host arrays of n_targets; lo[t] == hi[t]: that target is held): solves the program at the
   (degree + 1)^d Chebyshev nodes of the d varying targets (one cold-start launch, synchronous), takes the
   tensor Chebyshev coefficients of every free coordinate by discrete orthogonality and keeps the terms up to
   total degree `degree` (<= 0: 7).  Launches with opts.predictor != 0 on the program's own geometry start
   every chain head at that polynomial (targets clamped to the box) instead of the design state.  Refitting
   replaces the previous model. */
int32_t okx_program_fit_predictor(okx_program* p, const double* lo, const double* hi, int32_t degree, void* stream) {
  if (!p || !lo || !hi) return fail(OKX_ERR_INVALID, "null pointer");
  attach_when_ready(p, false);
  {
    std::shared_lock<std::shared_mutex> kernels(p->kern_mutex);  // (released before the node solve takes it itself)
    if (!p->quad_fn_u) return fail(OKX_ERR_INVALID, "the predictor belongs to the quad kernel: %s", p->quad_note);
    if (p->quad_ppw != 16) return fail(OKX_ERR_INVALID, "pair-mode kernels carry no predictor (register-bound)");
  }
  const okx::DevProgram& H = p->host;
  const int T = H.n_targets;
  if (T < 1) return fail(OKX_ERR_INVALID, "program has no targets");
  const int D = degree <= 0 ? okx::kPredictorDegree : degree;
  if (D > okx::kPredictorMaxDegree) return fail(OKX_ERR_INVALID, "degree must be <= %d", okx::kPredictorMaxDegree);
  std::vector<int> out_of(H.n_points, -1);
  for (int k = 0; k < H.n_out; ++k) out_of[H.out_point[k]] = k;
  for (int f = 0; f < H.n_free; ++f)
    if (out_of[H.free_point[f]] < 0) return fail(OKX_ERR_INVALID, "free point %d is not an output point", H.free_point[f]);
  std::vector<double> mid(T), half(T);
  std::vector<int> deg(T), vary;
  for (int t = 0; t < T; ++t) {
    if (!(hi[t] >= lo[t])) return fail(OKX_ERR_INVALID, "target %d: hi < lo", t);
    mid[t] = 0.5 * (lo[t] + hi[t]);
    half[t] = 0.5 * (hi[t] - lo[t]);
    deg[t] = half[t] > 1e-9 ? D : 0;
    if (deg[t]) vary.push_back(t);
  }
  const int d = (int)vary.size(), N = D + 1;
  long long S = 1;
  for (int k = 0; k < d; ++k) {
    S *= N;
    if (S > 32768) return fail(OKX_ERR_LIMIT, "%d varying targets at degree %d need too many nodes", d, D);
  }
  std::vector<double> node(N);
  for (int a = 0; a < N; ++a) node[a] = cos(3.14159265358979323846 * (a + 0.5) / N);
  // node k <-> digits a_0 .. a_{d-1} (dimension 0 slowest)
  auto digit = [&](long long k, int j) {
    for (int q = d - 1; q > j; --q) k /= N;
    return (int)(k % N);
  };
  std::vector<double> targets((size_t)S * T);
  for (long long k = 0; k < S; ++k) {
    for (int t = 0; t < T; ++t) targets[(size_t)k * T + t] = mid[t];
    for (int j = 0; j < d; ++j) targets[(size_t)k * T + vary[j]] = mid[vary[j]] + half[vary[j]] * node[digit(k, j)];
  }
  std::vector<double> out((size_t)S * H.n_out * 3);
  std::vector<okx_info> info((size_t)S);
  if (const int32_t rc = solve_predictor_nodes(p, targets, &out, &info, stream)) return rc;
  for (long long k = 0; k < S; ++k)
    if (!(info[k].flags & OKX_INFO_CONVERGED) || (info[k].flags & (OKX_INFO_FAILED | OKX_INFO_RESIDUAL_EXCEEDED)))
      return fail(OKX_ERR_INVALID, "node %lld of the target box did not converge", k);
  // Chebyshev values at the nodes
  std::vector<double> cheb((size_t)N * N);  // [i][a] = T_i(node_a)
  for (int a = 0; a < N; ++a) {
    cheb[a] = 1.0;
    if (N > 1) cheb[(size_t)N + a] = node[a];
    for (int i = 2; i < N; ++i) cheb[(size_t)i * N + a] = 2.0 * node[a] * cheb[(size_t)(i - 1) * N + a] - cheb[(size_t)(i - 2) * N + a];
  }
  // Table in the kernel's layout (okx_quadgen.cpp): per target (mid, 1 / half-range, degree), the
  // total-degree cap, the table length, then one [free][4] block per term in the kernel's loop order:
  // target 0 outermost, index i_t <= degree_t and <= the remaining total degree.
  const int nv = H.n_free * 4;
  std::vector<double> table((size_t)3 * T + 2, 0.0);
  for (int t = 0; t < T; ++t) {
    table[3 * t] = mid[t];
    table[3 * t + 1] = deg[t] ? 1.0 / half[t] : 0.0;
    table[3 * t + 2] = (double)deg[t];
  }
  table[3 * T] = (double)D;
  std::vector<int> idx(T, 0), slot_of(T, -1);
  for (int j = 0; j < d; ++j) slot_of[vary[j]] = j;
  std::vector<double> block(nv);
  std::function<void(int, int)> walk = [&](int t, int budget) {
    if (t == T) {
      std::fill(block.begin(), block.end(), 0.0);
      double scale = 1.0;
      for (int j = 0; j < d; ++j) scale *= (idx[vary[j]] == 0 ? 1.0 : 2.0) / N;
      for (long long k = 0; k < S; ++k) {
        double w = scale;
        for (int j = 0; j < d; ++j) w *= cheb[(size_t)idx[vary[j]] * N + digit(k, j)];
        for (int f = 0; f < H.n_free; ++f) {
          const int o = out_of[H.free_point[f]];
          for (int c = 0; c < 3; ++c) block[f * 4 + c] += w * out[((size_t)k * H.n_out + o) * 3 + c];
        }
      }
      table.insert(table.end(), block.begin(), block.end());
      return;
    }
    for (int i = 0; i <= deg[t] && i <= budget; ++i) {
      idx[t] = i;
      walk(t + 1, budget - i);
    }
    idx[t] = 0;
  };
  walk(0, D);
  table[3 * T + 1] = (double)table.size();
  double* d_table = nullptr;
  HIP_TRY(hipMalloc(&d_table, table.size() * sizeof(double)));
  if (hipMemcpy(d_table, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d_table);
    return fail(OKX_ERR_DEVICE, "copy failed");
  }
  if (p->predictor_dev) {
    HIP_TRY(hipDeviceSynchronize());  // launches in flight may still read the old table
    (void)hipFree(p->predictor_dev);
  }
  p->predictor_dev = d_table;
  p->predictor_len = (long long)table.size();
  return OKX_OK;
}

}  // extern "C"
