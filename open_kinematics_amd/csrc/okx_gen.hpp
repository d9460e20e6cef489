// okx_gen.hpp — what the two kernel source generators (okx_quadgen.cpp, okx_lanegen.cpp) have in common: the text
// emitter, the block elimination order and the program lookups both use, and the device functions whose text is the same
// in both generated modules.  Internal to csrc/.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "okx_plan.hpp"

namespace okx {

struct PairView;  // okx_quad.hpp

// Block F of the generated code (x{F}, rows 3F+c of J^T J, elimination step F of the LDL^T) is the program's free point
// perm[F]: a greedy minimum-degree order on the block graph of J^T J (ties: program order), so that leaf chains (rack
// pickup, pushrod / rocker / drop-link) are eliminated before the upright's clique and create no fill-in.
// ONE function for every generator: the first-step table of okx_quad_head_u/_g is laid out in this block order and the
// lane kernels read it, so the quad and the lane module of a program must number their blocks alike.
// `last_point` >= 0: the block of that free point is held back and eliminated last (pair mode with one joining row,
// okx_quadgen.cpp).
std::vector<int> elimination_order(const DevProgram& P, int last_point = -1);

// Base of a source generator specialised to one program: the text under construction and the lookups on `P`.
class GenBase {
 public:
  explicit GenBase(const DevProgram& prog, int last_point = -1);

  const DevProgram& P;
  std::vector<int> perm;                        // elimination_order(P, last_point)
  std::vector<int> blk_of_point, dop_of_point;  // point -> block of a free point / derived op that writes it, -1: neither
  std::string out;                              // the text emitted so far
  std::string why;                              // why an emission refused the program
  int uid = 0;                                  // numbers the temporaries: the text depends on the ORDER of emission calls

  int fp(int F) const { return P.free_point[perm[F]]; }
  int target_of_row(int i) const { return (int)P.row_param[i][3]; }
  // The three LINE_PIN rows that one point-on-line constraint flattens into (same point, same line in the program's own
  // geometry, components 0/1/2) share their line parameters and their cross product: the first of them is the group's
  // leader.  Per-geometry tables keep them equal (okx_rebind_design writes the same anchor for every pin of a point).
  int pin_leader(int i) const;

  void f(const char* fmt, ...) __attribute__((format(printf, 2, 3)));  // one line of text (printf-style) + '\n'
  std::string tmp(const char* base) { return "_" + std::string(base) + std::to_string(uid++); }
  void fill_info(const char* indent);  // `okx_info inf` filled from a solve's final scalars: the same text in both modules
};

// Layout of one geometry's first-step table (okx_quad_head_u/_g write it, the solve bodies and the lane kernels read
// it, okx_api.hip allocates quad_head_stride() doubles per geometry), in doubles:
// Q[k][F][4] (lane components, 0 in slot 3; pair mode: one such block per half), M[j][k] = Q_j . G_k, N[j][k] = Q_j . Q_k,
// then dmax, min pivot, sum of squared constraint residuals, max |constraint residual|, ok, max pivot, pairs carried, 0.
// Column k = 0 is the constraint rows' own gradient G_0 = Jc^T rc at the design state (the reference's distance
// rows carry softnorm's -1e-6 offset there, constraints.py:125-134, so it is small but not zero) with weight 1;
// column k = t + 1 belongs to target t: G_k = J^T e_t, weight = that target's residual.  Q_k = (J^T J + lambda I)^-1 G_k.
// Pair mode carries the first-order table too.  Measured on the axle grid, round 3: cold starts 5.57 -> 4.72
// evaluations, 0.483 -> 0.455 ms; chained grids unchanged (0.211 vs 0.212 ms) - in round 2 the block's registers still
// cost the chained grid 3 %, before the LM scalars and constants had homes in LDS.
struct HeadLayout {
  // columns of the table: the constraint gradient, then one per PROGRAM target (pair mode: a side target stands for one
  // program target per half that carries it; the column's weight is that half's residual, its Q spans both halves)
  struct Col { int t, side, prog_t; };
  std::vector<Col> cols;
  // Second-order terms of the shared first step: S_st = (J^T J + lambda I)^-1 J^T r''(Q_s, Q_t) for the target
  // columns s <= t, [pair][F][4] after the scalars (pair mode: one such block per half, the left half's first);
  // scalar 6 says how many pairs the table carries.
  std::vector<std::pair<int, int>> pairs;
  int side;    // doubles of one half's Q block
  int off;     // where the 8 scalars start
  int s_off;   // where the S blocks start
  int s_side;  // doubles of one half's S block (room for every pair, carried or not)
  int stride;  // doubles per geometry

  // `P`: the program the kernels are specialised to - in pair mode the side program of `pv`
  HeadLayout(const DevProgram& P, const PairView* pv);
};

// Device functions both generated modules define with the same text; each generator splices them into its own prelude
// where that prelude has always had them (the argument structs' declarations: okx_quad.hpp, beside their host mirrors).
// Everything else of the two preludes differs at least in its comments and stays with its generator: generated text is
// the kernel cache key.
constexpr const char* kDevFastRcp = R"SRC(DEV double fast_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  double e = fma(-x, r, 1.0);
  r = fma(e, r, r);
  e = fma(-x, r, 1.0);
  return fma(e, r, r);
}
)SRC";
constexpr const char* kDevPivotRcp = R"SRC(DEV double pivot_rcp(double x) {
  const double r = __builtin_amdgcn_rcp(x);
  return fma(fma(-x, r, 1.0), r, r);
}
)SRC";
constexpr const char* kDevFastSqrtRsqrt = R"SRC(DEV void fast_sqrt_rsqrt(double x, double* root, double* inv) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  const double r = fma(-h, g, 0.5);
  g = fma(g, r, g);
  h = fma(h, r, h);
  const double d = fma(-g, g, x);
  g = fma(d, h, g);
  *root = g;
  *inv = h + h;
}
)SRC";

}  // namespace okx
