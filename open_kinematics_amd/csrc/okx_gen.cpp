// okx_gen.cpp — the shared part of the kernel source generators (okx_gen.hpp).
#include "okx_gen.hpp"

#include <cstdarg>
#include <cstdio>
#include <set>

#include "okx_quad.hpp"

namespace okx {

std::vector<int> elimination_order(const DevProgram& P, int last_point) {
  const int nf = P.n_free;
  std::vector<std::set<int>> adj(nf);
  for (int i = 0; i < P.m; ++i)
    for (int a = 0; a < P.row_nblk[i]; ++a)
      for (int b = 0; b < P.row_nblk[i]; ++b)
        if (a != b) adj[P.row_blk[i][a]].insert(P.row_blk[i][b]);
  std::vector<bool> gone(nf, false);
  std::vector<int> perm;
  int held_back = -1;
  if (last_point >= 0)
    for (int k = 0; k < nf; ++k)
      if (P.free_point[k] == last_point) held_back = k;
  for (int step = 0; step < nf; ++step) {
    int best = -1;
    for (int k = 0; k < nf; ++k)
      if (!gone[k] && k != held_back && (best < 0 || adj[k].size() < adj[best].size())) best = k;
    if (best < 0) best = held_back;
    perm.push_back(best);
    gone[best] = true;
    for (int u : adj[best]) {
      adj[u].erase(best);
      for (int w : adj[best])
        if (w != u) adj[u].insert(w);
    }
    adj[best].clear();
  }
  return perm;
}

GenBase::GenBase(const DevProgram& prog, int last_point) : P(prog), perm(elimination_order(prog, last_point)) {
  blk_of_point.assign(P.n_points, -1);
  dop_of_point.assign(P.n_points, -1);
  for (int F = 0; F < P.n_free; ++F) blk_of_point[fp(F)] = F;
  for (int e = 0; e < P.n_derived; ++e) dop_of_point[P.dop_out[e]] = e;
}

int GenBase::pin_leader(int i) const {
  if (i >= P.n_crows || P.row_type[i] != OKX_ROW_LINE_PIN) return i;
  for (int j = 0; j < i; ++j) {
    if (P.row_type[j] != OKX_ROW_LINE_PIN || P.row_pts[j][0] != P.row_pts[i][0]) continue;
    bool same = true;
    for (int k = 0; k < 6; ++k) same = same && P.row_param[j][k] == P.row_param[i][k];
    if (same) return j;
  }
  return i;
}

void GenBase::f(const char* fmt, ...) {
  char buf[2048];
  va_list ap, again;
  va_start(ap, fmt);
  va_copy(again, ap);
  const int need = std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (need >= (int)sizeof(buf)) {  // a long combined expression: format again into an exact-size buffer
    std::string big((size_t)need + 1, '\0');
    std::vsnprintf(&big[0], big.size(), fmt, again);
    big.resize((size_t)need);
    out += big;
  } else if (need > 0) {
    out += buf;
  }
  va_end(again);
  out += '\n';
}

void GenBase::fill_info(const char* indent) {
  f("%sokx_info inf; inf.max_residual = mres; inf.cost = Fc; inf.last_step = last_step;", indent);
  f("%sinf.iterations = iters; inf.nfev = nfev; inf.flags = flags; inf.reserved = 0;", indent);
}

HeadLayout::HeadLayout(const DevProgram& P, const PairView* pv) {
  const int nf = P.n_free, T = P.n_targets, prog_targets = pv ? pv->n_prog_targets : T;
  cols.push_back({-1, -1, -1});
  for (int pt = 0; pt < prog_targets; ++pt)
    for (int t = 0; t < T; ++t) {
      if (!pv) { if (t == pt) cols.push_back({t, -1, pt}); continue; }
      for (int sd = 0; sd < 2; ++sd)
        if (pv->tgt[sd][t] == pt) cols.push_back({t, sd, pt});
    }
  const int HK = (int)cols.size();
  side = 4 * nf * HK;
  off = (pv ? 2 : 1) * side + 2 * HK * HK;
  if (!(pv && dev_switch("pair_first_order_head")))
    for (int s2 = 1; s2 < HK; ++s2)
      for (int t2 = s2; t2 < HK; ++t2) pairs.push_back({s2, t2});
  s_off = off + 8;
  s_side = 4 * nf * (HK - 1) * HK / 2;
  stride = off + 8 + (pv ? 2 : 1) * s_side;
}

}  // namespace okx
