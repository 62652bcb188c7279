// mg_stop.h -- when a multigrid solve stops: the convergence test and the loop of the two single-level solvers (mg_cc.hip, mg_nd.hip) around it.
#pragma once
#include "vdn_internal.h"

// the test every solve applies to the norm of its residual (the reductions turn NaN into +inf: an infinite right-hand side never passes by rel_eps)
inline bool mg_converged(double rn, double bnorm, double rel_eps, double abs_eps) { return (rn <= rel_eps * bnorm && bnorm < HUGE_VAL) || rn <= abs_eps; }

// The cycles of one single-level solve that tests its residual.  The solver hands over what differs between the two multigrids:
//   first(blind)   pre-smoothing and the residual with its norm on the device (blind: the norm stays rank-local, it goes into the history)
//   cycle()        [coarse correction, post-smoothing, the next cycle's pre-smoothing, residual + norm] as ONE replayed graph
//   blind(n)       n such cycles as one graph, each followed by norm_hist_push of its rank-local norm
//   read()         the norm of the last residual, on the host: one 8-byte read-back
// -- the same launch sequence as testing the residual a cycle computes after its pre-smoothing.
// vdn_params.mg_predict (`predict`: the projections' calls, zero guess): the previous solve of this kind and size stopped after `pred` cycles, so the norms of
// the cycles before pred - 1 are not waited for -- they go into the device-side history and are read in one go (ONE all-reduce) after cycle pred - 1.  Should
// the history show that an earlier cycle had already met the tolerance, the solve is thrown away: `overshot` comes back set and the solver releases what it
// built and repeats itself through mg_repeat_unpredicted, with a read-back per cycle (rare: the count dropped by two or more from one solve to the next).
// The result is the one the plain loop gives, whatever the prediction was.  `remember`: a converged solve leaves its count for the next one.
struct MgStop { int cycles = 0; double res = 0.0; bool conv = false, overshot = false; };
template <class First, class Cycle, class Blind, class Read>
MgStop mg_stop_loop(int solver, const int gn[3], bool predict, bool remember, const MgRequest &q, double bnorm, const double *d_nrm,
                    First first, Cycle cycle, Blind blind, Read read) {
  MgStop s;
  s.conv = (bnorm == 0.0);
  const int pred = (predict && !s.conv) ? std::min(mg_predict_get(solver, gn), std::min(q.max_iter, 63)) : 0;
  if (!s.conv) {
    first(pred >= 2);
    if (pred >= 2) {
      norm_hist_reset(); norm_hist_push(d_nrm);
      blind(pred - 1);
      const double *h = norm_hist_read(pred);
      int stop = -1;                                             // the first cycle count at which the plain loop would have stopped
      for (int c = 0; c < pred && stop < 0; c++)
        if (mg_converged(h[c], bnorm, q.rel_eps, q.abs_eps) || !(h[c] < HUGE_VAL)) stop = c;
      if (stop >= 0 && stop < pred - 1) { s.overshot = true; return s; }
      s.cycles = pred - 1; s.res = h[pred - 1];
    } else s.res = read();
  }
  while (!s.conv) {
    if (mg_converged(s.res, bnorm, q.rel_eps, q.abs_eps)) { s.conv = true; break; }
    if (s.cycles >= q.max_iter || !(s.res < HUGE_VAL) || !(bnorm < HUGE_VAL)) break;     // also: a NaN / inf norm
    cycle();
    s.cycles++;
    s.res = read();
  }
  if (s.conv && remember && s.cycles >= 1) mg_predict_set(solver, gn, s.cycles);
  return s;
}
// the repeat of a solve whose prediction overshot: the same request once more, with mg_predict_get answering 0 meanwhile
template <class Solve> int mg_repeat_unpredicted(Solve solve) {
  struct Off { Off() { g_mg_predict_off++; } ~Off() { g_mg_predict_off--; } } off_;
  return solve();
}
