// Screened best-UCB calls: the bound, the threshold and the acceptance test.  One restatement for the device (screen.hip,
// predict.hip: keyed_argmax_stage2) and for the host (gpso_screen_eval_host: the CPU tests), built like acq.hpp.  DESIGN.md 4.1.
//
// finalize_leaf (predict.hip) forms, for a leaf with mean my = fl(sum of the row blocks' mean shares + mean_c):
//     v = sum_b part_var[b]  (>= 0: a sum of squares, starting at 0),  fv = fl(variance - v),  vy = fl(fv + noise),
//     u = fl(my + fl(varsigma * vy)).
// Every rounding is monotone, so for varsigma >= 0 the u the kernel computes can never exceed the same expression at v = 0:
//     ub = fl(my + fl(varsigma * fl(variance + noise))),
// PROVIDED my is the mean the tile kernel itself computes, bit for bit (screen.hip: leaf_mean_kernel).  A bound in the
// kernel's own arithmetic: no error analysis, no second product.
//
// A call keeps ("survives") every leaf with  !(ub < T'),  T' = fl(max finite my + fl(varsigma * noise)), and every leaf whose
// mean is not finite (NaN ranks first in the arg-max); it scores the survivors with the tile kernel and ACCEPTS the winner's
// record iff its ucb u* is NaN or u* >= T': every pruned leaf then had ub < T' <= u* and could neither win nor tie.  T' is the
// ucb the leaf of the largest mean has when its variance share is exactly zero; nothing relies on that -- a u* below T' is
// refused and the call runs the general sequence.
#pragma once
#include <cmath>
#include <cstdint>

#include "acq.hpp"

namespace gpso {

// gpso_last_count(ctx, 8)
constexpr int kScreenNone = 0, kScreenAccepted = 1, kScreenRefused = 2;

// finalize_leaf's ucb under the reference's rule, from the leaf's mean and its summed variance share v
GPSO_ACQ_HD inline double screen_ucb(double my, double v, double variance, double noise, double varsigma) {
#pragma clang fp contract(off)
  const double fv = variance - v;
  const double vy = fv + noise;
  return acq_mul_then_add(my, varsigma, vy);
}
// ... and what it cannot exceed, whatever v >= 0 turns out to be (varsigma >= 0)
GPSO_ACQ_HD inline double screen_bound(double my, double variance, double noise, double varsigma) {
  return screen_ucb(my, 0.0, variance, noise, varsigma);
}
// max_my: the largest FINITE mean of the batch; -inf where there is none (then nothing is pruned)
GPSO_ACQ_HD inline double screen_threshold(double max_my, double noise, double varsigma) {
  return acq_mul_then_add(max_my, varsigma, noise);
}
GPSO_ACQ_HD inline bool screen_finite(double x) { return x - x == 0.0; }
GPSO_ACQ_HD inline bool screen_survives(double my, double ub, double threshold) {
  return !screen_finite(my) || !(ub < threshold);
}
// the survivors' winner: count survivors (cap: how many the survivors' launch had room for), u_star the winner's ucb
GPSO_ACQ_HD inline bool screen_accepts(double u_star, double threshold, int64_t count, int64_t cap) {
  return count > 0 && count <= cap && (u_star != u_star || u_star >= threshold);
}

// The survivors' launch has two tiles (leaf_split.hpp: the batch kernel's 256 leaves per workgroup, or the narrow 64), and only
// the device knows the count: both are enqueued, each behind a live-row word of its own in the screen's control block, of which
// the compaction zeroes one -- that launch leaves at once.  Words of screen_ctl: [0] live rows, [1] the count, [2] T', and
constexpr int kScreenCtlNarrow = 3, kScreenCtlWide = 4;  // the live rows as the narrow / the wide launch sees them
// Up to how many survivors the narrow tile is the faster one: a makespan model written like leaf_row_splits, in k-steps of the
// wide kernel.  Either launch gives a workgroup one row block (8 (b + 1) k-steps for block b), heaviest first, one workgroup per
// CU at a time (neither tile's LDS fits a CU twice).  A launch lasts as long as its heaviest block's chain, 8 nbi steps, or as
// the chip's share of all its steps, tiles x 4 nbi (nbi + 1) / CUs, whichever is longer; a narrow step takes kNarrowStep of a
// wide one (measured on lists of 28 .. 2 048 rows, where both launches are chain-bound: 66 against 128 us at N = 2048, 262
// against 500 us at N = 8192 -- profiles/screen_narrow_ab.txt).  Below the crossover the wide launch is its chain and the narrow
// one gains; above it the narrow launch is its share of four times as many workgroups, each with the whole row block's L^-1
// traffic and DMA issue to itself, and loses (N = 2048: x 0.92 at 6 144 rows, x 1.10 at the room's 8 192; model: 6 976).
// -> the largest count, a multiple of 64 and at most cap, that takes the narrow tile; 0: none.  Monotone: a count above it never does.
inline int64_t survivor_narrow_max(int nbi, int ncu, int64_t cap) {
  constexpr double kNarrowStep = 0.52;
  if (nbi < 1 || ncu < 1) return 0;
  const double chain = 8.0 * nbi, per_tile = 4.0 * nbi * (nbi + 1.0) / ncu;
  int64_t best = 0;
  for (int64_t c = 64; c <= cap; c += 64) {
    const double narrow = kNarrowStep * (chain > per_tile * (double)(c / 64) ? chain : per_tile * (double)(c / 64));
    const double wide = chain > per_tile * (double)((c + 255) / 256) ? chain : per_tile * (double)((c + 255) / 256);
    if (!(narrow < wide)) break;
    best = c;
  }
  return best;
}

// The compaction's partition of a batch of m leaves over `parts` workgroups: part w owns the leaves [lo, hi), ranges of equal
// length -- a multiple of 64, one coalesced load per lane and step -- in ascending order; the last non-empty range may be
// shorter, the ranges behind it are empty.  Every leaf belongs to exactly one part.
struct ScreenRange {
  int64_t lo, hi;
};
GPSO_ACQ_HD inline ScreenRange screen_partition(int64_t m, int parts, int w) {
  const int64_t span = (int64_t)parts * 64;
  const int64_t seg = (m + span - 1) / span * 64;
  const int64_t lo = w * seg < m ? w * seg : m;
  return ScreenRange{lo, lo + seg < m ? lo + seg : m};
}
// how many parts a batch of m leaves is compacted in: one wave per 256 leaves up to kScreenMaxParts (then longer ranges) -- a
// part sums the counts of all parts in front of it, so their number is what its walk starts behind
constexpr int kScreenMaxParts = 256;
inline int screen_parts(int64_t m) {
  const int64_t p = (m + 255) / 256;
  return (int)(p < 1 ? 1 : p > kScreenMaxParts ? kScreenMaxParts : p);
}

}  // namespace gpso
