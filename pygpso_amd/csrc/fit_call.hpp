// An exact-GP fit call in flight: the map of the pinned scratch it reads and writes (FitScratch), how it is to be enqueued
// (FitPlan) and what was enqueued (FitCall).  Host side only; api.hip is the one file of the library that includes this
// (tools/fit_call_check.cpp compiles it on its own, so the three constants of the map come in as template arguments).
// gpso_fit_eval / gpso_fit_eval_loo decide the plan once and pass it down; the enqueue stages fill the record; finish_fit
// reads it.  Neither lives on the engine; the record's members are written by the named transitions below alone.  DESIGN.md 7o.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gpso {

// The context's pinned scratch as a fit call sees it, in doubles from its base.  [120, 128) holds two flags of other calls.
// A batched evaluation (gpso_fit_eval_u_batch) lays its results over the whole of it: it stages no theta here.
template <int kGradMaxLs, int kHyperHeader, int kMaxD>
struct FitScratch {
  // [0] nlml, [1] info (int), [7] the completion token, [8 ..] the gradient (ls..., variance, noise, c): the kernels' `scal`
  static constexpr size_t kScalDoubles = 8 + kGradMaxLs + 3;
  static constexpr size_t kTokenSlot = 7;  // (unused by the scalars' layout)
  static constexpr size_t kReadbackAt = 0, kReadbackDoubles = kScalDoubles;
  // set_theta stages the hyper block here and enqueues the copy to the device: the read-backs stay below it
  static constexpr size_t kThetaAt = 128, kThetaDoubles = kHyperHeader + kMaxD;
  // the LOO scalars (the same layout as the fit's), behind set_theta's staging block
  static constexpr size_t kLooAt = 256, kLooDoubles = kScalDoubles;
  static_assert(kTokenSlot < 8, "the token's word lies in front of the gradient");
  static_assert(kReadbackAt + kReadbackDoubles <= kThetaAt, "pinned scratch layout");
  static_assert(kThetaAt + kThetaDoubles <= kLooAt, "pinned scratch layout");
  // what a fit call asks the scratch for, once, before anything takes a pointer into it (growing it moves it)
  static constexpr size_t doubles(bool loo) { return loo ? kLooAt + kLooDoubles : kLooAt; }
};

struct FitPlan {
  const char* who = "";  // the entry point's name, for messages: gpso_fit_eval_loo where LOO is wanted, else gpso_fit_eval
  bool grad = false;     // the NLML gradient is wanted (and K^-1 with it)
  bool loo = false;      // the LOO tail runs behind the fit
  bool small = false;    // the one-launch fit (N <= 128); else the dense sequence
  bool timed = false;    // record the event pair gpso_last_ms(2) reads (and write no completion token)
  int64_t n = 0;

  static FitPlan make(bool grad, bool loo, bool small, bool timed, int64_t n) {
    FitPlan p;
    p.who = loo ? "gpso_fit_eval_loo" : "gpso_fit_eval";
    p.grad = grad; p.loo = loo; p.small = small; p.timed = timed; p.n = n;
    return p;
  }
  // the one-launch kernel writes the device's hyper block itself; every other fit has set_theta copy it
  bool theta_from_host() const { return !small; }
  // the split pieces of L^-1 wait for the first predict (ensure_split_pieces): a loss evaluation rarely sees one
  bool split_deferred() const { return grad && !small; }
  // 16-row tile rows of linv_p the fit writes (every dense fit writes, or will write, all 8)
  int tile_rows() const { return small ? (int)((n + 15) / 16) : 8; }
};

enum class FitWait { LooToken, FitToken, Stream };

template <typename Scratch>
struct FitCall {
  double* scratch = nullptr;  // the pinned scratch at the call's final size: the one pointer every stage uses
  double fit_token = 0.0;     // what the one-launch fit writes behind its scalars (0: none)
  double loo_token = 0.0;     // what the one-workgroup LOO tail writes behind its own (0: none)
  bool linv_p_deferred = false;  // the dense fit left the packed native-type L^-1 to ensure_linv_p

  double* readback() const { return scratch ? scratch + Scratch::kReadbackAt : nullptr; }
  double* theta_stage() const { return scratch ? scratch + Scratch::kThetaAt : nullptr; }
  double* loo_readback() const { return scratch ? scratch + Scratch::kLooAt : nullptr; }
  // ==== transitions ====
  // fit_eval_impl, behind its refusals: pinned_scratch(Scratch::doubles(plan.loo)), NULL where that failed
  static FitCall begun(double* pinned) {
    FitCall c;
    c.scratch = pinned;
    return c;
  }
  // enqueue_small_fit / enqueue_loo_tail (N <= 128), before the launch: `fresh` is the next sequence number, 0 on a timed
  // call.  The token's word is zeroed either way -- whatever an earlier call left there cannot pass for this one's
  double arm_fit_token(double fresh) { return fit_token = arm(readback(), fresh); }
  double arm_loo_token(double fresh) { return loo_token = arm(loo_readback(), fresh); }
  // enqueue_dense_fit
  void linv_p_left(bool deferred) { linv_p_deferred = deferred; }
  // finish_fit: what ends the call
  FitWait wait_on(const FitPlan& plan) const {
    if (loo_token != 0.0) return FitWait::LooToken;
    if (plan.small && fit_token != 0.0 && !plan.timed && !plan.loo) return FitWait::FitToken;
    return FitWait::Stream;
  }
  // ... and, for a token, the word the host spins on and the value it waits for
  const double* token_word(FitWait how) const { return (how == FitWait::LooToken ? loo_readback() : readback()) + Scratch::kTokenSlot; }
  double token(FitWait how) const { return how == FitWait::LooToken ? loo_token : fit_token; }

 private:
  static double arm(double* region, double fresh) {
    if (region == nullptr) return 0.0;
    region[Scratch::kTokenSlot] = 0.0;
    return fresh;
  }
};

}  // namespace gpso
