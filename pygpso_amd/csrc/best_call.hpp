// A best-UCB call in flight: how it is to be enqueued (BestPlan) and what was enqueued (BestCall).  Host side only; api.hip
// is the one file of the library that includes this (tools/best_call_check.cpp compiles it on its own).  The entry point
// decides the plan once and passes it down; the enqueue functions fill the record; whoever finishes the call consumes it.
// Neither lives on the engine; their members are written by the named constructors and transitions below alone.  DESIGN.md 3.4.
#pragma once
#include <cstdint>

#include "acq.hpp"

namespace gpso {

struct BestPlan {
  bool one_launch = true;  // the one-launch kernel may be tried (it may ask for the sequence with the append counter)
  bool screen = false;     // the screen may be tried: the leaves stay where they are until the record is read, for a re-run
  bool is_rerun = false;   // repeats a call that asked for the general sequence: the screen's counters (7 / 8) stay
  bool timed = false;      // record the event pairs gpso_last_ms reads (and write no completion token)
  double* slot = nullptr;  // the pinned result memory of a ticket; NULL: the context's shared scratch

  // gpso_best_ucb(_acq), gpso_best_ucb_grow(_acq); gpso_fold_winners (nothing of it asks for a re-run)
  static BestPlan synchronous(bool timed, bool may_screen) { return BestPlan{true, may_screen, false, timed, nullptr}; }
  // gpso_best_ucb_begin / _grow_begin: untimed, into its own slot.  No one-launch kernel -- gpso_best_ucb_end could run it
  // again, but the device work of the next call is queued behind this one by then; the screen travels with what a re-run needs
  static BestPlan ticket(double* slot, bool may_screen) { return BestPlan{false, may_screen, false, false, slot}; }
  // a sharded call's local half, gpso_shard_winners(_grow): its payload's status slot is the group's, nobody could re-run it
  static BestPlan group_half(bool timed) { return BestPlan{false, false, false, timed, nullptr}; }
  // the call again after it asked for the general sequence: synchronous, into the shared scratch, timed as the plan was
  BestPlan rerun() const { return BestPlan{false, false, true, timed, nullptr}; }
};

enum class BestKind { None, General /* several workgroups finalise */, Small /* one workgroup does */, OneLaunch, Screened, Folded };

struct BestCall {
  BestKind kind = BestKind::None;
  int nseg = 0;
  int mode = 0;             // the read-back: 0 winners, 1 + the live row count -> last_count[0], 2 a folded group payload
  double* host = nullptr;   // pinned memory the call's last kernel writes its records to (NULL: they are copied from the device)
  double token = 0.0;       // the completion token that kernel writes behind them (0: none -- wait for an event)
  bool timed = false;       // the plan's
  bool coll_timed = false;  // the event pair around the collective (all-gather + fold) was recorded
  int tile_pairs = 0;       // event pairs recorded around the tile kernel
  // a screened call: what running it again takes (one segment; device leaves the caller leaves untouched until then)
  struct Rerun {
    const void* xs = nullptr;
    int xs_dtype = 0;
    int64_t m = 0;
    AcqSpec acq;
  } screen;
  int64_t narrow_max = 0;  // ... and up to how many survivors its survivors' launch took the narrow tile (gpso_last_count 9)

  bool none() const { return kind == BestKind::None; }
  // ==== transitions ====
  // every enqueue_best_* begins with it (and the sharded entry points, whose half may fail before it enqueues anything)
  static BestCall begun(const BestPlan& plan) {
    BestCall c;
    c.timed = plan.timed;
    return c;
  }
  // score_device_leaves returned (enqueue_best_leaves / _grow / _screened), the one-launch kernel was launched
  void tiles_recorded(int pairs) { tile_pairs = pairs; }
  // the kernel about to be launched as the call's last one writes its records here (a group call's fold replaces its half's)
  double* writes_host(double* pinned) { token = 0.0; return host = pinned; }
  // ... and behind them `fresh` -- 0 where the call is timed (events needed), that kernel is no single workgroup or there is no
  // pinned memory.  Whatever an earlier call left in the token's word (a record of a call with more segments) cannot pass for it
  double arm_token(bool single_workgroup, int nseg_, double fresh) {
    token = (single_workgroup && !timed && host != nullptr) ? fresh : 0.0;
    if (token != 0.0) host[4 * nseg_ + 2] = 0.0;
    return token;
  }
  // try_one_launch_t: the launch helper declined with 2 (nothing was launched) -- the next sequence names its own pointer
  void one_launch_declined() { host = nullptr; token = 0.0; }
  // the last launch of enqueue_best_leaves / _grow (General, Small), try_one_launch_t (OneLaunch)
  void enqueued(BestKind k, int nseg_, int mode_) { kind = k; nseg = nseg_; mode = mode_; }
  // enqueue_best_screened
  void screened(const void* xs, int xs_dtype, int64_t m, const AcqSpec& acq, int64_t narrow_max_) {
    enqueued(BestKind::Screened, 1, 0);
    screen = Rerun{xs, xs_dtype, m, acq};
    narrow_max = narrow_max_;
  }
  // enqueue_fold (gpso_best_ucb(_grow)_sharded behind the all-gather, gpso_fold_winners): the tile pairs of the half stay
  void folded(int nseg_, bool collective_recorded) {
    enqueued(BestKind::Folded, nseg_, 2);
    coll_timed = collective_recorded;
  }
  // finish_best, payload_out, a ticket's take(): what the record held; it is none again
  BestCall consumed() {
    const BestCall c = *this;
    *this = BestCall{};
    return c;
  }
};

// gpso_best_ucb_begin stores the enqueue's record, gpso_best_ucb_end takes it; Event: the call's completion event
template <typename Event>
struct BestTicket {
  BestCall call;
  Event ev{};
  bool in_use = false;
  void store(const BestCall& c) { call = c; in_use = true; }
  BestCall take() { in_use = false; return call.consumed(); }
};

}  // namespace gpso
