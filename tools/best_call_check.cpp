// csrc/best_call.hpp on its own, on the CPU: every plan constructor and its rerun(), a BestCall after each enqueue kind (the
// transitions in the order api.hip runs them), consumed() back to none, a token armed on a record with no host pointer
// (0, and nothing written), the token's word zeroed where one is armed, and a ticket that stores a call and gives it back
// unchanged.  Exits 0 when every check holds (tests/test_tools_cpu.py builds it with -Wall -Wextra -Werror and runs it).
// By hand, under the sanitizers:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/best_call_check.cpp -o best_call_check
//     ./best_call_check
#include <cstdio>
#include <initializer_list>

#include "../pygpso_amd/csrc/best_call.hpp"

using namespace gpso;

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                   \
    }                                                               \
  } while (0)

static bool same(const BestCall& a, const BestCall& b) {
  return a.kind == b.kind && a.nseg == b.nseg && a.mode == b.mode && a.host == b.host && a.token == b.token && a.timed == b.timed &&
         a.coll_timed == b.coll_timed && a.tile_pairs == b.tile_pairs && a.screen.xs == b.screen.xs &&
         a.screen.xs_dtype == b.screen.xs_dtype && a.screen.m == b.screen.m && a.screen.acq.kind == b.screen.acq.kind &&
         a.screen.acq.latent == b.screen.acq.latent && a.screen.acq.varsigma == b.screen.acq.varsigma &&
         a.screen.acq.incumbent == b.screen.acq.incumbent && a.screen.acq.xi == b.screen.acq.xi;
}

static void plans() {
  double slot[8];
  const BestPlan s = BestPlan::synchronous(true, true);
  CHECK(s.one_launch && s.screen && !s.is_rerun && s.timed && s.slot == nullptr);
  const BestPlan s0 = BestPlan::synchronous(false, false);
  CHECK(s0.one_launch && !s0.screen && !s0.is_rerun && !s0.timed && s0.slot == nullptr);
  const BestPlan t = BestPlan::ticket(slot, true);
  CHECK(!t.one_launch && t.screen && !t.is_rerun && !t.timed && t.slot == slot);
  const BestPlan g = BestPlan::group_half(true);
  CHECK(!g.one_launch && !g.screen && !g.is_rerun && g.timed && g.slot == nullptr);
  // a re-run takes neither sequence that could ask for another, goes to the shared scratch and keeps the plan's timing
  for (const BestPlan& p : {s, s0, t, g}) {
    const BestPlan r = p.rerun();
    CHECK(!r.one_launch && !r.screen && r.is_rerun && r.slot == nullptr && r.timed == p.timed);
    const BestPlan rr = r.rerun();
    CHECK(!rr.one_launch && !rr.screen && rr.is_rerun && rr.slot == nullptr && rr.timed == p.timed);
  }
}

static void calls() {
  double host[4 * 3 + 3];
  for (double& v : host) v = 7.0;
  CHECK(BestCall{}.none());
  // general / small: tiles, the pointer, the token, the kind
  for (const BestKind k : {BestKind::General, BestKind::Small}) {
    BestCall c = BestCall::begun(BestPlan::synchronous(false, false));
    CHECK(c.none() && !c.timed && c.host == nullptr && c.token == 0.0);
    c.tiles_recorded(2);
    c.writes_host(host);
    host[4 * 3 + 2] = 7.0;
    CHECK(c.arm_token(true, 3, 41.0) == 41.0 && c.token == 41.0 && host[4 * 3 + 2] == 0.0 && host[4 * 3 + 1] == 7.0);
    c.enqueued(k, 3, 1);
    CHECK(c.kind == k && c.nseg == 3 && c.mode == 1 && c.host == host && c.tile_pairs == 2 && !c.coll_timed && !c.none());
    const BestCall held = c.consumed();
    CHECK(c.none() && same(c, BestCall{}) && held.kind == k && held.token == 41.0 && held.host == host);
  }
  // no token: several workgroups, a timed call, no pinned memory -- and then nothing is written
  {
    BestCall c = BestCall::begun(BestPlan::synchronous(false, false));
    CHECK(c.arm_token(true, 3, 5.0) == 0.0 && c.token == 0.0);  // (no host pointer)
    c.writes_host(host);
    host[4 * 3 + 2] = 7.0;
    CHECK(c.arm_token(false, 3, 5.0) == 0.0 && host[4 * 3 + 2] == 7.0);
    BestCall timed = BestCall::begun(BestPlan::synchronous(true, false));
    timed.writes_host(host);
    CHECK(timed.timed && timed.arm_token(true, 3, 5.0) == 0.0 && host[4 * 3 + 2] == 7.0);
    // a later pointer drops an earlier token
    CHECK(c.arm_token(true, 3, 6.0) == 6.0);
    c.writes_host(host);
    CHECK(c.token == 0.0);
  }
  // one-launch: declined with 2 -> neither pointer nor token; launched -> its kind
  {
    BestCall c = BestCall::begun(BestPlan::synchronous(false, false));
    c.writes_host(host);
    CHECK(c.arm_token(true, 2, 9.0) == 9.0);
    c.one_launch_declined();
    CHECK(c.none() && c.host == nullptr && c.token == 0.0 && c.arm_token(true, 2, 10.0) == 0.0);
    c.writes_host(host);
    c.arm_token(true, 2, 11.0);
    c.tiles_recorded(0);
    c.enqueued(BestKind::OneLaunch, 2, 1);
    CHECK(c.kind == BestKind::OneLaunch && c.nseg == 2 && c.mode == 1 && c.token == 11.0);
    c.consumed();
    CHECK(c.none() && c.host == nullptr && c.token == 0.0);
  }
  // screened: one segment, winners only, and what a re-run takes
  {
    const float leaves[2] = {0.0f, 1.0f};
    BestCall c = BestCall::begun(BestPlan::ticket(host, true));
    c.tiles_recorded(1);
    c.writes_host(host);
    c.arm_token(true, 1, 12.0);
    c.screened(leaves, 1, 24000, AcqSpec(50.0), 15744);
    CHECK(c.kind == BestKind::Screened && c.nseg == 1 && c.mode == 0 && c.screen.xs == leaves && c.screen.xs_dtype == 1 &&
          c.screen.m == 24000 && c.screen.acq.varsigma == 50.0 && c.narrow_max == 15744 && c.token == 12.0 && host[4 + 2] == 0.0);
    CHECK(c.consumed().screen.m == 24000 && c.none() && c.screen.xs == nullptr && c.screen.m == 0);
  }
  // folded: the half's tile pairs stay, the half's pointer and token are replaced
  {
    BestCall c = BestCall::begun(BestPlan::group_half(true));
    c.tiles_recorded(3);
    c.writes_host(host);
    c.arm_token(true, 3, 13.0);
    c.enqueued(BestKind::General, 3, 0);
    c.writes_host(host);
    c.arm_token(true, 3, 14.0);
    c.folded(3, true);
    CHECK(c.kind == BestKind::Folded && c.nseg == 3 && c.mode == 2 && c.coll_timed && c.tile_pairs == 3 && c.timed && c.token == 0.0);
    c.consumed();
    CHECK(c.none() && !c.coll_timed && c.tile_pairs == 0 && !c.timed);
  }
}

static void tickets() {
  double host[8] = {0};
  BestTicket<int> t;
  CHECK(!t.in_use && t.call.none());
  BestCall c = BestCall::begun(BestPlan::ticket(host, true));
  c.tiles_recorded(1);
  c.writes_host(host);
  c.arm_token(true, 1, 21.0);
  c.screened(host, 1, 512, AcqSpec(2, 1, 0.5, 0.25, 0.125), 512);
  t.ev = 5;
  t.store(c);
  CHECK(t.in_use && same(t.call, c));
  const BestCall back = t.take();
  CHECK(same(back, c) && !t.in_use && t.call.none() && same(t.call, BestCall{}) && t.ev == 5);
}

int main() {
  plans();
  calls();
  tickets();
  if (failures) {
    std::fprintf(stderr, "best_call_check: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("best_call_check: ok\n");
  return 0;
}
