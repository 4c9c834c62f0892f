// csrc/fit_call.hpp on its own, on the CPU: every FitPlan for {grad, LOO, small, timed} and its derived members, the wait rule
// over all of (small, LOO, timed, token armed) against the table written out below, a token's word zeroed where one is armed
// (and no other word touched), a record with no scratch (no token, nothing written, no pointer handed out), and the sizes of
// the scratch map.  Exits 0 when every check holds (tests/test_tools_cpu.py builds it with -Wall -Wextra -Werror and runs it).
// By hand, under the sanitizers:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/fit_call_check.cpp -o fit_call_check
//     ./fit_call_check
#include <cstdio>
#include <cstring>
#include <vector>

#include "../pygpso_amd/csrc/fit_call.hpp"

using namespace gpso;

// the library's constants (kernels.hpp: kGradMaxLs; context.hpp: kHyperHeader, kMaxD)
using Map = FitScratch<64, 8, 48>;
using Call = FitCall<Map>;

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                   \
    }                                                               \
  } while (0)

static void map() {
  static_assert(Map::kScalDoubles == 75 && Map::kReadbackAt == 0 && Map::kReadbackDoubles == 75, "read-backs");
  static_assert(Map::kThetaAt == 128 && Map::kThetaDoubles == 56, "theta stage");
  static_assert(Map::kLooAt == 256 && Map::kLooDoubles == 75 && Map::kTokenSlot == 7, "LOO region");
  static_assert(Map::doubles(false) == 256 && Map::doubles(true) == 331, "what a call asks for");
  using Other = FitScratch<16, 8, 24>;
  static_assert(Other::kScalDoubles == 27 && Other::kThetaDoubles == 32 && Other::doubles(true) == 283 && Other::doubles(false) == 256, "");
  // the regions in order, none into the next, all inside what the call asked for
  CHECK(Map::kReadbackAt + Map::kReadbackDoubles <= Map::kThetaAt);
  CHECK(Map::kThetaAt + Map::kThetaDoubles <= Map::kLooAt);
  CHECK(Map::kThetaAt + Map::kThetaDoubles <= Map::doubles(false));
  CHECK(Map::kLooAt + Map::kLooDoubles <= Map::doubles(true));
  CHECK(Map::kTokenSlot >= 2 && Map::kTokenSlot < 8);  // (behind nlml and info, in front of the gradient)
}

static void plans() {
  for (int bits = 0; bits < 16; ++bits) {
    const bool grad = bits & 1, loo = bits & 2, small = bits & 4, timed = bits & 8;
    for (const int64_t n : {1, 16, 17, 52, 128, 300}) {
      const FitPlan p = FitPlan::make(grad, loo, small, timed, n);
      CHECK(p.grad == grad && p.loo == loo && p.small == small && p.timed == timed && p.n == n);
      CHECK(std::strcmp(p.who, loo ? "gpso_fit_eval_loo" : "gpso_fit_eval") == 0);
      CHECK(p.theta_from_host() == !small);
      CHECK(p.split_deferred() == (grad && !small));
    }
    CHECK(FitPlan::make(grad, loo, small, timed, 1).tile_rows() == (small ? 1 : 8));
    CHECK(FitPlan::make(grad, loo, small, timed, 16).tile_rows() == (small ? 1 : 8));
    CHECK(FitPlan::make(grad, loo, small, timed, 17).tile_rows() == (small ? 2 : 8));
    CHECK(FitPlan::make(grad, loo, small, timed, 52).tile_rows() == (small ? 4 : 8));
    CHECK(FitPlan::make(grad, loo, small, timed, 128).tile_rows() == 8);
    if (!small) CHECK(FitPlan::make(grad, loo, small, timed, 300).tile_rows() == 8);  // (a one-launch plan has N <= 128)
  }
}

// What ends a call, as api.hip's stages arm the tokens: the one-launch fit arms its token (a fresh number on an untimed call,
// 0 on a timed one), the LOO tail arms one only behind a one-launch fit, a dense fit arms none.  `armed`: the sequence
// numbers were fresh (untimed) -- a row with armed = 1 and timed = 1 is the record of an untimed enqueue read under a timed
// plan, which api.hip never produces; the rule still has to answer Stream for the fit token there
struct Row {
  bool small, loo, timed, armed;
  FitWait want;
};
static const Row kTable[16] = {
    // small  loo    timed  armed
    {false, false, false, false, FitWait::Stream},    // dense fit
    {false, false, false, true, FitWait::Stream},     //   (arms nothing)
    {false, false, true, false, FitWait::Stream},     // dense fit, timed
    {false, false, true, true, FitWait::Stream},      //
    {false, true, false, false, FitWait::Stream},     // dense fit + LOO launches: the copy of the LOO scalars is stream work
    {false, true, false, true, FitWait::Stream},      //
    {false, true, true, false, FitWait::Stream},      //
    {false, true, true, true, FitWait::Stream},       //
    {true, false, false, false, FitWait::Stream},     // one-launch fit whose token is 0
    {true, false, false, true, FitWait::FitToken},    // the optimiser loop's call
    {true, false, true, false, FitWait::Stream},      // one-launch fit, timed: events, no token
    {true, false, true, true, FitWait::Stream},       //
    {true, true, false, false, FitWait::Stream},      // one-launch fit + one-workgroup LOO, tokens 0
    {true, true, false, true, FitWait::LooToken},     // ... armed: the LOO kernel is the call's last
    {true, true, true, false, FitWait::Stream},       // ... timed
    {true, true, true, true, FitWait::LooToken},      // (an armed LOO token always wins)
};

static void waits() {
  std::vector<double> mem(Map::doubles(true));
  for (const Row& r : kTable)
    for (const bool grad : {false, true}) {
      const FitPlan plan = FitPlan::make(grad, r.loo, r.small, r.timed, r.small ? 52 : 300);
      Call c = Call::begun(mem.data());
      if (r.small) c.arm_fit_token(r.armed ? 41.0 : 0.0);
      else c.linv_p_left(true);
      if (r.small && r.loo) c.arm_loo_token(r.armed ? 42.0 : 0.0);
      const FitWait how = c.wait_on(plan);
      CHECK(how == r.want);
      if (how == FitWait::FitToken) CHECK(c.token_word(how) == mem.data() + 7 && c.token(how) == 41.0);
      if (how == FitWait::LooToken) CHECK(c.token_word(how) == mem.data() + 256 + 7 && c.token(how) == 42.0);
    }
  // a LOO token alone (no fit token) still ends the call; a fit token under a LOO plan never does
  Call c = Call::begun(mem.data());
  c.arm_loo_token(9.0);
  CHECK(c.wait_on(FitPlan::make(true, true, true, false, 52)) == FitWait::LooToken);
  Call f = Call::begun(mem.data());
  f.arm_fit_token(9.0);
  CHECK(f.wait_on(FitPlan::make(true, true, true, false, 52)) == FitWait::Stream);
  CHECK(f.wait_on(FitPlan::make(true, false, false, false, 300)) == FitWait::Stream);
}

static void records() {
  std::vector<double> mem(Map::doubles(true), 7.0);
  Call c = Call::begun(mem.data());
  CHECK(c.scratch == mem.data() && c.fit_token == 0.0 && c.loo_token == 0.0 && !c.linv_p_deferred);
  CHECK(c.readback() == mem.data() && c.theta_stage() == mem.data() + 128 && c.loo_readback() == mem.data() + 256);
  // arming zeroes the token's word and no other, with a fresh number and with 0 alike
  CHECK(c.arm_fit_token(5.0) == 5.0 && c.fit_token == 5.0 && c.loo_token == 0.0);
  for (size_t i = 0; i < mem.size(); ++i) CHECK(mem[i] == (i == 7 ? 0.0 : 7.0));
  CHECK(c.arm_loo_token(6.0) == 6.0 && c.loo_token == 6.0 && c.fit_token == 5.0);
  for (size_t i = 0; i < mem.size(); ++i) CHECK(mem[i] == (i == 7 || i == 256 + 7 ? 0.0 : 7.0));
  mem[7] = mem[256 + 7] = 3.0;
  CHECK(c.arm_fit_token(0.0) == 0.0 && c.fit_token == 0.0 && mem[7] == 0.0 && mem[256 + 7] == 3.0);
  CHECK(c.arm_loo_token(0.0) == 0.0 && c.loo_token == 0.0 && mem[256 + 7] == 0.0);
  c.linv_p_left(true);
  CHECK(c.linv_p_deferred && c.scratch == mem.data());
  c.linv_p_left(false);
  CHECK(!c.linv_p_deferred);
  // no scratch: no pointer into it, no token, nothing written anywhere -- and the call waits for the stream
  Call none = Call::begun(nullptr);
  CHECK(none.scratch == nullptr && none.readback() == nullptr && none.theta_stage() == nullptr && none.loo_readback() == nullptr);
  CHECK(none.arm_fit_token(8.0) == 0.0 && none.fit_token == 0.0);
  CHECK(none.arm_loo_token(8.0) == 0.0 && none.loo_token == 0.0);
  CHECK(none.wait_on(FitPlan::make(true, true, true, false, 52)) == FitWait::Stream);
  CHECK(none.wait_on(FitPlan::make(false, false, true, false, 52)) == FitWait::Stream);
}

int main() {
  map();
  plans();
  waits();
  records();
  if (failures) {
    std::fprintf(stderr, "fit_call_check: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("fit_call_check: ok\n");
  return 0;
}
