// gpso_paths_batch_host on its own, on the CPU, for the host sanitizers: the shapes of
// tests/test_mcbatch_cpu.py -- S in {1, 17, 129}, m in {1, 5, 65}, b in {0, 3}, q in {1, 2, 64}, both kinds, scalar and per-draw
// bars -- with every buffer exactly as long as the call may touch (the sanitizer sees a read or write past it), the rules
// (a NaN column, copies of the winner, -inf bars, nothing to improve) and every refusal.  It checks what needs no oracle:
// picks distinct and in range, QEI gains never rising, batch_value the running sum and -- recomputed from the picks -- the
// batch's sample-average value.  Exits 0 when every check holds.  Against the sanitizer build of the library:
//     make -C pygpso_amd/csrc -j8 asan
//     CXX=/opt/rocm/llvm/bin/clang++; RT=$(dirname $($CXX -print-file-name=libclang_rt.asan-x86_64.so))
//     $CXX -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -shared-libsan
//         tools/mcbatch_host_check.cpp -Iinclude -Lpygpso_amd -lgpso_hip_asan -Wl,-rpath,$PWD/pygpso_amd -Wl,-rpath,$RT
//         -o mcbatch_host_check && ./mcbatch_host_check          (one command line)
// (a stand-alone program: its own main, no Python, nothing preloaded, no GPU -- the host call makes no HIP call; the
// compiler is the one hipcc drives, so the program and the library share one sanitizer runtime)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <set>
#include <vector>

#include "gpso_hip.h"

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                   \
    }                                                               \
  } while (0)

static uint64_t state = 88172645463325252ull;
static double uniform() {  // xorshift64: (0, 1)
  state ^= state << 13;
  state ^= state >> 7;
  state ^= state << 17;
  return ((double)(state >> 11) + 0.5) / 9007199254740992.0;
}
static double normal() { return std::sqrt(-2.0 * std::log(uniform())) * std::cos(6.283185307179586 * uniform()); }

struct Out {
  int rc, n;
  std::vector<int64_t> idx;
  std::vector<double> gain, value, gain0;
};

static Out run(int kind, double xi, double inc, const std::vector<double>& V, int64_t s, int64_t m, int b, const std::vector<double>* bars,
               int q, bool want = true) {
  Out o;
  o.idx.assign((size_t)q, -7);
  o.gain.assign((size_t)q, -7.0);
  o.value.assign((size_t)q, -7.0);
  o.gain0.assign((size_t)m, -7.0);
  o.n = -1;
  gpso_mcacq acq{kind, xi, inc};
  o.rc = gpso_paths_batch_host(&acq, V.data(), s, m, b, bars ? bars->data() : nullptr, q, o.idx.data(), want ? o.gain.data() : nullptr,
                               want ? o.value.data() : nullptr, &o.n, want ? o.gain0.data() : nullptr);
  return o;
}

static void random_case(int64_t s, int64_t m, int b, int q, int kind, bool per_draw) {
  std::vector<double> V((size_t)(s * (m + b))), bars((size_t)s);
  for (double& v : V) v = normal();
  for (double& t : bars) t = -0.5 + 0.1 * normal();
  const double xi = per_draw ? 0.01 : 0.0, inc = -1.0;
  const Out o = run(kind, xi, inc, V, s, m, b, per_draw ? &bars : nullptr, q);
  CHECK(o.rc == GPSO_OK && o.n >= 1 && o.n <= q && o.n <= m);
  std::set<int64_t> seen;
  double sum = 0.0;
  for (int t = 0; t < o.n; ++t) {
    CHECK(o.idx[t] >= 0 && o.idx[t] < m && seen.insert(o.idx[t]).second);
    sum = t == 0 ? o.gain[t] : sum + o.gain[t];
    CHECK(o.value[t] == sum);
    if (t > 0) CHECK(o.gain[t] > 0.0);
    if (t > 0 && kind == GPSO_MC_QEI) CHECK(o.gain[t] <= o.gain[t - 1]);
  }
  CHECK(o.gain[0] == o.gain0[o.idx[0]]);
  for (int64_t j = 0; j < m; ++j) CHECK(o.gain0[j] <= o.gain[0] && o.gain0[j] >= 0.0);
  for (int t = o.n; t < q; ++t) CHECK(o.idx[t] == -7 && o.gain[t] == -7.0 && o.value[t] == -7.0);  // not written
  if (kind == GPSO_MC_QEI) {  // the batch's value from its definition: improvements over the original bars, beyond the pending points'
    double total = 0.0;
    for (int64_t d = 0; d < s; ++d) {
      const double t0 = per_draw ? bars[d] : inc;
      double held = 0.0, best = 0.0;
      for (int c = 0; c < b; ++c) held = std::fmax(held, V[d * (m + b) + m + c] - t0 - xi);
      for (int t = 0; t < o.n; ++t) best = std::fmax(best, V[d * (m + b) + o.idx[t]] - t0 - xi);
      total += std::fmax(best - held, 0.0);
    }
    CHECK(std::fabs(total / (double)s - o.value[o.n - 1]) <= 1e-12 * (1.0 + std::fabs(total)));
  }
  const Out bare = run(kind, xi, inc, V, s, m, b, per_draw ? &bars : nullptr, q, false);  // every optional output NULL
  CHECK(bare.rc == GPSO_OK && bare.n == o.n && bare.idx == o.idx);
}

static void rules() {
  const int64_t s = 17, m = 9;
  std::vector<double> V((size_t)(s * m));
  for (double& v : V) v = normal();
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (int kind : {GPSO_MC_QEI, GPSO_MC_QPI}) {
    std::vector<double> W = V;
    W[5 * m + 6] = nan;  // a NaN column wins and ends the batch
    Out o = run(kind, 0.0, -1.0, W, s, m, 0, nullptr, 4);
    CHECK(o.rc == GPSO_OK && o.n == 1 && o.idx[0] == 6 && o.gain[0] != o.gain[0]);
    o = run(kind, 0.0, 100.0, V, s, m, 0, nullptr, 4);  // nothing to improve: round 0's pick, then the end
    CHECK(o.rc == GPSO_OK && o.n == 1 && o.idx[0] == 0 && o.gain[0] == 0.0);
    o = run(kind, 0.0, -inf, V, s, m, 0, nullptr, 3);  // -inf bars: the first row wins round 0
    CHECK(o.rc == GPSO_OK && o.n >= 1 && o.idx[0] == 0 && (kind == GPSO_MC_QEI ? std::isinf(o.gain[0]) : o.gain[0] == 1.0));
    // two copies of the winner behind the batch are never picked, whatever the margin
    for (double xi : {0.0, 0.05, -0.05}) {
      const Out first = run(kind, xi, -1.0, V, s, m, 0, nullptr, 1);
      std::vector<double> D((size_t)(s * (m + 2)));
      for (int64_t d = 0; d < s; ++d) {
        for (int64_t j = 0; j < m; ++j) D[d * (m + 2) + j] = V[d * m + j];
        D[d * (m + 2) + m] = D[d * (m + 2) + m + 1] = V[d * m + first.idx[0]];
      }
      o = run(kind, xi, -1.0, D, s, m + 2, 0, nullptr, 11);
      CHECK(o.rc == GPSO_OK && o.idx[0] == first.idx[0]);
      for (int t = 1; t < o.n; ++t) CHECK(o.idx[t] != m && o.idx[t] != m + 1);
    }
  }
}

static void refusals() {
  std::vector<double> V(4 * 8, 0.25), bars(4, 0.0);
  std::vector<int64_t> idx(64);
  int n = 0;
  gpso_mcacq acq{GPSO_MC_QEI, 0.0, 0.0};
  const double nan = std::numeric_limits<double>::quiet_NaN();
  auto call = [&](const gpso_mcacq* a, const double* v, int64_t s, int64_t m, int b, const double* t, int q, int64_t* i, int* np) {
    return gpso_paths_batch_host(a, v, s, m, b, t, q, i, nullptr, nullptr, np, nullptr);
  };
  CHECK(call(&acq, V.data(), 4, 6, 2, nullptr, 2, idx.data(), &n) == GPSO_OK);
  CHECK(call(nullptr, V.data(), 4, 6, 2, nullptr, 2, idx.data(), &n) == GPSO_E_ARG);
  CHECK(call(&acq, nullptr, 4, 6, 2, nullptr, 2, idx.data(), &n) == GPSO_E_ARG);
  CHECK(call(&acq, V.data(), 4, 6, 2, nullptr, 2, nullptr, &n) == GPSO_E_ARG);
  CHECK(call(&acq, V.data(), 4, 6, 2, nullptr, 2, idx.data(), nullptr) == GPSO_E_ARG);
  for (int64_t s : {(int64_t)0, (int64_t)257}) CHECK(call(&acq, V.data(), s, 6, 2, nullptr, 2, idx.data(), &n) == GPSO_E_ARG);
  for (int64_t m : {(int64_t)0, (int64_t)-1, ((int64_t)1 << 26)}) CHECK(call(&acq, V.data(), 4, m, 2, nullptr, 2, idx.data(), &n) == GPSO_E_ARG);
  for (int q : {0, 65}) CHECK(call(&acq, V.data(), 4, 6, 2, nullptr, q, idx.data(), &n) == GPSO_E_ARG);
  for (int b : {-1, 65}) CHECK(call(&acq, V.data(), 4, 6, b, nullptr, 2, idx.data(), &n) == GPSO_E_ARG);
  for (gpso_mcacq bad : {gpso_mcacq{2, 0.0, 0.0}, gpso_mcacq{-1, 0.0, 0.0}, gpso_mcacq{GPSO_MC_QEI, nan, 0.0}, gpso_mcacq{GPSO_MC_QPI, 0.0, nan}})
    CHECK(call(&bad, V.data(), 4, 6, 2, nullptr, 2, idx.data(), &n) == GPSO_E_ARG);
  bars[3] = nan;
  CHECK(call(&acq, V.data(), 4, 6, 2, bars.data(), 2, idx.data(), &n) == GPSO_E_ARG);
  bars[3] = -std::numeric_limits<double>::infinity();
  gpso_mcacq unread{GPSO_MC_QEI, -0.5, nan};  // (the scalar is not read beside per-draw bars)
  CHECK(call(&unread, V.data(), 4, 6, 2, bars.data(), 2, idx.data(), &n) == GPSO_OK);
}

int main() {
  for (int64_t s : {(int64_t)1, (int64_t)17, (int64_t)129})
    for (int64_t m : {(int64_t)1, (int64_t)5, (int64_t)65})
      for (int b : {0, 3})
        for (int q : {1, 2, 64})
          for (int kind : {GPSO_MC_QEI, GPSO_MC_QPI})
            for (bool per_draw : {false, true}) random_case(s, m, b, q, kind, per_draw);
  rules();
  refusals();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::puts("mcbatch_host_check: ok");
  return 0;
}
