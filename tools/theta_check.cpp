// csrc/theta.hpp on its own, on the CPU: the decoder, copy-out, the chain rule and every rule of the validator, with NaN
// and +-inf slots and n_ls at 1 and at kThetaMaxLs.  Exits 0 when every check holds.  Prints, for a list of u values,
//     <bits of u> <bits of softplus(u)> <bits of 1e-6 + softplus(u)> <bits of sigmoid(u)>
// which pygpso_amd/model.py must reproduce bit for bit (tests/test_tools_cpu.py builds this, runs it and compares).
// By hand, under the sanitizers:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/theta_check.cpp -o theta_check
//     ./theta_check > c.txt && python3 -c "import sys, struct; from pygpso_amd.model import _softplus1 as s, _sigmoid as g
//     h = lambda x: struct.pack('>d', x).hex()
//     for l in sys.stdin:
//         u = struct.unpack('>d', bytes.fromhex(l.split()[0]))[0]; print(h(u), h(s(u)), h(1e-6 + s(u)), h(float(g(u))))" < c.txt | diff c.txt -
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../pygpso_amd/csrc/theta.hpp"

using namespace gpso;

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                   \
    }                                                               \
  } while (0)

static uint64_t bits(double x) {
  uint64_t b;
  std::memcpy(&b, &x, 8);
  return b;
}
static bool same(double a, double b) { return bits(a) == bits(b); }

static void decode_and_back(int n_ls, bool train_mean) {
  // u exactly as long as the call reads (the sanitizer sees a read past it), slots on both branches of softplus
  std::vector<double> u((size_t)n_ls + 2 + (train_mean ? 1 : 0));
  for (size_t k = 0; k < u.size(); ++k) u[k] = (k % 3 == 0 ? -1.5 : k % 3 == 1 ? 0.4 : 31.5) + 0.01 * (double)k;
  Theta th;
  CHECK(theta_from_u(2, u.data(), n_ls, train_mean, 0.375, 1.0e-6, &th) == ThetaDecode::Ok);
  CHECK(th.kernel == 2 && th.n_ls == n_ls);
  for (int k = 0; k < n_ls; ++k) CHECK(same(th.ls[k], gpso_softplus(u[k])));
  CHECK(same(th.variance, gpso_softplus(u[n_ls])));
  CHECK(same(th.lik, 1.0e-6 + gpso_softplus(u[n_ls + 1])));
  CHECK(same(th.mean_c, train_mean ? u[n_ls + 2] : 0.375));
  Theta scale;
  CHECK(theta_from_u(2, u.data(), n_ls, train_mean, 0.375, 0.0, &scale) == ThetaDecode::Ok);
  CHECK(same(scale.lik, gpso_softplus(u[n_ls + 1])));  // (the Student-t scale: no shift)
  CHECK(same(th.with_lik(7.0).lik, 7.0) && same(th.with_lik(7.0).variance, th.variance));

  std::vector<double> out((size_t)n_ls + 3), g((size_t)n_ls + 3), gu(u.size());
  theta_copy_out(th, out.data());
  for (int k = 0; k < n_ls; ++k) CHECK(same(out[k], th.ls[k]));
  CHECK(same(out[n_ls], th.variance) && same(out[n_ls + 1], th.lik) && same(out[n_ls + 2], th.mean_c));
  for (size_t k = 0; k < g.size(); ++k) g[k] = 0.25 - (double)k;
  grad_to_u(u.data(), n_ls, train_mean, g.data(), gu.data());
  for (int k = 0; k < n_ls + 2; ++k) CHECK(same(gu[k], g[k] * gpso_sigmoid(u[k])));
  if (train_mean) CHECK(same(gu[n_ls + 2], g[n_ls + 2]));

  Theta parts;
  theta_from_parts(2, out.data(), n_ls, out[n_ls], out[n_ls + 1], out[n_ls + 2], &parts);
  CHECK(!theta_refusal(parts, n_ls, true));
  for (int k = 0; k < n_ls; ++k) CHECK(same(parts.ls[k], th.ls[k]));
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (int n_ls : {1, 3, kThetaMaxLs})
    for (bool train_mean : {false, true}) decode_and_back(n_ls, train_mean);

  // what the decoder refuses, without reading u or writing theta
  Theta th;
  double u4[4] = {0.1, 0.2, 0.3, 0.4};
  CHECK(theta_from_u(0, nullptr, 1, true, 0.0, 1.0e-6, &th) == ThetaDecode::NullU);
  CHECK(theta_from_u(0, u4, 0, true, 0.0, 1.0e-6, &th) == ThetaDecode::NlsRange);
  CHECK(theta_from_u(0, u4, -1, true, 0.0, 1.0e-6, &th) == ThetaDecode::NlsRange);
  CHECK(theta_from_u(0, u4, kThetaMaxLs + 1, true, 0.0, 1.0e-6, &th) == ThetaDecode::NlsRange);
  // more lengthscales than a Theta holds: n_ls is kept for the validator, no more than kThetaMaxLs are read or written
  std::vector<double> many((size_t)kThetaMaxLs, 0.5);
  theta_from_parts(0, many.data(), kThetaMaxLs + 36, 1.0, 1.0, 0.0, &th);
  CHECK(th.n_ls == kThetaMaxLs + 36 && theta_refusal(th, kThetaMaxLs + 36, false).rule == ThetaRule::Nls);

  // the validator: every rule, its precedence, and NaN / +-inf in every slot
  CHECK(theta_from_u(1, u4, 1, true, 0.0, 1.0e-6, &th) == ThetaDecode::Ok);
  CHECK(!theta_refusal(th, 1, true) && !theta_refusal(th, 5, true));  // (n_ls = 1 fits any D)
  CHECK(!theta_shape_refusal(3, 4, 4) && theta_shape_refusal(4, 4, 4).rule == ThetaRule::Kernel);
  CHECK(theta_shape_refusal(-1, 1, 1).index == -1 && theta_shape_refusal(0, 2, 3).rule == ThetaRule::Nls);
  CHECK(theta_shape_refusal(0, 2, 3).index == 2 && theta_shape_refusal(0, 0, 3).rule == ThetaRule::Nls);
  Theta bad = th;
  bad.kernel = 7, bad.n_ls = 2, bad.ls[0] = 0.0, bad.variance = 0.0, bad.lik = 0.0;  // everything wrong at once
  CHECK(theta_refusal(bad, 3, true).rule == ThetaRule::Lik && theta_refusal(bad, 3, false).rule == ThetaRule::Kernel);
  CHECK(theta_refusal(bad, 3, false).index == 7);
  bad.kernel = 0;
  CHECK(theta_refusal(bad, 3, false).rule == ThetaRule::Nls && theta_refusal(bad, 3, false).index == 2);
  bad.ls[1] = -1.0;
  CHECK(theta_refusal(bad, 2, false).rule == ThetaRule::Lengthscale && theta_refusal(bad, 2, false).index == 0);
  bad.ls[0] = 1.0;
  CHECK(theta_refusal(bad, 2, false).index == 1 && same(theta_refusal(bad, 2, false).value, -1.0));
  bad.ls[1] = 1.0;
  CHECK(theta_refusal(bad, 2, false).rule == ThetaRule::Variance && !theta_refusal(bad.with_lik(0.0), 2, false).index);
  bad.variance = 1.0;
  CHECK(!theta_refusal(bad, 2, false) && theta_refusal(bad, 2, true).rule == ThetaRule::Lik);
  for (double v : {nan, -inf, -0.0, 0.0}) {
    Theta t = th;
    t.ls[0] = v;
    CHECK(theta_refusal(t, 1, true).rule == ThetaRule::Lengthscale);
    t = th, t.variance = v;
    CHECK(theta_refusal(t, 1, true).rule == ThetaRule::Variance);
    t = th, t.lik = v;
    CHECK(theta_refusal(t, 1, true).rule == ThetaRule::Lik && !theta_refusal(t, 1, false));
    t = th, t.mean_c = v;
    CHECK(!theta_refusal(t, 1, true));  // (the mean is the caller's business)
  }
  Theta big = th;
  big.ls[0] = big.variance = big.lik = inf;  // +inf is positive: the factorisation, not the validator, has the word on it
  CHECK(!theta_refusal(big, 1, true));
  // u slots that are not finite: softplus(-inf) = 0 and NaN stays NaN -- both refused; softplus(+inf) = +inf
  double special[4] = {-inf, nan, inf, 0.0};
  CHECK(theta_from_u(0, special, 1, true, 0.0, 1.0e-6, &th) == ThetaDecode::Ok);
  CHECK(same(th.ls[0], 0.0) && th.variance != th.variance && th.lik == inf);
  CHECK(theta_refusal(th, 1, true).rule == ThetaRule::Lengthscale);
  CHECK(same(gpso_sigmoid(-inf), 0.0) && same(gpso_sigmoid(inf), 1.0) && gpso_sigmoid(nan) != gpso_sigmoid(nan));

  // the transforms' bits, for the Python twins to reproduce
  std::vector<double> us = {0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1e-300, -1e-300, 1e-17, -1e-17, 29.999, 30.0, 30.001, 36.5, 37.0,
                            700.0, 709.9, 710.0, 1e6, -30.0, -36.5, -37.0, -700.0, -745.2, -800.0, -1e6, inf, -inf,
                            0.6931471805599453, 2.2521684610440906, -6.907754778981887, -13.815509557963773};
  for (int k = 0; k < 400; ++k) us.push_back(-40.0 + 0.2003 * (double)k + 1e-3 * (double)((k * 7919) % 13));
  for (double u : us)
    std::printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits(u), bits(gpso_softplus(u)),
                bits(1.0e-6 + gpso_softplus(u)), bits(gpso_sigmoid(u)));
  if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
  return failures ? 1 : 0;
}
