"""Max-value entropy search without a GPU: the host twins of the device map (``gpso_acq_mes_eval_host``) and of the
max-CDF reduction (``gpso_max_logcdf_host``) against the 60-digit truth of tests/mes_oracle.py, the rules of the map, the
Python specs, and the Gumbel fit of pygpso_amd/mes.py."""
import math

import mpmath as mp
import numpy as np
import pytest
from scipy import special as sp

from pygpso_amd import HipGPEngine
from pygpso_amd import _lib as L
from pygpso_amd import acquisition as A
from pygpso_amd import mes
from tests import mes_oracle as MO

E = HipGPEngine


def test_the_map_meets_the_tolerance_on_the_grid():
    ystar, mean, s2 = MO.grid()
    tol, own = MO.tolerance()
    got = np.array([E.acq_mes_eval_host([y], [m], [v], latent=False)[0] for y, m, v in zip(ystar, mean, s2)])
    err = MO.error(got, MO.grid_truth())
    worst = max(range(len(got)), key=lambda i: MO.error(got[i:i + 1], MO.grid_truth()[i:i + 1]))
    print(f"library {err / MO.ULP:.2f} ulp (worst at y*={ystar[worst]}, s2={s2[worst]}); restatement {own / MO.ULP:.2f} ulp; "
          f"tolerance {tol / MO.ULP:.2f} ulp")
    assert err <= tol, (err / MO.ULP, tol / MO.ULP)
    # (the form a careful user would build from log_ndtr is far outside it: what the three pieces are for)
    g = -38.0
    naive = 0.5 * g * np.exp(-0.5 * g * g - 0.5 * np.log(2 * np.pi) - sp.log_ndtr(g)) - sp.log_ndtr(g)
    assert MO.error([naive], MO.truth([g], [0.0], [1.0])) > max(1e4 * MO.ULP, 10.0 * tol)


def test_k_3_across_the_three_pieces_is_the_index_ordered_mean():
    mean, s2 = np.array([0.25]), np.array([0.49])
    ystar = np.array([0.25 + 0.7 * 2.0, 0.25 - 0.7 * 5.0, 0.25 - 0.7 * 40.0])  # g about 2, -5, -40: one leaf in all three pieces
    g = (ystar - mean[0]) / 0.7
    assert g[0] >= -1.0 and -10.0 < g[1] < -1.0 and g[2] <= -10.0
    singles = [E.acq_mes_eval_host([y], mean, s2, latent=False)[0] for y in ystar]
    got = E.acq_mes_eval_host(ystar, mean, s2, latent=False)[0]
    assert got == ((singles[0] + singles[1]) + singles[2]) / 3.0
    assert MO.error([got], MO.truth(ystar, mean, s2)) <= MO.tolerance()[0]
    # (the order is the index order: another one gives other bits somewhere on a spread of leaves)
    means = np.linspace(-3.0, 3.0, 41)
    fwd = E.acq_mes_eval_host(ystar, means, np.full(41, 0.49), latent=False)
    for i, m in enumerate(means):
        t = [E.acq_mes_eval_host([y], [m], [0.49], latent=False)[0] for y in ystar]
        assert fwd[i] == ((t[0] + t[1]) + t[2]) / 3.0


def test_zero_variance_nan_and_latent_rules():
    ystar = [0.5, -0.25]
    assert np.array_equal(E.acq_mes_eval_host(ystar, [2.0, 0.5, -2.0], [0.0, 0.0, 0.0], latent=False), [0.0, 0.0, 0.0])
    assert np.array_equal(E.acq_mes_eval_host(ystar, [2.0, -2.0], [-1e-3, -0.0], latent=False), [0.0, 0.0])  # (clamped at 0)
    got = E.acq_mes_eval_host(ystar, [np.nan, 0.0, np.nan], [1.0, np.nan, np.nan], latent=False)
    assert np.all(np.isnan(got))
    # latent: the map reads var - noise
    mean, var, noise = np.array([0.1, -0.3, 0.7]), np.array([0.5, 0.25, 0.0625 + 0.015625]), 0.015625
    lat = E.acq_mes_eval_host(ystar, mean, var, noise=noise, latent=True)
    assert np.array_equal(lat, E.acq_mes_eval_host(ystar, mean, var - noise, latent=False))
    assert not np.array_equal(lat, E.acq_mes_eval_host(ystar, mean, var, noise=noise, latent=False))
    assert MO.error(lat, MO.truth(ystar, mean, var, s2_add=(-noise,))) <= MO.tolerance()[0]
    assert np.array_equal(E.acq_mes_eval_host(ystar, [0.3], [noise], noise=noise, latent=True), [0.0])
    # bad maxima
    for bad in ([], [np.nan], [np.inf], list(range(65))):
        with pytest.raises(L.GpsoHipError) as err:
            E.acq_mes_eval_host(bad, [0.0], [1.0])
        assert err.value.code == L.E_ARG


def test_values_are_non_negative_and_grow_with_s_below_the_maximum():
    ystar = [1.0, 1.5, 4.0]
    for mean in (0.9, 0.0, -7.0):  # mean < every y*
        s = np.geomspace(1e-6, 1e4, 200)
        val = E.acq_mes_eval_host(ystar, np.full(200, mean), s * s, latent=False)
        assert np.all(np.isfinite(val)) and np.all(val >= 0.0)
        assert np.all(np.diff(val) >= 0.0), (mean, np.where(np.diff(val) < 0.0))
    # across the joins of the pieces at fixed s: g sweeps -12 .. 2, the value stays finite, non-negative and decreasing in g
    g = np.linspace(-12.0, 2.0, 200)
    val = E.acq_mes_eval_host([0.0], -g, np.ones(200), latent=False)
    assert np.all(np.isfinite(val)) and np.all(val >= 0.0) and np.all(np.diff(val) < 0.0)


def _leaves(m, seed):
    rng = np.random.default_rng(seed)
    mean = rng.normal(0.0, 1.0, m)
    var = rng.uniform(0.01, 2.0, m)
    return mean, var


@pytest.mark.parametrize("g", [1, 64])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 4097])
def test_max_logcdf_host_against_truth(m, g):
    mean, var = _leaves(m, seed=m)
    var_sub = 0.005
    if m >= 63:
        mean[5], var[9] = np.nan, np.nan  # skipped rows
        var[11] = var_sub                 # s = 0 rows: one far below every threshold but the lowest ones, one that
        mean[11] = -9.0                   # decides the sign (a threshold on it, thresholds on both sides)
        var[17], mean[17] = 0.001, 0.125  # (var - var_sub < 0: clamped)
    # from far below every mean (z < -10: the tail form; finite) to far above (the sum rounds to 0 from below)
    y = np.array([0.125]) if g == 1 else np.concatenate([np.linspace(-60.0, 8.0, 61), [-9.0, 0.125, 40.0]])
    got, used = E.max_logcdf_host(mean, var, y, var_sub, want_used=True)
    if m * g <= 8192:
        want, n = MO.truth_logcdf(mean, var, y, var_sub)
        own = MO.error(MO.restatement_logcdf(mean, var, y, var_sub)[0], want)
    else:  # (60 digits on 4097 x 64 terms take a minute: 200 rows of them, the exactly rounded float64 sum for the rest)
        want, n, own = MO.truth_logcdf_sampled(mean, var, y, var_sub, n_exact=200)
    assert used == n == m - (2 if m >= 63 else 0)
    tol = MO.logcdf_tolerance(m, own)
    err = MO.error(got, want)
    print(f"m={m} g={g}: library {err / MO.ULP:.2f} ulp, restatement {own / MO.ULP:.2f} ulp, tolerance {tol / MO.ULP:.2f} ulp")
    assert err <= tol
    if m >= 63 and g == 64:
        assert np.isneginf(got[y < 0.125]).all() and np.isfinite(got[y >= 0.125]).all()  # (row 17: s = 0 at mean 0.125)
    # without the s = 0 rows every threshold gives a finite number, however far below
    if m >= 63:
        keep = np.ones(m, bool)
        keep[[11, 17]] = False
        far = E.max_logcdf_host(mean[keep], var[keep], y, var_sub)
        assert np.all(np.isfinite(far)) and np.all(far <= 0.0)
        if m * g <= 8192:
            assert MO.error(far, MO.truth_logcdf(mean[keep], var[keep], y, var_sub)[0]) <= tol
    for bad_y in ([], [np.nan], np.zeros(65)):
        with pytest.raises(L.GpsoHipError):
            E.max_logcdf_host(mean, var, bad_y)


def test_names_records_and_what_is_out_of_scope():
    spec = A.resolve("mes")
    assert isinstance(spec, A.MES) and spec.kind == L.ACQ_MES == 5 and spec.latent and spec.maxima is None and not spec.score_units
    assert np.array_equal(A.resolve("mes", maxima=[1.0, 2.0], latent=False).maxima, [1.0, 2.0])
    with pytest.raises(ValueError) as mes_err:
        A.score_unit_spec("mes", 1.0)
    with pytest.raises(ValueError) as ei_err:
        A.score_unit_spec("ei", 1.0)
    assert str(mes_err.value).replace("'mes'", "'ei'") == str(ei_err.value)
    # gpso_acq_eval_host cannot see the maxima
    rec = A.MES().c_struct()
    out = np.zeros(1)
    one = np.ones(1)
    assert L.load().gpso_acq_eval_host(rec, L.dptr(one), L.dptr(one), 0.0, 1, L.dptr(out)) == L.E_ARG
    with pytest.raises(L.GpsoHipError):
        E.acq_eval_host(A.MES(maxima=[1.0]), [0.0], [1.0])
    # the host greedy twin under MES: its first pick is the arg-max of the host map
    rng = np.random.default_rng(3)
    Bm = rng.normal(size=(12, 12))
    cov = Bm @ Bm.T / 12.0
    mean, noise = rng.normal(size=12), 0.01
    s2 = np.diag(cov) + noise
    ystar = [2.0, 2.5]
    idx, var, val, after = E.batch_greedy_mes_host(ystar, mean, s2, cov, noise, noise, 3, latent=True)
    col = E.acq_mes_eval_host(ystar, mean, s2, noise=noise, latent=True)
    assert len(idx) == 3 and len(set(idx)) == 3 and idx[0] == int(np.argmax(col)) and val[0] == col[idx[0]] and var[0] == s2[idx[0]]
    assert np.all(after <= s2)


def test_the_gumbel_fit_recovers_the_quartiles_of_a_known_law():
    """512 leaves of one mean and one variance: P(y* < y) = Phi((y - mu) / s)^512, whose quantiles are known in closed form,
    y_p = mu + s Phi^-1(p^(1/512)).  The bar: each fitted quartile lies within ONE spacing of the fine grid of the exact one
    -- the interpolation's input is known on that grid, between two neighbours it is a straight line in logcdf.  The
    coarse grid spans [mu, mu + 6 s] in 63 steps, the fine one the (at most) few coarse cells that hold the three
    quartiles in 63 steps again: its spacing h is returned by the fit and asserted below to be under s / 100.  (a, b)
    then follow from the quartiles by the two formulas of pygpso_amd/mes.py, so they are within the propagated bound of
    the same formulas applied to the exact quartiles."""
    m, mu, s = 512, 0.75, 0.4
    mean, var = np.full(m, mu), np.full(m, s * s)
    calls = []

    def logcdf(y):
        calls.append(len(y))
        return E.max_logcdf_host(mean, var, y)

    a, b, q, h = mes.gumbel_fit(logcdf, mu, mu + 6.0 * s)
    assert calls == [64, 64]
    assert 0.0 < h < s / 100.0
    exact = np.array([float(mu + s * mp.sqrt(2) * mp.erfinv(2 * mp.mpf(p) ** (mp.mpf(1) / m) - 1)) for p in (0.25, 0.5, 0.75)])
    assert np.all(np.abs(q - exact) <= h), (q - exact, h)
    den = abs(math.log(math.log(4.0 / 3.0)) - math.log(math.log(4.0)))
    b_exact = (exact[2] - exact[0]) / den
    a_exact = exact[1] + b_exact * math.log(math.log(2.0))
    assert b > 0.0 and abs(b - b_exact) <= 2.0 * h / den
    assert abs(a - a_exact) <= h + abs(math.log(math.log(2.0))) * 2.0 * h / den
    # a law that IS a Gumbel's (its logcdf handed over directly): (a, b) come back to the interpolation's accuracy
    a0, b0 = 1.25, 0.3
    a1, b1, _, h1 = mes.gumbel_fit(lambda y: -np.exp(-(y - a0) / b0), a0 - 2.0 * b0, a0 + 4.0 * b0)
    assert abs(b1 - b0) <= 2.0 * h1 / den and abs(a1 - a0) <= h1 + abs(math.log(math.log(2.0))) * 2.0 * h1 / den
    # a bracket that misses the quartiles is widened, a seed reproduces the draws, the clamp holds
    a2, b2, _, _ = mes.gumbel_fit(lambda y: -np.exp(-(y - a0) / b0), a0 + 1.0, a0 + 1.5)
    assert abs(a2 - a0) < 0.05 and abs(b2 - b0) < 0.05
    d1, d2 = mes.gumbel_draw(a, b, 16, 7), mes.gumbel_draw(a, b, 16, np.random.default_rng(7))
    assert np.array_equal(d1, d2) and np.all(np.isfinite(d1))
    assert np.all(mes.clamp_at(d1, 2.0) >= 2.0) and np.array_equal(mes.clamp_at(d1, -1e9), d1)


def _ulps(got, want):
    worst = 0.0
    for g, w in zip(got, want):
        den = max(abs(w), mp.mpf(2) ** -1022)
        worst = max(worst, float(abs(mp.mpf(float(g)) - w) / den) / MO.ULP)
    return worst


def test_the_written_out_functions_against_mpmath():
    """exp, log, log1p, erfc and the Mills table of csrc/acq.hpp on their own (``gpso_acq_math_host``), 2 000 arguments each
    over what the maps send them, against mpmath at 60 digits.  Bounds, from how each is built: exp and log are msun's,
    documented below 1 ulp; log1p = log(u) x / (u - 1) adds a division and a product, 2 ulp; erfc = t h(t) exp(-x^2) (1 - lo):
    t 1 ulp, the 32-term recurrence on coefficients rounded to float64 2 ulp, exp 1 ulp, three products 1.5 ulp -- 6 ulp,
    down to the subnormals; the Mills table p: its argument 1 / T 1 ulp (p' w / p < 1), the 44-term recurrence 2.5 ulp -- 4 ulp."""
    rng = np.random.default_rng(0)
    cases = {
        "exp": (np.concatenate([rng.uniform(-745.0, 5.0, 1500), rng.uniform(-1.0, 1.0, 500), [0.0, -708.5, -744.9, -1e-20]]), mp.exp, 1.0),
        "log": (np.concatenate([np.exp(rng.uniform(-700.0, 700.0, 1000)), rng.uniform(0.5, 2.0, 1000), [1.0, 5e-324, 1e-310, 2.0 ** -0.5]]),
                mp.log, 1.0),
        "log1p": (np.concatenate([-np.exp(rng.uniform(-80.0, np.log(0.5), 1500)), np.exp(rng.uniform(-50.0, 3.0, 500)), [0.0, -0.5, -1e-17]]),
                  mp.log1p, 2.0),
        "erfc": (np.concatenate([rng.uniform(0.0, 28.0, 1500), rng.uniform(-6.0, 0.0, 250), np.exp(rng.uniform(-40.0, 0.0, 250)),
                                 [0.0, 26.5, 27.2, 39.0, 45.0]]), mp.erfc, 6.0),
        "mills_p": (np.concatenate([rng.uniform(1.0, 10.0, 1990), [1.0, 10.0, 9.999, 1.0000001, 6.0]]),
                    lambda t: t * t * (1 - t * mp.sqrt(mp.pi / 2) * mp.erfc(t / mp.sqrt(2)) * mp.exp(t * t / 2)), 4.0),
    }
    for name, (x, ref, bound) in cases.items():
        got = E.acq_math_host(name, x)
        worst = _ulps(got, [ref(mp.mpf(float(v))) for v in x])
        print(f"{name}: {worst:.2f} ulp (bound {bound})")
        assert worst <= bound, (name, worst)
    assert E.acq_math_host("log", [0.0, -1.0])[0] == -np.inf and np.isnan(E.acq_math_host("log", [-1.0])[0])
    assert E.acq_math_host("exp", [-800.0])[0] == 0.0 and E.acq_math_host("erfc", [-50.0])[0] == 2.0
    assert L.load().gpso_acq_math_host(9, L.dptr(np.zeros(1)), 1, L.dptr(np.zeros(1))) == L.E_ARG


def test_the_header_holds_the_tables_the_fit_script_prints():
    import subprocess
    import sys
    from pathlib import Path

    root = Path(__file__).resolve().parents[1]
    done = subprocess.run([sys.executable, str(root / "tools" / "fit_acq_tables.py"), "--check"], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
