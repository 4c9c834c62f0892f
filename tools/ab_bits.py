#!/usr/bin/env python3
"""Do two builds of libgpso_hip.so give the SAME BITS?  Every library named on the command line predicts the same leaves
from the same posteriors in a fresh process (a list of engine configurations x shapes); the SHA-1 of mean and variance
are printed side by side, differing rows marked.  A last section hashes (loss, grad_u, theta) of every entry point in the
optimiser's variables u (and of the batch) at the shapes of tests/test_gpu_theta.py; --theta runs that section alone.
--points runs (alone, and only then) the section of the calls that evaluate the posterior at given points: points_section.
--fit runs (alone, and only then) the section of the exact-GP fit call: fit_section, every row once with the library's
timing on and once with it off (the two wait differently); the pairs must agree with each other as well.

    python tools/ab_bits.py [--theta | --points | --fit] pygpso_amd/libgpso_hip_prev.so pygpso_amd/libgpso_hip.so
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [  # dtype, math, generation, contraction (None: leave the default)
    ("float32", "f16x3", "float32", "f32"),
    ("float32", "f16x3", "float32", None),
    ("mixed", "f16x3", "float64", None),
    ("float32", "bf16x6", "float32", None),
    ("float32", "bf16x3", "float32", None),
    ("float32", "native", "float32", None),
    ("float64", None, None, None),
]
SHAPES = [(256, 6, 1000, "Matern52"), (2048, 12, 4096, "Matern52"), (768, 20, 700, "Matern32"), (512, 40, 513, "SquaredExponential")]


def theta_section(out):
    """(loss, grad_u, theta) of the calls in u: the exact GP on every engine type, the families on float64."""
    import numpy as np

    from tests import test_gpu_theta as T

    def put(name, *parts):
        out[name] = hashlib.sha1(b"".join(np.asarray(p, dtype=np.float64).tobytes() for p in parts)).hexdigest()[:12]

    Z = T._problem()[2]
    exact = {dtype: T._engine(dtype) for dtype in ("float64", "float32", "mixed")}
    family = [(entry, lik, T._engine("float64", lik, inducing=not entry.startswith("vgp"))) for entry, lik in T.FAMILY]
    for n_ls, train_mean in T.SHAPES:
        for which in ("ordinary", "branches"):
            u, tag = T._u(n_ls, train_mean, which), f"n_ls={n_ls} mean={int(train_mean)} {which}"
            for dtype, eng in exact.items():
                put(f"fit_eval_u {dtype} {tag}", *eng.fit_eval_u(T.KERNEL, u, n_ls, train_mean, 0.375))
                if dtype != "float32":
                    put(f"fit_eval_loo_u {dtype} {tag}", *eng.fit_eval_loo_u(T.KERNEL, u, n_ls, train_mean, 0.375))
            for entry, lik, eng in family:
                res = getattr(eng, entry)(T.KERNEL, u, n_ls, train_mean, 0.375, **({"Z": Z} if entry.endswith("uz") else {}))
                put(f"{entry} {lik[0]} {tag}", *res)
        a, b = T._u(n_ls, train_mean, "ordinary"), T._u(n_ls, train_mean, "branches")
        bad = a.copy()
        bad[n_ls - 1] = -800.0
        put(f"fit_eval_u_batch n_ls={n_ls} mean={int(train_mean)}",
            *exact["float64"].fit_eval_u_batch(T.KERNEL, np.stack([a, b, bad, 0.5 * (a + b), a + 0.25]), n_ls, train_mean, 0.375))
    for eng in list(exact.values()) + [f[2] for f in family]:
        eng.close()


def points_section(out):
    """Every output of the calls that evaluate the posterior at given points -- predict, acq_values (EI), predict_grad,
    predict_joint, sample_joint (fixed normals), paths_draw + paths_eval (two segments) -- on a float64 and a mixed context,
    from host float64 points and from device float32 points; paths_draw_q + paths_eval after an SGPR install on float64.
    The suite's smallest shapes: N = 129, D = 3, Matern-5/2, noise 1e-3, M = 130; M = 1024 + 130 crosses predict_grad's
    chunk, M = 16384 + 3 paths_eval's (on tests/paths_cases.py's N = 17 case, as the suite's chunking test does)."""
    import numpy as np
    import torch

    from pygpso_amd import HipGPEngine
    from pygpso_amd import acquisition as A
    from tests import paths_cases as pc
    from tests import sgpr_oracle as SG
    from tests.helpers import synthetic_problem

    def put(name, *parts):
        out[name] = hashlib.sha1(b"".join(np.ascontiguousarray(p).tobytes() for p in parts)).hexdigest()[:12]

    def feeds(eng, pts):
        yield "host f64", pts
        yield "device f32", torch.from_numpy(pts.astype(np.float32)).to(torch.device("cuda", eng.device))

    kernel, d, m, seg = "Matern52", 3, 130, np.array([0, 70, 130], dtype=np.int64)
    X, y = synthetic_problem(129, d, seed=17 + 129)
    ls, c = 0.25 * np.sqrt(d) * np.ones(1), float(y.mean())
    pts = pc.points_at(1024 + m, d)
    z = np.random.default_rng(4).standard_normal((3, m))
    Xc, yc = synthetic_problem(17, d, seed=17 + 17)
    ptc = pc.points_at(pc.CHUNK + 3, d)
    for dtype in ("float64", "mixed"):
        eng = HipGPEngine(dtype)
        eng.set_data(X, y)
        eng.fit_eval(kernel, ls, 1.3, 1.0e-3, c, want_grad=False)
        for feed, xs in feeds(eng, pts):
            tag = f"{dtype} {feed}"
            put(f"points predict {tag}", *eng.predict(xs[:m]))
            put(f"points acq_values EI {tag}", *eng.acq_values(xs[:m], A.EI(incumbent=float(y.max())), incumbent=float(y.max())))
            put(f"points predict_grad M=130 {tag}", *eng.predict_grad(xs[:m]))
            put(f"points predict_grad M=1154 {tag}", *eng.predict_grad(xs))
            put(f"points predict_joint {tag}", *eng.predict_joint(xs[:m], 0.25))
            put(f"points sample_joint {tag}", *eng.sample_joint(xs[:m], z, 0.25))
            eng.paths_draw(*pc.inputs(kernel, 17, 64, 129, d, seed=100))
            put(f"points paths_draw + paths_eval {tag}", *eng.paths_eval(xs[:m], seg_off=seg))
        eng.close()
        eng = HipGPEngine(dtype)
        eng.set_data(Xc, yc)
        eng.fit_eval(kernel, ls, 1.3, 1.0e-3, float(yc.mean()), want_grad=False)
        eng.paths_draw(*pc.inputs(kernel, 1, 4, 17, d, seed=110))
        for feed, xs in feeds(eng, ptc):
            put(f"points paths_eval M=16387 {dtype} {feed}", *eng.paths_eval(xs, seg_off=np.array([0, 70, pc.CHUNK + 3], dtype=np.int64)))
        eng.close()
    eng = HipGPEngine("float64")
    eng.set_data(X, y)
    eng.sgpr_set_inducing(np.ascontiguousarray(X[:33]))
    eng.sgpr_posterior(kernel, SG.initial_u(ls, 1.3, 1.0e-3, c), 1, True, 0.0)
    eng.paths_draw_q(*pc.inputs(kernel, 17, 64, 33, d, seed=120))
    for feed, xs in feeds(eng, pts[:m]):
        put(f"points sgpr paths_draw_q + paths_eval float64 {feed}", *eng.paths_eval(xs, seg_off=seg))
    eng.close()


def fit_section(out):
    """What a fit call leaves behind, through every branch of it (csrc/api.hip: fit_eval_impl's stages) at the
    smallest shapes of the suite that reach it: the one-launch fit, the single-level dense fit, the forced two-level fits
    (double: GPSO_OPT_FIT_OVERLAP 0 / 2 / 3, float: the fp16 and bf16 plane paths), both LOO tails (also behind a plain fit, so
    the pinned scratch grows between the calls), the batch, and gpso_append in place, by refit and refused.  A fit row hashes
    (nlml, grad, GPSO_FITMATH_*, L, L^-1, K^-1 with a gradient, alpha), a LOO row the LOO loss and gradient as well."""
    import numpy as np

    from pygpso_amd import HipGPEngine
    from pygpso_amd import _lib as L
    from tests.helpers import synthetic_leaves, synthetic_problem

    def put(name, *parts):
        out[name] = hashlib.sha1(b"".join(np.ascontiguousarray(np.asarray(p, dtype=np.float64)).tobytes() for p in parts)).hexdigest()[:12]

    def problem(n, d, noise=1.0e-3, seed=None):
        X, y = synthetic_problem(n, d, seed=17 + n if seed is None else seed)
        return X, y, ("Matern52", 0.25 * np.sqrt(d) * np.ones(1), 1.3, noise, float(y.mean()))

    def engine(dtype, timed, two_level=False, overlap=None):
        eng = HipGPEngine(dtype, precision_check=False)
        eng.set_timing(timed)
        if two_level:
            eng.set_fit_single_level_max(0)
        if overlap is not None:
            eng._check(eng._lib.gpso_set_option(eng._h, L.OPT_FIT_OVERLAP, overlap))
        return eng

    def state(eng, kinv):
        mats = [L.MAT_CHOL, L.MAT_LINV] + ([L.MAT_KINV] if kinv else [])
        return [eng.last_count(2)] + [eng.get_matrix(m) for m in mats] + [eng.get_vector(L.VEC_ALPHA)]

    def fit_rows(tag, dtype, n, d, timed, noise=1.0e-3, **kw):
        X, y, th = problem(n, d, noise)
        for grad in (True, False):
            eng = engine(dtype, timed, **kw)
            eng.set_data(X, y)
            f, g = eng.fit_eval(*th, want_grad=grad)
            put(f"fit {tag} N={n} D={d} {dtype} grad={int(grad)} {'timed' if timed else 'untimed'}", f, g if grad else [], *state(eng, grad))
            eng.close()

    for timed in (True, False):
        t = "timed" if timed else "untimed"
        for dtype in ("float64", "mixed", "float32"):
            fit_rows("one-launch", dtype, 52, 2, timed)
            fit_rows("one-launch", dtype, 128, 3, timed)
            fit_rows("single-level", dtype, 300, 3, timed)
        for overlap in (0, 2, 3):
            fit_rows(f"two-level overlap={overlap}", "float64", 700, 5, timed, two_level=True, overlap=overlap)
            fit_rows(f"two-level overlap={overlap}", "float64", 1100, 3, timed, two_level=True, overlap=overlap)
        for noise in (1.0e-3, 1.0e-2):
            fit_rows(f"two-level planes noise={noise:g}", "float32", 900, 6, timed, noise=noise, two_level=True)
        for n, d in ((52, 2), (300, 3)):
            X, y, th = problem(n, d)
            for dtype in ("float64", "mixed"):
                for first_a_plain_fit in (False, True) if dtype == "float64" else (False,):
                    eng = engine(dtype, timed)
                    eng.set_data(X, y)
                    if first_a_plain_fit:
                        eng.fit_eval(*th, want_grad=False)
                    loss, g, nlml = eng.fit_eval_loo(*th)
                    put(f"loo N={n} D={d} {dtype} behind_a_fit={int(first_a_plain_fit)} {t}", loss, g, nlml, *state(eng, True))
                    eng.close()
        X, y, th = problem(52, 2)
        eng = engine("float64", timed)
        eng.set_data(X, y)
        U = np.array([[0.3, 0.5, -6.0, 0.1], [0.1, 0.2, -5.0, 0.0], [0.3, -800.0, -6.0, 0.1], [-0.2, 0.4, -7.0, 0.3]])
        put(f"batch fit_eval_u_batch N=52 D=2 float64 {t}", *eng.fit_eval_u_batch("Matern52", U, 1, True))
        eng.close()
        for n0, k, d, dtype in ((297, 3, 3, "float64"), (2041, 7, 12, "float32"), (100, 3, 3, "float64")):
            X, y, th = problem(n0 + k, d)
            eng = engine(dtype, timed)
            eng.set_data(X[:n0], y[:n0])
            eng.fit_eval(*th, want_grad=False)
            f, in_place = eng.append(X[n0:], y[n0:])
            put(f"append N={n0}+{k} D={d} {dtype} in_place={int(in_place)} {t}", f, *state(eng, False))
            eng.close()
        # the in-place refusal of tests/test_gpu_append.py: a NaN input, the block is not positive definite
        X, y, th = problem(300, 3, noise=1.0e-6, seed=11)
        eng = engine("float64", timed)
        eng.set_data(X, y)
        eng.fit_eval(*th, want_grad=False)
        try:
            eng.append(np.vstack([X[:2], np.full((1, 3), np.nan)]), np.zeros(3))
            refused = 0
        except np.linalg.LinAlgError:
            refused = 1
        put(f"append N=300+3 D=3 float64 refused={refused} then predict {t}", eng.n, *eng.predict(synthetic_leaves(400, 3)), *state(eng, False))
        eng.close()


def worker():
    sys.path.insert(0, ROOT)
    import numpy as np

    from pygpso_amd import HipGPEngine
    from tests.helpers import synthetic_leaves, synthetic_problem

    out = {}
    for flag, section in (("--theta", theta_section), ("--points", points_section), ("--fit", fit_section)):
        if flag in sys.argv:
            section(out)
            print("AB_BITS " + json.dumps(out), flush=True)
            return
    for n, d, m, kernel in SHAPES:
        X, y = synthetic_problem(n, d, seed=1)
        Xs = synthetic_leaves(m, d, seed=3)
        for dtype, math, gen, contraction in CASES:
            kw = {}
            if math:
                kw["predict_math"] = math
            if gen:
                kw["generation"] = gen
            eng = HipGPEngine(dtype, precision_check=False, **kw)
            if contraction and hasattr(eng, "set_contraction"):
                eng.set_contraction(contraction)
            eng.set_data(X, y)
            eng.fit_eval(kernel, 0.3 * np.sqrt(d) * np.ones(1), 1.7, 1e-3, float(y.mean()), want_grad=False)
            mean, var = eng.predict(Xs)
            idx, mu, vv, ucb = eng.best_ucb(Xs, 2.0)
            h = hashlib.sha1(mean.tobytes() + var.tobytes() + np.asarray(idx).tobytes() + np.asarray(ucb).tobytes()).hexdigest()[:12]
            out[f"N{n} D{d} {kernel} | {dtype} {math} gen={gen} contraction={contraction}"] = h
            eng.close()
    # gpso_append (round 6: the same arithmetic in three launches instead of six + two copies): fit N - k, append k, hash what
    # the extended posterior is -- NLML, the factor's new rows, alpha, predictions
    from pygpso_amd import _lib as L

    for n, d, k, dtype in [(2048, 12, 7, "float32"), (2048, 12, 1, "mixed"), (1000, 5, 20, "float64"), (4096, 6, 40, "float32"),
                           (4096, 6, 64, "float64"), (300, 3, 3, "float64"), (8192, 20, 7, "float32")]:
        X, y = synthetic_problem(n, d, seed=2)
        Xs = synthetic_leaves(1500, d, seed=3)
        eng = HipGPEngine(dtype, precision_check=False)
        eng.set_data(X[:n - k], y[:n - k])
        eng.fit_eval("Matern52", 0.25 * np.sqrt(d) * np.ones(1), 1.0, 1e-3, float(y.mean()), want_grad=False)
        eng.predict(Xs[:256])
        f, in_place = eng.append(X[n - k:], y[n - k:])
        mean, var = eng.predict(Xs)
        h = hashlib.sha1(np.float64(f).tobytes() + mean.tobytes() + var.tobytes() + eng.get_vector(L.VEC_ALPHA).tobytes()
                         + (eng.get_matrix(L.MAT_LINV)[n - k:].tobytes() if n <= 4096 else b"")).hexdigest()[:12]
        out[f"append N{n - k}+{k} D{d} {dtype} in_place={in_place}"] = h
        eng.close()
    theta_section(out)
    print("AB_BITS " + json.dumps(out), flush=True)


def main():
    if "--worker" in sys.argv:
        return worker()
    libs = [a for a in sys.argv[1:] if not a.startswith("--")]
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    res = []
    for lib in libs:
        env = dict(os.environ, GPSO_HIP_LIB=os.path.abspath(lib), GPSO_HIP_LIB_OLDER="1")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + flags, env=env, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("AB_BITS ")]
        if not line:
            print(lib, "FAILED", p.stderr[-1500:])
            return 1
        res.append(json.loads(line[0][8:]))
    ndiff = 0
    for k in res[0]:
        hs = [r.get(k) for r in res]
        same = all(h == hs[0] for h in hs)
        ndiff += not same
        print(("same  " if same else "DIFF  ") + " ".join(hs) + "  " + k)
    print(f"{ndiff} differing rows of {len(res[0])}")
    if "--fit" in flags:  # timed against untimed, in every library
        pairs = [(k, k[:-len(" timed")] + " untimed") for k in res[0] if k.endswith(" timed")]
        bad = [(lib, a) for lib, r in zip(libs, res) for a, b in pairs if r.get(a) != r.get(b)]
        for lib, a in bad:
            print("TIMED != UNTIMED  " + lib + "  " + a)
        print(f"{len(bad)} of {len(pairs) * len(res)} timed rows differ from their untimed row")
    return 0


if __name__ == "__main__":
    sys.exit(main())
