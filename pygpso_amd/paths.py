"""
The random inputs of pathwise posterior draws (``gpso_paths_draw``): random Fourier features of the
four stationary kernels (Rahimi & Recht 2007) for the prior part of Matheron's rule (Wilson et al. 2020).  Everything is
drawn on the host, so a seed reproduces a path set; there is no generator on the device.

A feature is  phi_j(x) = sqrt(2 variance / F) cos(omega_j . (x / l) + b_j)  with omega_j from the kernel's spectral density
in SCALED coordinates and b_j uniform on [0, 2 pi):  E[phi(x) . phi(x')] = k(x, x'), the error falling as 1 / sqrt(F).
"""
import numpy as np

# Matern-nu: the spectral density is a multivariate Student-t with 2 nu degrees of freedom
MATERN_NU = {"Matern12": 0.5, "Matern32": 1.5, "Matern52": 2.5}
KERNEL_NAMES = ("Matern52", "Matern32", "Matern12", "SquaredExponential")


def _generator(rng):
    """A seed or a ``numpy.random.Generator`` (None: a fresh generator) -- ``model._standard_normals``' convention."""
    return rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)


def spectral_frequencies(kernel, n_features, d, rng=None):
    """``n_features`` frequencies [F, D] of ``kernel`` (its GPflow class name) in scaled coordinates x / l: standard normal
    z for the squared exponential; z sqrt(2 nu / g), g ~ chi^2(2 nu) -- one g per frequency -- for the Matern-nu."""
    f, d = int(n_features), int(d)
    if f < 1 or d < 1:
        raise ValueError(f"n_features={n_features}, d={d}: at least one of each")
    if kernel not in KERNEL_NAMES:
        raise ValueError(f"unknown kernel {kernel!r}: one of {KERNEL_NAMES}")
    gen = _generator(rng)
    z = gen.standard_normal((f, d))
    if kernel == "SquaredExponential":
        return z
    nu = MATERN_NU[kernel]
    g = gen.chisquare(2.0 * nu, size=(f, 1))
    return z * np.sqrt(2.0 * nu / g)


def draw_path_inputs(kernel, n_paths, n_features, n, d, rng=None):
    """Everything ``HipGPEngine.paths_draw`` takes, from one generator in a fixed order: (omega [F, D], phase [F],
    w [S, F], eps [S, N])."""
    s = int(n_paths)
    if s < 1:
        raise ValueError(f"n_paths={n_paths}: at least one draw")
    gen = _generator(rng)
    omega = spectral_frequencies(kernel, n_features, d, gen)
    phase = gen.uniform(0.0, 2.0 * np.pi, size=int(n_features))
    w = gen.standard_normal((s, int(n_features)))
    eps = gen.standard_normal((s, int(n)))
    return omega, phase, w, eps

