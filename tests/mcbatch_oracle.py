"""Independent numpy oracle of the Monte-Carlo batch acquisition over path draws (``gpso_paths_best_batch`` /
``gpso_paths_batch_host``): sequential greedy selection of the sample-average qEI / qPI over a given
value matrix.  Plain ``np.maximum`` / ``mean`` / ``argmax`` on whole arrays; it shares no code with csrc/mcbatch.hpp and
sums in numpy's order, not the header's.

qEI is written from its definition, not from the header's bookkeeping of bars and margins: with imp[s, j] = max(V[s, j] -
t0[s] - xi, 0) the improvement of row j in draw s and held[s] the largest improvement among the picks (and pending points) so
far, the gain of row j is mean_s max(imp[s, j] - held[s], 0) -- what the batch's value mean_s max_picks imp grows by.
"""
import numpy as np

QEI, QPI = "qei", "qpi"


def _argmax(gain, live):
    """The first maximum among the live rows, a NaN beating every number (np.argmax's rule); -1 with no live row."""
    if not live.any():
        return -1
    g = np.where(live, gain, -np.inf)
    nan = np.isnan(g) & live
    if nan.any():
        return int(np.argmax(nan))
    best = g.max()
    return int(np.argmax(live & (g == best)))


def greedy(V, m, q, kind, bars, xi=0.0):
    """V [S, m + b]: the candidates' columns, then the pending ones; bars [S] (or a scalar).  Returns (idx, gain,
    batch_value, gain0, margins): the picks, the gain each was ranked by, the running sum, every row's round-0 gain, and per
    round that ranked rows the gap between its two highest gains among the live rows (inf with one live row)."""
    V = np.asarray(V, dtype=np.float64)
    s = V.shape[0]
    cand, pend = V[:, :m], V[:, m:]
    bars = np.broadcast_to(np.asarray(bars, dtype=np.float64), (s,)).copy()
    improved = np.zeros(s, dtype=bool)
    held = np.zeros(s)
    with np.errstate(invalid="ignore"):
        imp = np.maximum(cand - bars[:, None] - xi, 0.0)
        if pend.shape[1]:
            held = np.fmax(held, np.max(np.nan_to_num(np.maximum(pend - bars[:, None] - xi, 0.0), nan=0.0), axis=1))
            improved = (pend > (bars + xi)[:, None]).any(axis=1)
    live = np.ones(m, dtype=bool)
    idx, gains, values, margins = [], [], [], []
    gain0 = None
    for t in range(q):
        with np.errstate(invalid="ignore"):
            if kind == QEI:
                gain = np.mean(np.maximum(imp - held[:, None], 0.0), axis=0)
            else:
                hits = (cand > (bars + xi)[:, None]) & ~improved[:, None]
                gain = np.where(np.isnan(cand).any(axis=0), np.nan, hits.sum(axis=0) / s)
        if t == 0:
            gain0 = gain.copy()
        p = _argmax(gain, live)
        if p < 0:
            break
        top = np.sort(gain[live])[::-1]
        margins.append(float(top[0] - top[1]) if top.size > 1 and np.isfinite(top[:2]).all() else np.inf)
        g = gain[p]
        if t > 0 and not np.isnan(g) and not g > 0.0:
            margins.pop()
            break
        idx.append(p)
        gains.append(g)
        values.append(g if t == 0 else values[-1] + g)
        live[p] = False
        if np.isnan(g):
            break
        if kind == QEI:
            held = np.fmax(held, imp[:, p])
        else:
            improved |= cand[:, p] > bars + xi
    return (np.array(idx, dtype=np.int64), np.array(gains, dtype=np.float64), np.array(values, dtype=np.float64), gain0,
            np.array(margins, dtype=np.float64))


def batch_value_qei(V, m, picks, bars0, xi=0.0):
    """(1/S) sum_s max_t max(V[s, p_t] - bars0[s] - xi, 0): the sample-average value of the batch ``picks`` -- over what the
    pending columns V[:, m:] already hold."""
    V = np.asarray(V, dtype=np.float64)
    bars0 = np.broadcast_to(np.asarray(bars0, dtype=np.float64), (V.shape[0],))
    imp = np.maximum(V - bars0[:, None] - xi, 0.0)
    held = imp[:, m:].max(axis=1) if V.shape[1] > m else np.zeros(V.shape[0])
    return float(np.mean(np.maximum(np.max(imp[:, picks], axis=1) - held, 0.0)))


def decided_by(V, m, q, kind, bars, xi=0.0):
    """How far the rounds of ``greedy`` on V are from going another way under a perturbation of V: the smallest of (a) half
    the gap between the two highest gains of every round that reports a pick, (b) for QEI the distance by which every live
    row misses a positive term in the round that ends the batch, and (c) for QPI the distance of every entry of V from its
    draw's threshold (inside it the counts are exact).  A perturbation of every entry by less than a quarter of this leaves
    the picks and -- for QPI -- the gains as they are."""
    V = np.asarray(V, dtype=np.float64)
    s = V.shape[0]
    bars = np.broadcast_to(np.asarray(bars, dtype=np.float64), (s,))
    idx, gains, _, _, margins = greedy(V, m, q, kind, bars, xi)
    least = float(np.min(margins)) / 2.0 if margins.size else np.inf
    if kind == QPI:
        return float(np.min(np.abs(V - (bars + xi)[:, None])))  # (gains are exact counts: a tie goes to the first row on both sides)
    if idx.size < min(q, m) and not np.isnan(gains[-1]):  # the batch ended on a round without a positive gain
        raw = V - bars[:, None] - xi
        held = np.maximum(np.max(np.maximum(raw[:, list(idx) + list(range(m, V.shape[1]))], 0.0), axis=1), 0.0)
        live = np.setdiff1d(np.arange(m), idx)
        if live.size:
            least = min(least, float(np.min(held[:, None] - raw[:, live])))
    return least
