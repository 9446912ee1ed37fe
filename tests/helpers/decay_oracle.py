"""NumPy restatement of the decay measurement, written from its statement: Schroeder integral, the two energy
thresholds, the first samples at or below them, the crossing-time estimate and the least-squares fit over [i_a, i_b).  ``dtype`` is
float64 or np.longdouble; the two threshold factors are formed once in double, as the library forms them, whatever ``dtype`` is.
The sums run in NumPy's own order (a backward cumulative sum, pairwise sums): only the device pins an order."""
import numpy as np


def family(L, rt, fs=8000, seed=7):
    """h[k] = g[k] 10^(-3 k / (fs rt)), g standard normal: a response that decays 60 dB in rt seconds"""
    g = np.random.default_rng(seed).standard_normal(L)
    return g * 10.0 ** (-3.0 * np.arange(L) / (fs * rt))


def factors(start_db=5.0, decay_db=20.0):
    return 10.0 ** (-float(start_db) / 10.0), 10.0 ** (-(float(start_db) + float(decay_db)) / 10.0)


def edc(h, dtype=np.float64):
    """E[n] = sum_{k >= n} h[k]^2"""
    q = np.asarray(h, dtype=np.float64).astype(dtype) ** 2
    return np.cumsum(q[::-1])[::-1]


def _first_at_or_below(E, theta):
    hit = np.nonzero(E <= theta)[0]
    return int(hit[0]) if hit.size else -1


def _margin(E, i, theta):
    """relative distance from the threshold of the nearer of E[i] and E[i - 1]"""
    near = [abs(E[i] - theta)] + ([abs(E[i - 1] - theta)] if i > 0 else [])
    return float(min(near) / theta)


def measure(h, fs, decay_db=20.0, start_db=5.0, dtype=np.float64):
    """{"E", "e0", "i_a", "i_b", "sum_d", "sum_nd", "rt60_cross", "rt60_fit", "margin", "window"} of one response; margin: the
    smallest relative distance of a crossing from its threshold (inf without a crossing)"""
    E = edc(h, dtype)
    e0 = E[0]
    fa, fb = factors(start_db, decay_db)
    out = {"E": E, "e0": e0, "i_a": -1, "i_b": -1, "sum_d": dtype(0), "sum_nd": dtype(0), "rt60_cross": np.nan, "rt60_fit": np.nan,
           "margin": np.inf, "window": 0}
    if not e0 > 0:
        return out
    theta_a, theta_b = e0 * dtype(fa), e0 * dtype(fb)
    i_a, i_b = _first_at_or_below(E, theta_a), _first_at_or_below(E, theta_b)
    out.update(i_a=i_a, i_b=i_b)
    out["margin"] = min([_margin(E, i, th) for i, th in ((i_a, theta_a), (i_b, theta_b)) if i >= 0] + [np.inf])
    in_window = (E > theta_b) & (E <= theta_a)
    n = np.nonzero(in_window)[0]
    D = dtype(10) * np.log10(E[n] / e0)
    out.update(sum_d=np.sum(D), sum_nd=np.sum(n.astype(dtype) * D), window=int(n.size))
    if i_b < 0:
        return out
    N = dtype(i_b - i_a)
    out["rt60_cross"] = float(dtype(60) / dtype(decay_db) * N / dtype(fs))
    if i_b - i_a >= 2:
        nbar = dtype(i_a + i_b - 1) / dtype(2)
        m = (out["sum_nd"] - nbar * out["sum_d"]) / (N * (N * N - dtype(1)) / dtype(12))
        out["rt60_fit"] = float(dtype(-60) / (m * dtype(fs)))
    return out
