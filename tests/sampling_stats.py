"""Exact probability laws of the samplers and the statistics that hold their output to them (numpy and ``math`` only).

Laws
  uniform without replacement   inclusion M/N, pair co-inclusion M(M-1)/(N(N-1))
  with replacement              every draw uniform over the N slots, draws independent
  weighted without replacement  A-Res = successive draws proportional to the remaining weight: ``weighted_inclusion``
  temporal                      the law above over the qualifying slots (weight 1 when unbiased); a row with q <= M qualifying
                                slots returns all q

Statistics: every function returns ``(statistic, p_value)``; a p-value that carries a Bonferroni factor is already
multiplied by it.  One level for every test: ``ALPHA``.  The bounds are quantiles of the exact law (chi-square through the
regularised incomplete gamma function, normal through ``erfc``), never figures taken from a sampler."""
import itertools
import math

import numpy as np

ALPHA = 1e-6
GOLDEN = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1


# ---- tails ------------------------------------------------------------------------------------------------------------------

def _gamma_p_series(a, x):
    """P(a, x) by the power series (x < a + 1)."""
    term = 1.0 / a
    total = term
    for n in range(1, 200000):
        term *= x / (a + n)
        total += term
        if abs(term) < abs(total) * 1e-17:
            break
    return total * math.exp(-x + a * math.log(x) - math.lgamma(a))


def _gamma_q_fraction(a, x):
    """Q(a, x) by the continued fraction, modified Lentz (x >= a + 1)."""
    tiny = 1e-300
    b = x + 1.0 - a
    c = 1.0 / tiny
    d = 1.0 / b
    h = d
    for n in range(1, 200000):
        an = -n * (n - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return h * math.exp(-x + a * math.log(x) - math.lgamma(a))


def chi2_sf(x, dof):
    """P(chi-square with ``dof`` degrees of freedom > x) = Q(dof / 2, x / 2)."""
    a, x = 0.5 * dof, 0.5 * float(x)
    if x <= 0.0:
        return 1.0
    if x < a + 1.0:
        return max(0.0, 1.0 - _gamma_p_series(a, x))
    return _gamma_q_fraction(a, x)


def norm_sf(z):
    """P(standard normal > z)."""
    return 0.5 * math.erfc(z / math.sqrt(2.0))


def _two_sided(z, k=1):
    return min(1.0, 2.0 * k * norm_sf(abs(z)))


# ---- exact laws -------------------------------------------------------------------------------------------------------------

def weighted_inclusion(w, M):
    """Inclusion probability of every slot when M slots are drawn one after the other, each with probability proportional to
    its weight among the slots that remain (the law of A-Res), by enumeration of the ordered M-tuples over the
    positive-weight slots.  Fewer than M + 1 positive slots: each of them has probability 1 and the zero-weight slots are
    left at 0 (which of them fill a row up is not part of the law).  M = 1 is w / sum(w) for any N."""
    w = np.asarray(w, dtype=np.float64)
    pos = np.nonzero(w > 0)[0]
    p = np.zeros(w.shape[0])
    k = pos.shape[0]
    if k <= M:
        p[pos] = 1.0
        return p
    wp = w[pos]
    if M == 1:
        p[pos] = wp / wp.sum()
        return p
    assert math.perm(k, M) <= 100000, "enumeration is meant for N <= 12, M <= 5"
    tup = np.array(list(itertools.permutations(range(k), M)), dtype=np.int64)          # [T, M]
    wt = wp[tup]
    before = np.cumsum(wt, axis=1) - wt                                                  # weight already drawn
    prob = np.prod(wt / (wp.sum() - before), axis=1)
    inc = np.zeros(k)
    for t in range(M):
        inc += np.bincount(tup[:, t], weights=prob, minlength=k)
    p[pos] = inc
    return p


def hop_seed(random_state, hop):
    """The walk's seed schedule, restated: hop k of a call with ``random_state`` draws with random_state + k * golden."""
    return (int(random_state) + hop * GOLDEN) & MASK64


# ---- from sampler output to matrices ----------------------------------------------------------------------------------------

def inclusion_matrix(row, slot, n, N):
    """0/1 matrix [n, N]: entry (i, j) is set when pick list row i holds slot j.  A slot listed twice in a row is an error."""
    cell = np.asarray(row, dtype=np.int64) * N + np.asarray(slot, dtype=np.int64)
    assert cell.size == 0 or (0 <= cell.min() and cell.max() < n * N)
    a = np.bincount(cell, minlength=n * N)
    assert a.max(initial=0) <= 1, "a slot picked twice by a sampler without replacement"
    return a.astype(np.uint8).reshape(n, N)


# ---- statistics -------------------------------------------------------------------------------------------------------------

def folds(N, bins=64):
    """The two foldings of N slots into ``bins`` bins: lane-patterned (j mod bins) and range-patterned (floor(bins j / N))."""
    j = np.arange(N)
    return {"mod": j % bins, "range": (bins * j) // N}


def incl(h, n, M, N):
    """Equal inclusion probabilities M/N, without replacement, n rows; h = hits per slot.  The hits have variance
    n p (1 - p) and covariance -n p (1 - p) / (N - 1), so sum (h - n p)^2 / (n p (1 - p)) * (N - 1) / N is chi-square(N - 1).
    N > 256: the bins of each folding instead (bin of s slots: variance s times, same covariance structure, chi-square(63));
    returns the smaller p-value of the two, doubled."""
    h = np.asarray(h, dtype=np.float64)
    assert h.shape[0] == N and 0 < M < N
    p = M / N
    var = n * p * (1.0 - p) * N / (N - 1.0)
    if N <= 256:
        x = float(((h - n * p) ** 2).sum() / var)
        return x, chi2_sf(x, N - 1)
    out = []
    for bins in folds(N).values():
        s = np.bincount(bins, minlength=64).astype(np.float64)
        hb = np.bincount(bins, weights=h, minlength=64)
        x = float(((hb - s * n * p) ** 2 / (var * s)).sum())
        out.append((x, chi2_sf(x, 63)))
    x, pv = min(out, key=lambda v: v[1])
    return x, min(1.0, 2.0 * pv)


def multinomial(h, expected, fold=False):
    """Pearson's statistic of counts against expectations of the same total (independent draws), chi-square(k - 1).
    ``fold``: more than 256 cells are folded into 64 bins both ways first, 65 to 256 cells into 16 bins (Pearson's
    approximation wants more than a handful of expected hits per cell, which single slots of such rows do not get from 8192
    draws), expectations summed per bin; the smaller p-value of the two foldings, doubled."""
    h, e = np.asarray(h, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    assert h.shape == e.shape and abs(h.sum() - e.sum()) <= 1e-6 * e.sum()
    if not fold or h.shape[0] <= 64:
        assert np.all(e > 0)
        x = float(((h - e) ** 2 / e).sum())
        return x, chi2_sf(x, h.shape[0] - 1)
    bins = 64 if h.shape[0] > 256 else 16
    out = []
    for fold_of in folds(h.shape[0], bins).values():
        hb, eb = np.bincount(fold_of, weights=h, minlength=bins), np.bincount(fold_of, weights=e, minlength=bins)
        x = float(((hb - eb) ** 2 / eb).sum())
        out.append((x, chi2_sf(x, bins - 1)))
    x, pv = min(out, key=lambda v: v[1])
    return x, min(1.0, 2.0 * pv)


def incl_unequal(h, n, p):
    """Unequal inclusion probabilities p over n rows: per-slot z with the binomial variance n p (1 - p), max |z| against the
    two-sided Bonferroni bound over the slots with 0 < p < 1.  A slot of probability 0 that was hit, or one of probability 1
    that was missed, gives p-value 0."""
    h, p = np.asarray(h, dtype=np.float64), np.asarray(p, dtype=np.float64)
    sure = (p <= 0) | (p >= 1)
    if np.any(h[sure] != n * p[sure]):
        return math.inf, 0.0
    t = ~sure
    if not t.any():
        return 0.0, 1.0
    z = (h[t] - n * p[t]) / np.sqrt(n * p[t] * (1.0 - p[t]))
    zmax = float(np.abs(z).max())
    return zmax, _two_sided(zmax, int(t.sum()))


def pair(a, M, N):
    """Pair co-inclusion of a uniform sampler without replacement (N <= 64): a is the [n, N] inclusion matrix, every pair of
    slots is together in a row with probability M(M-1)/(N(N-1)); per-pair z with the binomial variance, Bonferroni over
    the N(N-1)/2 pairs."""
    assert N <= 64 and 1 < M < N
    n = a.shape[0]
    f = a.astype(np.float64)
    c = f.T @ f
    p2 = M * (M - 1.0) / (N * (N - 1.0))
    iu = np.triu_indices(N, 1)
    z = (c[iu] - n * p2) / math.sqrt(n * p2 * (1.0 - p2))
    zmax = float(np.abs(z).max())
    return zmax, _two_sided(zmax, N * (N - 1) // 2)


def overlap(a, b, M, N):
    """Independence of two pick lists row by row: a and b are inclusion matrices of equal shape whose rows hold M of N slots.
    The number of common slots of two independent rows, one of them uniform, is hypergeometric: mean M^2 / N, variance
    M (M/N) (1 - M/N) (N - M) / (N - 1).  Returns the standardised sum over the rows and its two-sided p-value."""
    assert a.shape == b.shape and a.shape[1] == N and 0 < M < N
    n = a.shape[0]
    common = float((a & b).sum(dtype=np.int64))
    p = M / N
    var = n * M * p * (1.0 - p) * (N - M) / (N - 1.0)
    z = (common - n * M * p) / math.sqrt(var)
    return z, _two_sided(z)


def overlap_shift(a, shift, M, N):
    """``overlap`` between rows i and i + shift of one matrix."""
    return overlap(a[:-shift], a[shift:], M, N)


def _table(x, y, N):
    h = np.bincount(np.asarray(x, dtype=np.int64).ravel() * N + np.asarray(y, dtype=np.int64).ravel(), minlength=N * N)
    x2 = multinomial(h, np.full(N * N, h.sum() / (N * N)))
    return x2


def serial(d, N):
    """Serial dependence of draws with replacement (N <= 16): d is the [n, M] matrix of drawn slots.  The N x N table of
    (draw t, draw t + 1) of a row and that of (row i, row i + 1) at equal t, each as chi-square(N^2 - 1).  Pairs that share a
    draw are not independent of each other, so each table is built twice, from the pairs that start at an even and at an
    odd position: four tables of disjoint pairs, each an exact multinomial sample.  Returns the largest statistic and the
    smallest p-value times four."""
    assert N <= 16 and d.ndim == 2
    out = []
    for par in (0, 1):
        if d.shape[1] >= par + 2:
            out.append(_table(d[:, par:-1:2], d[:, par + 1::2], N))
        out.append(_table(d[par:-1:2], d[par + 1::2], N))
    x = max(v[0] for v in out)
    return x, min(1.0, len(out) * min(v[1] for v in out))


def describe(name, stat, pv):
    return f"{name}: statistic {stat:.4g}, p {pv:.3g}"


def size_class_weights(N):
    return (0.05 + 3.0 * np.random.default_rng(1000 + N).random(N)).astype(np.float32)


def accept(results, what):
    """Every statistic inside its bound; the message (and the captured output) lists them all."""
    lines = [describe(k, *v) for k, v in results.items()]
    print(f"STAT {what} | " + " | ".join(lines))
    bad = [k for k, v in results.items() if not v[1] >= ALPHA]
    assert not bad, (what, bad, lines)


def rejected(results):
    return [k for k, v in results.items() if v[1] < ALPHA]


# ---- the checks of one case, shared by the host and the GPU tests ----------------------------------------------------------

def uniform_checks(a, M, N, shifts=(1, 32, 64)):
    n = a.shape[0]
    assert np.all(a.sum(1) == M), "M distinct slots per row"
    out = {"incl": incl(a.sum(0), n, M, N)}
    if N <= 64:
        out["pair"] = pair(a, M, N)
    for s in shifts:
        out[f"overlap(i,i+{s})"] = overlap_shift(a, s, M, N)
    return out


def replace_checks(d, N):
    out = {"freq": multinomial(np.bincount(d.ravel(), minlength=N), np.full(N, d.size / N), fold=N > 256)}
    if N <= 16:
        out["serial"] = serial(d, N)
    return out


def temporal_checks(a, ok, M, w=None, law=True):
    """a: [n, N] inclusion matrix of the slots returned for n rows with the same qualifying slots ``ok`` (bool [N]).  No
    other slot is returned; q <= M qualifying slots are all returned; of q > M exactly M, with inclusion probability M/q
    or, with weights w, that of ``weighted_inclusion`` over the qualifying slots (``law=False``: the counts only)."""
    ok = np.asarray(ok, dtype=bool)
    n, q = a.shape[0], int(ok.sum())
    if a[:, ~ok].any():
        return {"only qualifying slots": (math.inf, 0.0)}
    if q <= M:
        return {"all q returned": (0.0, 1.0) if a[:, ok].all() else (math.inf, 0.0)}
    if not np.all(a.sum(1) == M):
        return {"M slots per row": (math.inf, 0.0)}
    if not law:
        return {"M qualifying slots per row": (0.0, 1.0)}
    if w is None:
        return {"incl": incl(a[:, ok].sum(0), n, M, q)}
    return {"incl": incl_unequal(a.sum(0), n, weighted_inclusion(np.where(ok, w, 0.0), M))}
