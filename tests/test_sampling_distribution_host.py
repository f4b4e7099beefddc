"""CPU: the oracle's samplers against the exact probability law each is supposed to have (``sampling_stats.py``).

The other sampling tests pin the kernels to the oracle bit for bit; these pin the oracle to the law, so a defect that a
kernel and its restatement share does not pass.  Every input is fixed, every bound is the 1e-6 quantile of the exact law.

a. the helper against tabulated values, scipy where it is installed, and a Monte Carlo of successive weighted draws;
b. deliberately wrong samplers, each of which the statistics must reject at the shapes and row counts used in c;
c. the oracle: uniform, with replacement, weighted (enumeration, M = 1 per size class, scaling), the seed schedule of the
   walk, the temporal hop restated with effective weights;
d. the schedule never produces two seeds 2^63 apart (DESIGN.md, next to assumption A1)."""
import numpy as np
import pytest

import sampling_stats as S
from sampling_stats import (ALPHA, accept, rejected, replace_checks, size_class_weights, temporal_checks, uniform_checks)

N_ROWS = 8192
N_ROWS_WEIGHTED = 16384
SEED_UNIFORM, SEED_REPLACE, SEED_WEIGHTED, SEED_SCHEDULE = 777, 4242, 99, 1000

UNIFORM_CASES = [(7, 5, N_ROWS), (11, 10, N_ROWS), (40, 10, N_ROWS), (36, 15, N_ROWS), (26, 25, N_ROWS), (100, 25, N_ROWS),
                 (33, 32, N_ROWS), (64, 5, N_ROWS), (200, 40, N_ROWS), (600, 200, N_ROWS), (3000, 1100, 2048)]
REPLACE_CASES = [(3, 25), (7, 5), (16, 10), (40, 10), (1000, 3)]
W_1_TO_8 = np.arange(1, 9, dtype=np.float32)
W_10_AND_1 = np.array([10.0] * 5 + [1.0] * 7, dtype=np.float32)
W_NINE = np.array([0.05, 3, 0.5, 0.5, 1, 1, 2, 0.01, 0.2], dtype=np.float32)
W_MASK_5 = np.array([0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0], dtype=np.float32)
W_MASK_2 = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0], dtype=np.float32)
WEIGHTED_CASES = {"1..8": (W_1_TO_8, 3), "10x5+1x7": (W_10_AND_1, 5), "nine": (W_NINE, 4), "mask5": (W_MASK_5, 3),
                  "1..8 f64": (W_1_TO_8.astype(np.float64), 3), "nine f64": (W_NINE.astype(np.float64), 4)}
SIZE_CLASS_DEGREES = [17, 33, 65, 129, 257, 513, 1025]          # one row per candidate-list class of wg_common.hpp
SCHEDULE_SHAPES = [(40, 10), (64, 5), (100, 25), (33, 32)]
TEMPORAL_N, TEMPORAL_M, TEMPORAL_Q = 24, 5, [0, 1, 4, 5, 6, 12, 24]


# ---- a. the helper against known values ---------------------------------------------------------------------------------------

CHI2_TABLE = [  # (x, dof, upper tail)
    (0.4549364231195724, 1, 0.5), (3.841458820694124, 1, 0.05), (6.634896601021217, 1, 0.01), (32.84125336123679, 1, 1e-8),
    (1.386294361119891, 2, 0.5), (27.631021115928547, 2, 1e-6), (13.361566136511728, 8, 0.1), (31.82762800126232, 8, 1e-4),
    (38.33539737953598, 39, 0.5), (96.12556491301818, 39, 1e-6), (62.33460207230615, 63, 0.5), (131.36970205168686, 63, 1e-6),
    (147.46261034127772, 63, 1e-8), (4094.333352631608, 4095, 0.5), (4308.467865579965, 4095, 0.01),
    (4539.664051381019, 4095, 1e-6), (4623.373056164858, 4095, 1e-8)]
NORM_TABLE = [(0.0, 0.5), (1.2815515655446004, 0.1), (1.959963984540054, 0.025), (2.3263478740408408, 0.01),
              (3.7190164854556804, 1e-4), (4.753424308822899, 1e-6), (5.612001244174789, 1e-8)]


def test_tails_at_tabulated_points():
    for x, dof, p in CHI2_TABLE:
        assert abs(S.chi2_sf(x, dof) / p - 1.0) < 1e-9, (x, dof, p, S.chi2_sf(x, dof))
    for dof in (1, 2, 8, 63):                                                 # chi-square(2) is exp(-x/2) exactly
        assert S.chi2_sf(0.0, dof) == 1.0
    assert abs(S.chi2_sf(20.0, 2) / np.exp(-10.0) - 1.0) < 1e-12
    for z, p in NORM_TABLE:
        assert abs(S.norm_sf(z) / p - 1.0) < 1e-9, (z, p)
        assert abs(S.norm_sf(-z) - (1.0 - p)) < 1e-12
    try:
        from scipy.stats import chi2
    except ImportError:
        return
    rng = np.random.default_rng(0)
    for _ in range(200):
        dof = int(rng.integers(1, 4200))
        x = dof + rng.uniform(-3.0, 7.0) * np.sqrt(2.0 * dof)
        if x > 0:
            want = chi2.sf(x, dof)
            assert abs(S.chi2_sf(x, dof) - want) <= 1e-9 * want, (x, dof, want)


def test_weighted_enumeration_against_successive_draws():
    """4e6 rows of three successive draws proportional to the remaining weight, in float64, within 5 standard errors."""
    w, M, n = np.arange(1.0, 9.0), 3, 4_000_000
    p = S.weighted_inclusion(w, M)
    assert abs(p.sum() - M) < 1e-12
    rng = np.random.default_rng(7)
    left = np.tile(w, (n, 1))
    hits = np.zeros(8)
    for _ in range(M):
        cum = np.cumsum(left, axis=1)
        j = (cum <= (rng.random(n) * cum[:, -1])[:, None]).sum(1)
        hits += np.bincount(j, minlength=8)
        left[np.arange(n), j] = 0.0
    se = np.sqrt(p * (1.0 - p) / n)
    assert np.all(np.abs(hits / n - p) < 5.0 * se), (hits / n, p)
    # closed forms: M = 1; equal weights; a mask
    assert np.allclose(S.weighted_inclusion(w, 1), w / w.sum(), rtol=0, atol=1e-15)
    assert np.allclose(S.weighted_inclusion(np.ones(12), 5), 5 / 12, rtol=0, atol=1e-12)
    assert np.allclose(S.weighted_inclusion(W_MASK_5, 3), 0.6 * W_MASK_5.astype(np.float64), rtol=0, atol=1e-12)
    assert np.array_equal(S.weighted_inclusion(W_MASK_2, 3), W_MASK_2)


# ---- b. the statistics must have teeth ----------------------------------------------------------------------------------------

def np_fisher_yates(rng, n, N, M, wrong=False):
    """Partial Fisher-Yates over n rows; ``wrong``: the t-th draw is taken modulo N - t - 1, the last position unreachable."""
    perm = np.tile(np.arange(N), (n, 1))
    rows = np.arange(n)
    for t in range(M):
        j = t + rng.integers(0, 1 << 31, n) % (N - t - (1 if wrong else 0))
        perm[rows, t], perm[rows, j] = perm[rows, j], perm[rows, t]
    return S.inclusion_matrix(np.repeat(rows, M), perm[:, :M].ravel(), n, N)


def np_top_m(rng, n, N, M, w=None, coarse=False):
    """Top-M of per-slot keys u^(1/w); ``coarse``: keys rounded to 3 bits, ties towards the lowest index."""
    u = rng.random((n, N))
    key = np.floor(u * 8.0) if coarse else (np.log(u) / (1.0 if w is None else np.asarray(w, dtype=np.float64)))
    picks = np.argsort(-key, axis=1, kind="stable")[:, :M]
    return S.inclusion_matrix(np.repeat(np.arange(n), M), picks.ravel(), n, N)


def np_replace(rng, n, N, M, sticky=0.0):
    d = rng.integers(0, N, (n, M))
    for t in range(M - 1):
        stick = rng.random(n) < sticky
        d[:, t + 1] = np.where(stick, d[:, t], d[:, t + 1])
    return d


def np_temporal(rng, n, N, M, q, strict=False):
    """Uniform over the slots whose time (= slot index) passes the comparison against q - 1; ``strict``: <= read as <."""
    ok = np.arange(N) < (q - 1 if strict else q)
    key = np.where(ok, rng.random((n, N)), -1.0)
    order = np.argsort(-key, axis=1)[:, :M]
    keep = ok[order]
    return S.inclusion_matrix(np.repeat(np.arange(n), M)[keep.ravel()], order[keep], n, N)


def test_correct_numpy_samplers_are_accepted():
    """The controls: the same code as the mutants with the defect switched off stays inside every bound."""
    rng = np.random.default_rng(100)
    accept(uniform_checks(np_fisher_yates(rng, N_ROWS, 40, 10), 10, 40), "control fisher-yates (40,10)")
    accept(uniform_checks(np_top_m(rng, N_ROWS, 40, 10), 10, 40), "control top-M (40,10)")
    a = np_top_m(rng, N_ROWS_WEIGHTED, 8, 3, W_1_TO_8)
    accept({"incl": S.incl_unequal(a.sum(0), N_ROWS_WEIGHTED, S.weighted_inclusion(W_1_TO_8, 3))}, "control weighted 1..8")
    for N, M in ((7, 5), (16, 10), (3, 25)):
        accept(replace_checks(np_replace(rng, N_ROWS, N, M), N), f"control with replacement ({N},{M})")
    for q in TEMPORAL_Q:
        a = np_temporal(rng, N_ROWS, TEMPORAL_N, TEMPORAL_M, q)
        accept(temporal_checks(a, np.arange(TEMPORAL_N) < q, TEMPORAL_M), f"control temporal q={q}")


def test_mutant_fisher_yates_last_position_unreachable():
    for N, M in ((40, 10), (7, 5), (100, 25)):
        a = np_fisher_yates(np.random.default_rng(1), N_ROWS, N, M, wrong=True)
        res = uniform_checks(a, M, N)
        assert "incl" in rejected(res) and res["incl"][1] == 0.0, res


def test_mutant_coarse_keys_tie_to_low_index():
    for N, M in ((40, 10), (64, 5)):
        res = uniform_checks(np_top_m(np.random.default_rng(2), N_ROWS, N, M, coarse=True), M, N)
        assert "incl" in rejected(res), res


@pytest.mark.parametrize("name", ["1..8", "10x5+1x7", "nine"])
def test_mutant_weights_ignored_or_squared(name):
    w, M = WEIGHTED_CASES[name]
    p = S.weighted_inclusion(w, M)
    for wrong in (None, np.asarray(w, dtype=np.float64) ** 2):
        a = np_top_m(np.random.default_rng(3), N_ROWS_WEIGHTED, w.shape[0], M, wrong)
        assert S.incl_unequal(a.sum(0), N_ROWS_WEIGHTED, p)[1] < ALPHA


def test_mutant_neighbouring_rows_share_a_stream():
    for N, M in SCHEDULE_SHAPES:
        half = np_fisher_yates(np.random.default_rng(4), N_ROWS // 2, N, M)
        res = uniform_checks(np.repeat(half, 2, axis=0), M, N)
        assert "overlap(i,i+1)" in rejected(res), res


def test_mutant_window_of_neighbouring_slots():
    """M consecutive slots from a uniform start (cyclic): every slot has probability M/N; the pair law sees it at once."""
    for N, M in ((40, 10), (64, 5)):
        start = np.random.default_rng(9).integers(0, N, N_ROWS)
        slots = (start[:, None] + np.arange(M)[None, :]) % N
        res = uniform_checks(S.inclusion_matrix(np.repeat(np.arange(N_ROWS), M), slots.ravel(), N_ROWS, N), M, N)
        assert "pair" in rejected(res) and res["pair"][1] == 0.0, res


def test_mutant_next_batch_reuses_every_16th_draw():
    for N, M in SCHEDULE_SHAPES:
        rng = np.random.default_rng(5)
        a, b = np_fisher_yates(rng, N_ROWS, N, M), np_fisher_yates(rng, N_ROWS, N, M)
        assert S.overlap(a, b, M, N)[1] >= ALPHA
        b[::16] = a[::16]
        assert S.overlap(a, b, M, N)[1] < ALPHA, (N, M, S.overlap(a, b, M, N))


def test_mutant_sticky_draws_with_replacement():
    for N, M in ((3, 25), (7, 5), (16, 10)):
        res = replace_checks(np_replace(np.random.default_rng(6), N_ROWS, N, M, sticky=1.0 / 8.0), N)
        assert "serial" in rejected(res), res


def test_mutant_temporal_strict_comparison():
    for q in TEMPORAL_Q[1:]:
        a = np_temporal(np.random.default_rng(8), N_ROWS, TEMPORAL_N, TEMPORAL_M, q, strict=True)
        assert rejected(temporal_checks(a, np.arange(TEMPORAL_N) < q, TEMPORAL_M)), q


# ---- c. the oracle against the exact laws ---------------------------------------------------------------------------------------

def one_row(N):
    return np.array([0, N], np.int64), np.arange(N, dtype=np.int64)


def oracle_uniform(oracle_mod, N, M, n, rs):
    rp, col = one_row(N)
    off, dst, lid, gid = oracle_mod.unweighted_sample(rp, col, np.zeros(n, np.int64), M, rs)
    assert off[-1] == n * M
    return S.inclusion_matrix(lid, gid, n, N)


def oracle_weighted(oracle_mod, w, M, n, rs):
    rp, col = one_row(len(w))
    off, dst, lid, gid = oracle_mod.weighted_sample(rp, col, w, np.zeros(n, np.int64), M, rs)
    assert off[-1] == n * M
    return S.inclusion_matrix(lid, gid, n, len(w))


@pytest.mark.parametrize("N,M,n", UNIFORM_CASES)
def test_oracle_uniform_without_replacement(oracle_mod, N, M, n):
    accept(uniform_checks(oracle_uniform(oracle_mod, N, M, n, SEED_UNIFORM), M, N), f"oracle uniform ({N},{M}) n={n}")


@pytest.mark.parametrize("N,M", REPLACE_CASES)
def test_oracle_uniform_with_replacement(oracle_mod, N, M):
    rp, col = one_row(N)
    off, dst, lid, gid = oracle_mod.unweighted_sample_with_replacement(rp, col, np.zeros(N_ROWS, np.int64), M, SEED_REPLACE)
    assert np.array_equal(off, np.arange(N_ROWS + 1) * M) and np.array_equal(lid, np.repeat(np.arange(N_ROWS), M))
    accept(replace_checks(gid.reshape(N_ROWS, M), N), f"oracle with replacement ({N},{M})")


@pytest.mark.parametrize("name", sorted(WEIGHTED_CASES))
def test_oracle_weighted_against_enumeration(oracle_mod, name):
    w, M = WEIGHTED_CASES[name]
    a = oracle_weighted(oracle_mod, w, M, N_ROWS_WEIGHTED, SEED_WEIGHTED)
    assert np.all(a.sum(1) == M)
    accept({"incl": S.incl_unequal(a.sum(0), N_ROWS_WEIGHTED, S.weighted_inclusion(w, M))}, f"oracle weighted {name} M={M}")


def test_oracle_weighted_mask_with_fewer_positive_slots_than_picks(oracle_mod):
    a = oracle_weighted(oracle_mod, W_MASK_2, 3, N_ROWS_WEIGHTED, SEED_WEIGHTED)
    assert np.all(a.sum(1) == 3) and np.all(a[:, W_MASK_2 > 0] == 1)


@pytest.mark.parametrize("N,M", [(17, 10), (40, 10)])
def test_oracle_weighted_equal_weights(oracle_mod, N, M):
    a = oracle_weighted(oracle_mod, np.full(N, 0.7, np.float32), M, N_ROWS_WEIGHTED, SEED_WEIGHTED)
    res = uniform_checks(a, M, N)
    res["incl max|z|"] = S.incl_unequal(a.sum(0), N_ROWS_WEIGHTED, np.full(N, M / N))
    accept(res, f"oracle weighted equal ({N},{M})")


@pytest.mark.parametrize("N", SIZE_CLASS_DEGREES)
def test_oracle_weighted_single_pick_per_size_class(oracle_mod, N):
    w = size_class_weights(N)
    a = oracle_weighted(oracle_mod, w, 1, N_ROWS, SEED_WEIGHTED)
    p = w.astype(np.float64) / w.astype(np.float64).sum()
    accept({"freq": S.multinomial(a.sum(0), N_ROWS * p, fold=True)}, f"oracle weighted M=1 N={N}")


def test_oracle_weighted_scaling_leaves_picks_unchanged(oracle_mod):
    """1/w scales exactly by a power of two and the key product with it: the picks are bit-identical."""
    for w, M in ((W_NINE, 4), (W_1_TO_8, 3), (size_class_weights(129), 10), (size_class_weights(1025), 25)):
        rp, col = one_row(len(w))
        seeds = np.zeros(512, np.int64)
        want = oracle_mod.weighted_sample(rp, col, w, seeds, M, SEED_WEIGHTED)
        for scale in (2.0 ** 20, 2.0 ** -20):
            got = oracle_mod.weighted_sample(rp, col, (w * np.float32(scale)).astype(np.float32), seeds, M, SEED_WEIGHTED)
            assert all(np.array_equal(g, v) for g, v in zip(got, want)), (len(w), M, scale)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("N,M", SCHEDULE_SHAPES)
def test_oracle_seed_schedule_is_independent(oracle_mod, N, M, weighted):
    """Batch b draws with random_state + b, hop k with hop_seed(random_state, k): the samples of two seeds of the schedule,
    row by row (equal local index), are independent."""
    def draw(rs):
        if weighted:
            return oracle_weighted(oracle_mod, np.ones(N, np.float32), M, N_ROWS, rs)
        return oracle_uniform(oracle_mod, N, M, N_ROWS, rs)
    s = 12345 if (N, M, weighted) == (40, 10, False) else SEED_SCHEDULE
    pairs = {"s|s+1": (s, s + 1), "s|s+7": (s, s + 7), "s|hop1": (s, S.hop_seed(s, 1)),
             "hop1|hop2": (S.hop_seed(s, 1), S.hop_seed(s, 2))}
    cache = {}
    res = {}
    for name, (x, y) in pairs.items():
        for v in (x, y):
            if v not in cache:
                cache[v] = draw(v)
        res[f"overlap {name}"] = S.overlap(cache[x], cache[y], M, N)
    accept(res, f"oracle schedule {'weighted' if weighted else 'uniform'} ({N},{M})")


def oracle_temporal(oracle_mod, w, q, M, n, rs):
    """The temporal hop restated: effective weight 0 for a slot that does not qualify (slot time = slot index against a seed
    time of q - 1, monotonically_decreasing), the weighted sampler, then the drop of the zero-weight picks."""
    N = len(w)
    eff = np.where(np.arange(N) <= q - 1, w, 0).astype(np.float32)
    rp, col = one_row(N)
    off, dst, lid, gid = oracle_mod.weighted_sample(rp, col, eff, np.zeros(n, np.int64), M, rs)
    keep = eff[gid] > 0
    return S.inclusion_matrix(lid[keep], gid[keep], n, N)


@pytest.mark.parametrize("q", TEMPORAL_Q)
def test_oracle_temporal_hop(oracle_mod, q):
    a = oracle_temporal(oracle_mod, np.ones(TEMPORAL_N, np.float32), q, TEMPORAL_M, N_ROWS, SEED_WEIGHTED)
    accept(temporal_checks(a, np.arange(TEMPORAL_N) < q, TEMPORAL_M), f"oracle temporal N={TEMPORAL_N} M={TEMPORAL_M} q={q}")


def test_oracle_temporal_hop_biased(oracle_mod):
    N, M, q = 24, 3, 12
    w = size_class_weights(N)
    a = oracle_temporal(oracle_mod, w, q, M, N_ROWS_WEIGHTED, SEED_WEIGHTED)
    accept(temporal_checks(a, np.arange(N) < q, M, w), "oracle temporal biased N=24 q=12 M=3")


# ---- d. the schedule and the 2^63 finding -------------------------------------------------------------------------------------

def test_schedule_never_pairs_seeds_half_the_ring_apart():
    """Two random seeds that differ by exactly 2^63 give correlated picks (their generator states differ in the top bit
    only).  Batch b of hop k draws with random_state + b + k * golden: for G <= 4096 batches and <= 8 hops no two seeds of a
    call group are 2^63 apart, whatever random_state is."""
    from cugraph_pyg_amd.sampler.sampler import hop_seed
    assert all(hop_seed(rs, k) == S.hop_seed(rs, k) for rs in (0, 62, 2 ** 64 - 1) for k in range(8))
    assert S.GOLDEN % 2 == 1
    db = np.arange(-4095, 4096, dtype=np.int64).astype(np.uint64)
    for dk in range(-7, 8):
        diff = db + np.uint64((dk * S.GOLDEN) & S.MASK64)                 # (b - b') + (k - k') * golden modulo 2^64
        assert not np.any(diff == np.uint64(1 << 63)), dk
    seeds = {(S.hop_seed(5, k) + b) & S.MASK64 for k in range(8) for b in range(4096)}
    assert len(seeds) == 8 * 4096 and not any((v + (1 << 63)) & S.MASK64 in seeds for v in seeds)


def test_seeds_half_the_ring_apart_are_correlated(oracle_mod):
    """The finding itself, so that a change of generator that removes it is noticed: N = 3, one pick, seeds s and s + 2^63;
    the 3 x 3 table of the two picks is far from independent, while s and s + 1 are clean."""
    rp, col = one_row(3)
    seeds = np.zeros(N_ROWS_WEIGHTED, np.int64)

    def table(other):
        x = oracle_mod.unweighted_sample(rp, col, seeds, 1, SEED_UNIFORM)[3]
        y = oracle_mod.unweighted_sample(rp, col, seeds, 1, other)[3]
        h = np.bincount(x * 3 + y, minlength=9)
        return S.multinomial(h, np.full(9, h.sum() / 9.0))
    assert table(SEED_UNIFORM + 1)[1] >= ALPHA
    assert table(SEED_UNIFORM + (1 << 63))[1] < ALPHA
