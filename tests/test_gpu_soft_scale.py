"""Soft (likelihood) evidence at every weight scale (nip_amd/csrc/soft.hip
chain_soft_kernel): "scaling a step's vector by c adds log c to ll and moves no
row", for every finite non-negative vector with a positive entry.

Inputs: tests/soft_scale_util.py -- the builders of tests/test_gpu_soft.py (the
smallest shape that reaches each path of the kernel), B = 7, T = 24 and 37,
base weights 0.05 + U[0, 1), every step's vector of every soft column
multiplied by 2^k, one pattern of k per sequence (|k| up to 900), the grid once
more at 2^-530 in place of 2^-560 on the two-column models; and an edge batch:
a spread of 2^-600 inside a vector, vectors all denormal, vectors of DBL_MAX.
The oracle is soft_util.soft_smoother, which tests/test_soft_api.py pins on
these very inputs to a wide-exponent evaluation (rows 1e-14).

Expectations, the project's own: status 0 on every sequence, rows 1e-12
absolute, ll 1e-11 max(1, |ll|), a NaN an infinite error.  Under the
power-of-two patterns the rows are the unscaled run's, bit for bit, and
ll - K ln 2 is the unscaled ll (K the sum of the applied exponents) within
1e-11 max(1, |ll_0|) + 4 eps |ll|, the second term for representing
K ln 2 + ll_0 in one double.

Further: small_mass_util's rare steps through the soft entry (as hard columns,
as one-hot weights, mixed) against textbook_util.smoother; posterior rows with
exact zeros fed back as weights, also times 2^-700; and the unchanged
semantics -- bad weights, an all-zero vector, batch independence to the bit --
inside the scaled batches.

Before chain_soft_kernel took the scale out of each vector it formed e_t as
the plain product of the columns' sums, and 53 of the 246 cases here failed on
it (wrong numbers, no faults; one run on an MI355X; the figures are T = 24's,
T = 37 failed in the same sequences):

  test_scale_patterns, two soft columns (demo20-both), 2^-560: sequences 1, 2,
    3, 6 reported dead (status 1, ll = -DBL_MAX; fb rows 0.06 off, being zero);
    in sequence 3 the even steps' 2^1120 is inf and the filtered row of that
    step NaN.  At 2^-530: sequences 1, 2 rows 1.4e-4 off and ll 1e-8..3e-8
    relative off with status 0; 3 and 6 as before.  Four soft columns
    (five-children): sequences 1, 2, 3, 4, 6 dead (4 is +340 on four columns),
    filtered rows NaN in 3, 4, 6.  Patterns 4 and 5 passed on two columns, and
    every single-column model passed the patterns: one factor cannot leave
    fp64 at |k| <= 900.
  test_edge_batch, every model: the denormal vectors (sequences 3, 4) dead at
    16 states and above (rows 0.02..0.8 off); at 3 states (hmm3x20-long) alive
    with rows 2e-2 off, ll 4e-6..1e-5 relative off, status 0.  The DBL_MAX
    vectors (5, 6): the column's sum is inf -- dead with NaN filtered rows on
    hmm16, hmm16-proper, hmm3x20-long, both demo20 requests and factorial-yx;
    wide64 (8 weights) and five-children (2 weights) stayed finite and passed.
    The spread inside a vector (1, 2) passed everywhere.
  test_a_bad_weight_in_a_scaled_batch, test_an_all_zero_vector_in_a_scaled_batch,
    test_batch_independence_under_the_patterns: the filter cases of
    demo20-both (and five-children's independence case), by the NaN rows of
    the neighbouring sequence 3 alone.
  test_small_mass and test_rows_fed_back passed: hard columns and one-hot or
    posterior-row weights never leave the tables' own range.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import nip_amd

import small_mass_util as sm
import soft_scale_util as ssu
import soft_util as so
import test_gpu_soft as tg
import test_soft_api as tsa
from textbook_util import smoother
from viterbi_util import LN2

FB, FILTER = tg.FB, tg.FILTER
PTOL, LTOL = 1e-12, 1e-11
EPS = np.finfo(np.float64).eps
DBL_MAX = np.finfo(np.float64).max
B = ssu.B

_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def device(which, r, obs, liks):
    """numpy (rows, ll, status) of the request r; asserts the kernel."""
    return tg.run(which, r.m, obs if r.ov else None, r.ov, liks, r.sv, r.q)


def oracle(r, obs, liks):
    """(smoothed, filtered, ll, status) in the query's layout."""
    A, pi, Es = r.tables
    post, filt, ll, st = so._run(A, pi, Es, *ssu.oracle_args(r, obs, liks))
    return ssu.query_rows(r, post), ssu.query_rows(r, filt), ll, st


def errors(rows, ll, want_rows, want_ll):
    """Per sequence; a NaN counts as an infinite error."""
    perr = np.abs(rows - want_rows).reshape(rows.shape[0], -1).max(axis=1)
    lerr = np.abs(ll - want_ll) / np.maximum(1.0, np.abs(want_ll))
    return np.where(np.isnan(perr), np.inf, perr), np.where(np.isnan(lerr), np.inf, lerr)


def check(where, which, got, want):
    rows, ll, st = got
    want_rows = want[0] if which == FB else want[1]
    assert rows.shape == want_rows.shape, (rows.shape, want_rows.shape)
    assert np.all(want[3] == 0), "the oracle finds a sequence without mass"
    perr, lerr = errors(rows, ll, want_rows, want[2])
    print("%s: row error %s, ll error (relative) %s, status %s" % (
        where, " ".join("%.2g" % e for e in perr), " ".join("%.2g" % e for e in lerr), st.tolist()))
    bad = (perr > PTOL) | (lerr > LTOL) | (st != 0)
    assert not bad.any(), "%s: sequences %s: row error %.3g, ll error %.3g (relative), ll %s, status %s" % (
        where, np.nonzero(bad)[0].tolist(), perr.max(), lerr.max(), ll[bad][:3].tolist(), st[bad][:3].tolist())


def inputs(name, T):
    r = ssu.requests()[name]
    return r, ssu.hard_obs(r, T), memo(("base", name, T), lambda: ssu.base_weights(r, T))


def unscaled(name, T, which):
    r, obs, base = inputs(name, T)
    return memo(("unscaled", name, T, which), lambda: device(which, r, obs, base))


def scaled_inputs(name, T, big):
    r, obs, base = inputs(name, T)
    k = ssu.exponents(T, len(r.soft), big)
    return r, obs, ssu.scaled(base, k), k


# ---------------------------------------------------------------------------
# 1. the scale patterns

GRID = [(name, T, 560) for name in ssu.NAMES for T in ssu.TS] + \
       [(name, T, 530) for name in ssu.TWO_COLUMN for T in ssu.TS]


@pytest.mark.parametrize("which", [FB, FILTER])
@pytest.mark.parametrize("name,T,big", GRID, ids=["%s-T%d-%d" % g for g in GRID])
def test_scale_patterns(name, T, big, which):
    r, obs, liks, k = scaled_inputs(name, T, big)
    where = "%s %s T=%d 2^-%d" % (which, name, T, big)
    rows0, ll0, st0 = unscaled(name, T, which)
    check(where + " unscaled", which, (rows0, ll0, st0),
          memo(("oracle0", name, T), lambda: oracle(r, obs, inputs(name, T)[2])))
    rows, ll, st = device(which, r, obs, liks)
    check(where, which, (rows, ll, st), memo(("oracle", name, T, big), lambda: oracle(r, obs, liks)))
    # an exact scaling moves no bit of a row
    moved = [b for b in range(B) if not np.array_equal(rows[b], rows0[b])]
    assert not moved, "%s: rows differ from the unscaled run's in sequences %s" % (where, moved)
    # and adds K ln 2 to the ll
    K = k.sum(axis=(1, 2))
    err = np.abs(ll - K * LN2 - ll0)
    bound = LTOL * np.maximum(1.0, np.abs(ll0)) + 4 * EPS * np.abs(ll)
    print("%s: |ll - K ln 2 - ll_0| %s" % (where, " ".join("%.2g" % e for e in err)))
    assert np.all(err <= bound), (where, err.tolist(), bound.tolist())


@pytest.mark.parametrize("which", [FB, FILTER])
@pytest.mark.parametrize("T", ssu.TS)
@pytest.mark.parametrize("name", ssu.NAMES)
def test_edge_batch(name, T, which):
    """A spread inside the vector, denormal vectors, DBL_MAX vectors: against
    the oracle (no exact rescaling of the base weights, so no bit identity)."""
    r, obs, _ = inputs(name, T)
    liks = memo(("edge", name, T), lambda: ssu.edge_weights(r, T))
    check("%s %s T=%d edge batch" % (which, name, T), which, device(which, r, obs, liks),
          memo(("edge-oracle", name, T), lambda: oracle(r, obs, liks)))


# ---------------------------------------------------------------------------
# 2. small step masses through the soft entry

RARE = {
    "hmm16": lambda mu: sm.rare_hmm(16, 4, mu),
    "hmm20": lambda mu: sm.rare_hmm(20, 4, mu),
    "hmm40": lambda mu: sm.rare_hmm(40, 4, mu),
    "star17x4": lambda mu: sm.rare_star(17, sm.STAR_CARDS, sm.col_scale(mu, 4)),
}
RARE_GRID = [(mu, 24) for mu in sm.MUS] + [(1e-80, 37)]


def rare_reference(name, mu, T):
    """(case, obs, smoothed, filtered, ll, status 0) of textbook_util.smoother, once."""
    def make():
        c = RARE[name](mu)
        obs = sm.rare_obs(T, c.cards, B=B)
        post, filt, ll = smoother(*c.tables, c.cols(obs))
        assert np.isfinite(post).all() and np.isfinite(ll).all() and (ll > -DBL_MAX).all()
        return c, obs, post, filt, ll, np.zeros(B, np.int64)
    return memo(("rare", name, mu, T), make)


@pytest.mark.parametrize("which", [FB, FILTER])
@pytest.mark.parametrize("form", ["hard-columns", "one-hot-weights", "first-soft-rest-hard"])
@pytest.mark.parametrize("mu,T", RARE_GRID, ids=["%g-T%d" % g for g in RARE_GRID])
@pytest.mark.parametrize("name", list(RARE))
def test_small_mass(name, mu, T, form, which):
    c, obs, post, filt, ll, st = rare_reference(name, mu, T)
    nsoft = {"hard-columns": 0, "one-hot-weights": c.ncol, "first-soft-rest-hard": 1}[form]
    liks = []
    for j in range(nsoft):
        w = np.eye(c.cards[j])[np.maximum(obs[:, :, j], 0)]
        w[obs[:, :, j] < 0] = 1.0                            # missing: all ones
        liks.append(w)
    got = tg.run(which, c.m, obs[:, :, nsoft:] if nsoft < c.ncol else None, c.ov[nsoft:], liks, c.ov[:nsoft], c.q)
    check("%s %s mu=%g T=%d %s" % (which, name, mu, T, form), which, got, (post, filt, ll, st))


# ---------------------------------------------------------------------------
# 3. posterior rows fed back as weights

@pytest.mark.parametrize("which", [FB, FILTER])
@pytest.mark.parametrize("shift", [0, -700])
def test_rows_fed_back(shift, which):
    """forward_backward_inference's rows of two_blocks() -- exact zeros on the
    block the chain never reaches -- as the weights of soft_vars = [Q1] of a
    second model, as they are and times 2^-700."""
    m, P1, M1, _ = tg.two_blocks()
    m2, Q1, _, (A, pi, Es) = tg.hmm(4, 4, True)
    Bq, T = 3, 64
    obs = tg.gappy(Bq, T, (4,), 91)
    post, _, st = nip_amd.forward_backward_inference(m, torch.from_numpy(obs).cuda(), [M1], [P1])
    fed = post * 2.0 ** shift
    rows, ll, st2 = tg.DEVICE[which](m2, None, [], fed, [Q1], [Q1])
    assert nip_amd.last_kernel() == tg.KERNEL
    torch.cuda.synchronize()
    fed = fed.cpu().numpy()
    assert np.all(st.cpu().numpy() == 0) and np.all(fed[:, :, 2:] == 0.0) and np.all(fed.max(axis=2) > 0.0)
    args = ([so.HARD, so.SOFT], [np.full((Bq, T), -1), None], [None, fed])
    ref = tsa.wide_smoother(A, pi, Es + [np.eye(4)], *args)  # the conditions on this input, as test_soft_api's
    tsa.usable(ref)
    want = so._run(A, pi, Es + [np.eye(4)], *args)
    tsa.pinned(want, ref, "the fed rows")
    check("%s fed rows 2^%d" % (which, shift), which, (rows.cpu().numpy(), ll.cpu().numpy(), st2.cpu().numpy()), want)


# ---------------------------------------------------------------------------
# 4. unchanged semantics, inside the scaled batches

SEMANTICS = ["hmm16", "demo20-both", "hmm3x20-long"]


def neighbours_unchanged(good, got, victim):
    for b in range(B):
        if b != victim:
            assert np.array_equal(got[0][b], good[0][b]) and got[1][b] == good[1][b] and got[2][b] == good[2][b], b


@pytest.mark.parametrize("which", [FB, FILTER])
@pytest.mark.parametrize("value", [np.nan, -1.0, np.inf])
@pytest.mark.parametrize("entry", [0, -1])
@pytest.mark.parametrize("name", SEMANTICS)
def test_a_bad_weight_in_a_scaled_batch(name, entry, value, which):
    """entry 0: the weight that the lanes past the vector's end copy; -1: the
    last one (of hmm3x20-long: in the vector's second piece)."""
    T, victim, t = 24, 3, 7
    r, obs, liks, _ = scaled_inputs(name, T, 560)
    good = memo(("scaled", name, T, which), lambda: device(which, r, obs, liks))
    bad = [w.copy() for w in liks]
    bad[-1][victim, t, entry] = value
    rows, ll, st = device(which, r, obs, bad)
    assert st[victim] == (nip_amd.STATUS_BAD_EVIDENCE | nip_amd.STATUS_ZERO_MASS) == 5 and ll[victim] == -DBL_MAX
    assert not np.isnan(rows).any() and not np.isnan(ll).any()
    if which == FB:
        assert np.all(rows[victim] == 0.0)
    else:
        assert np.array_equal(rows[victim, :t], good[0][victim, :t]) and np.all(rows[victim, t:] == 0.0)
    neighbours_unchanged(good, (rows, ll, st), victim)


@pytest.mark.parametrize("which", [FB, FILTER])
@pytest.mark.parametrize("name", SEMANTICS)
def test_an_all_zero_vector_in_a_scaled_batch(name, which):
    T, victim, t = 24, 2, 9
    r, obs, liks, _ = scaled_inputs(name, T, 560)
    good = memo(("scaled", name, T, which), lambda: device(which, r, obs, liks))
    zero = [w.copy() for w in liks]
    zero[0][victim, t] = 0.0
    rows, ll, st = device(which, r, obs, zero)
    assert st[victim] == nip_amd.STATUS_ZERO_MASS == 1 and ll[victim] == -DBL_MAX
    assert not np.isnan(rows).any() and not np.isnan(ll).any()
    if which == FB:
        assert np.all(rows[victim] == 0.0)
    else:
        assert np.array_equal(rows[victim, :t], good[0][victim, :t]) and np.all(rows[victim, t:] == 0.0)
    neighbours_unchanged(good, (rows, ll, st), victim)


@pytest.mark.parametrize("which", [FB, FILTER])
@pytest.mark.parametrize("name", ["hmm16", "demo20-both", "demo20-a-soft-b-hard", "five-children-4-soft"])
def test_batch_independence_under_the_patterns(name, which):
    """The whole batch, the reversed batch and each sequence alone (pattern 6's
    random exponents among them): the same bits."""
    T = 24
    r, obs, liks, _ = scaled_inputs(name, T, 560)
    cut = lambda b: (obs[b], [w[b] for w in liks])
    whole = memo(("scaled", name, T, which), lambda: device(which, r, obs, liks))
    rev = device(which, r, *cut(slice(None, None, -1)))
    for a, b in zip(whole, rev):
        assert np.array_equal(a, b[::-1])
    for k in range(B):
        alone = device(which, r, *cut(slice(k, k + 1)))
        for a, b in zip(whole, alone):
            assert np.array_equal(a[k:k + 1], b), k
