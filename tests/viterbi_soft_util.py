"""The oracle of most_likely_states_soft (nipamd_mlss_soft): viterbi_util's
recursion and score with soft_util.step_evidence as the step evidence, in plain
numpy over an interface chain's own tables, vectorised over sequences.

  e_t[y]     = prod_hard E_k[y][o_{k,t}]  prod_soft sum_o w_{k,t}[o] E_k[y][o]
  delta_0    = (pi A) o e_0
  delta_t[y] = (max_x delta_{t-1}[x] A[x][y]) e_t[y],  psi_t[y] = the lowest x attaining the max
  logp       = ln max_y delta_{T-1}[y]   with the weights as given

step_evidence uses every soft vector at the scale of its largest valid weight
and returns the exponent taken out; those exponents are added to logp (and to
path_score_soft), so 2^k w gives the path of w bit for bit and adds k ln 2.  A
weight that is negative, NaN or infinite leaves its step without evidence: the
sequence is dead (path -1, logp -DBL_MAX, status 1 | 4); an all-zero vector or
evidence without overlap gives status 1 alone.

dtype=np.longdouble runs the recursion (not the step evidence, which is the
definition's fp64 value) in the wider format: where the fp64 and the wide
recursion disagree on a path, two paths tie to within fp64 rounding.
tests/test_viterbi_soft_api.py holds every input that tests/
test_gpu_viterbi_soft.py compares with this oracle to at most 2 % such
sequences per batch; the inputs themselves are below, one definition for both
files.  An input that fails that condition gets another seed in SEEDS here.
"""
import itertools

import numpy as np

import soft_scale_util as ssu
import soft_util as so
from soft_util import HARD, SOFT
from viterbi_util import DBL_MAX, LN2


def _steps(Es, kinds, cols, liks):
    T = next(c.shape[1] for kind, c in zip(kinds, cols) if kind == HARD) if HARD in kinds else \
        next(w.shape[1] for kind, w in zip(kinds, liks) if kind == SOFT)
    return [so.step_evidence(Es, kinds, cols, liks, t) for t in range(T)]


def viterbi_soft(A, pi, Es, kinds, cols, liks, dtype=np.float64):
    """(path [B, T] int64, logp [B] float64, status [B] int64); kinds, cols and
    liks as soft_util.step_evidence takes them."""
    ev = _steps(Es, kinds, cols, liks)
    T, (B, N) = len(ev), ev[0][0].shape
    Aw = np.asarray(A, dtype)
    d = (np.asarray(pi, dtype) @ Aw)[None, :] * ev[0][0].astype(dtype)
    bad = ev[0][1].copy()
    esum = ev[0][2].astype(np.int64)
    psi = np.zeros((B, T, N), np.int64)
    for t in range(1, T):
        e, b, k = ev[t]
        bad |= b
        _, ex = np.frexp(d.max(axis=1))
        d = np.ldexp(d, -ex[:, None])
        esum += ex + k
        p = d[:, :, None] * Aw[None, :, :]                  # [B, x, y]
        psi[:, t] = p.argmax(axis=1)                        # numpy: the lowest index
        d = p.max(axis=1) * e.astype(dtype)
    m = d.max(axis=1)
    dead = ~(m > 0)
    path = np.zeros((B, T), np.int64)
    path[:, T - 1] = d.argmax(axis=1)
    rows = np.arange(B)
    for t in range(T - 1, 0, -1):
        path[:, t - 1] = psi[rows, t, path[:, t]]
    with np.errstate(divide="ignore"):
        logp = np.where(dead, -DBL_MAX, np.asarray(np.log(np.where(dead, 1.0, m)) + esum * dtype(LN2), np.float64))
    path[dead] = -1
    assert not np.any(bad & ~dead)
    return path, logp, dead.astype(np.int64) | (bad.astype(np.int64) << 2)


def path_score_soft(A, pi, Es, kinds, cols, liks, path):
    """ln of the measure of (path, evidence) per sequence under the weights as
    given: the sum of the log terms of a path [B, T] plus the exponents taken
    out of the vectors; -inf where a term is 0 or a weight is bad."""
    ev = _steps(Es, kinds, cols, liks)
    B, T = path.shape
    rows = np.arange(B)
    ksum = np.zeros(B, np.int64)
    with np.errstate(divide="ignore"):
        s = np.log((pi @ A)[path[:, 0]])
        for t in range(T):
            e, _, k = ev[t]                                 # (a bad step's e is 0)
            if t > 0:
                s = s + np.log(A[path[:, t - 1], path[:, t]])
            s = s + np.log(e[rows, path[:, t]])
            ksum += k
    return s + ksum * LN2


def brute_force_soft(A, pi, Es, kinds, cols, liks, b):
    """Sequence b: the maximum of path_score_soft over all N^T paths, and the
    lexicographically lowest maximiser."""
    T = len(_steps(Es, kinds, cols, liks))
    paths = np.array(list(itertools.product(range(A.shape[0]), repeat=T)), np.int64)
    n = paths.shape[0]
    tile = lambda a: None if a is None else np.repeat(np.asarray(a)[b:b + 1], n, axis=0)
    s = path_score_soft(A, pi, Es, kinds, [tile(c) for c in cols], [tile(w) for w in liks], paths)
    k = int(s.argmax())
    return float(s[k]), paths[k]


# ---------------------------------------------------------------------------
# the inputs of tests/test_gpu_viterbi_soft.py that meet the oracle

# (name, B, T): B not a multiple of the sequences per wave (4, 2, 1) nor of a
# block; T around a back-pointer run (16, 12, 10 steps) and the 16-step path stores
PERIODS = [("hmm16", B, T) for B, T in ((1, 1), (5, 2), (6, 3), (5, 15), (5, 16), (5, 17), (6, 33), (33, 129))] + \
          [("demo20-both", 5, T) for T in (11, 12, 13, 25)] + \
          [("demo33-a-soft-b-hard", 5, T) for T in (9, 10, 11, 21)]
LONG = ("hmm16-proper", 8, 4097)
BRUTE = (3, 4, 8, 6)                                         # N, M, B, T

# seed offsets of period_case / long_case inputs, keyed by (name, B, T); 0 unless listed
SEEDS = {}

_requests = {}


def requests():
    """soft_scale_util.requests() and the one request only the periods use."""
    if not _requests:
        import test_gpu_soft as tg
        _requests.update(ssu.requests())
        m, v, tables = tg.demo1(33)
        _requests["demo33-a-soft-b-hard"] = ssu.Req("demo33-a-soft-b-hard", m, tables, (0,), (1,), [v["A1"]],
                                                    [v["B1"]], [v["C1"]], None)
    return _requests


def drawn(r, B, T, seed):
    """(obs int32 [B, T, n_hard], 20 % missing; one [B, T, M] weight array per
    soft column, 0.05 + U[0, 1))."""
    rng = np.random.default_rng(8000 + 100 * T + B + seed)
    cs = ssu.cards(r, r.hard)
    obs = np.stack([rng.integers(0, c, size=(B, T)) for c in cs], axis=2).astype(np.int32) if cs \
        else np.zeros((B, T, 0), np.int32)
    obs[rng.random(obs.shape) < 0.2] = -1
    return obs, [0.05 + rng.random((B, T, c)) for c in ssu.cards(r, r.soft)]


def grid_case(name, T):
    """The scale grid's control: soft_scale_util's base weights and codes, B = 7."""
    r = requests()[name]
    return r, ssu.hard_obs(r, T), ssu.base_weights(r, T)


def edge_case(name, T):
    r = requests()[name]
    return r, ssu.hard_obs(r, T), ssu.edge_weights(r, T)


def period_case(name, B, T):
    r = requests()[name]
    return (r,) + drawn(r, B, T, SEEDS.get((name, B, T), 0))


def long_case():
    return period_case(*LONG)


def fed_case():
    """Rows fed back: ((m1, ov1, q1, tables1, codes1), r2, obs2).  The first
    hmm16's smoothed rows on [P1] under codes1 are the likelihood vectors of
    the second hmm16's interface variable itself -- a column whose table is
    the identity -- beside its child's hard codes obs2."""
    import test_gpu_soft as tg
    B, T = 5, 40
    m1, P1, M1, tables1 = tg.hmm(16, 16, False)
    m2, Q1, N1, (A, pi, Es) = tg.hmm(16, 16, True, seed=5)
    r2 = ssu.Req("fed", m2, (A, pi, Es + [np.eye(16)]), (1,), (0,), [Q1], [N1], [Q1], None)
    return (m1, [M1], [P1], tables1, tg.gappy(B, T, (16,), 91)), r2, tg.gappy(B, T, (16,), 92)


def oracle_cases():
    """(label, (r, obs, liks)) of every input above.  (The scale grid's scaled
    batches are exact rescalings of grid_case's: the same e_t, bit for bit.)"""
    for name in ssu.NAMES:
        for T in ssu.TS:
            yield "grid %s T=%d" % (name, T), grid_case(name, T)
            yield "edge %s T=%d" % (name, T), edge_case(name, T)
    for name, B, T in PERIODS + [LONG]:
        yield "%s B=%d T=%d" % (name, B, T), period_case(name, B, T)


def oracle(r, obs, liks, dtype=np.float64):
    A, pi, Es = r.tables
    return viterbi_soft(A, pi, Es, *ssu.oracle_args(r, obs, liks), dtype=dtype)


def score(r, obs, liks, path):
    A, pi, Es = r.tables
    return path_score_soft(A, pi, Es, *ssu.oracle_args(r, obs, liks), path)


def joint_state(r, path):
    """path [B, T, nq] as the interface state [B, T] (a joint interface: the digits' sum)."""
    if r.digits is None:
        return path[:, :, 0].astype(np.int64)
    return sum(path[:, :, j].astype(np.int64) * s for j, (s, _) in enumerate(r.digits))
