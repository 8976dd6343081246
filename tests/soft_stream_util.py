"""The oracle of online inference under soft evidence (nip_amd.Stream with
soft_vars, nipamd_stream_push_soft): stream_util.fixed_lag with
soft_util.step_evidence as the step evidence and soft_util._run's forward pass,
in plain numpy over an interface chain's own tables, vectorised over sequences.

  row t = P(x_t | e_0 .. e_{min(t + L, T - 1)})
        = normalise(alpha^_t o beta),  beta = 1 at the endpoint,
          beta <- A (e_j o beta) for j = endpoint .. t + 1

A sequence whose step mass is zero at step d (an all-zero vector, a bad weight,
no overlap with the states the chain can be in) is dead from d on, by the
streams' rule (include/nip_amd.h): row t is all zeros where min(t + L, T - 1)
>= d, ll = -DBL_MAX, status 1, or 5 when a bad weight was met.  Rows with an
earlier endpoint are those of the live sequence.  tests/test_soft_stream_api.py
pins this oracle to soft_util.soft_smoother and to stream_util.fixed_lag.
"""
import numpy as np

from soft_util import HARD, SOFT, _run, step_evidence  # noqa: F401  (HARD, SOFT: for the callers)


def soft_fixed_lag(A, pi, Es, kinds, cols, liks, L):
    """kinds / cols / liks as soft_util.step_evidence takes them.  Returns the
    fixed-lag rows [B, T, N], the ll [B] of all T steps and the status [B]."""
    _, ah, ll, status = _run(A, pi, Es, kinds, cols, liks)
    B, T, N = ah.shape
    ev = [step_evidence(Es, kinds, cols, liks, t)[0] for t in range(T)]
    nomass = ah.sum(axis=2) == 0.0                          # alpha^ sums to 1 while there is mass
    dead = np.where(nomass.any(axis=1), nomass.argmax(axis=1), T)   # the first step without mass (T: none)
    rows = np.zeros_like(ah)
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(T):
            end = min(t + L, T - 1)
            ok = end < dead
            b = np.ones((B, N))
            for j in range(end, t, -1):
                b = (ev[j] * b) @ A.T
                b = np.where(ok[:, None], b / b.sum(axis=1, keepdims=True), 0.0)
            p = ah[:, t] * b
            rows[:, t] = np.where(ok[:, None], p / p.sum(axis=1, keepdims=True), 0.0)
    return rows, ll, status
