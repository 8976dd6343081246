"""Three and four observed columns through the lane-group kernels
(nip_amd/csrc/chain_group.h: chain_viterbi_kernel and chain_stream_kernel
share one NP x ncol launch ladder, and no other test model has more than two
observed columns).

The model is the star of tests/test_stream_api.py: P0 -> P1 plus four leaf
children O_k | P1 of cardinalities 2, 3, 4, 5 -- all different, so that a
swapped table or cardinality shows -- at 3 interface states (NP = 16) and 17
(NP = 32).  The observed lists: three children in non-declaration order, all
four, and three children plus the interface variable itself.  B = 5, T = 7,
20 % missing.

The oracles and tolerances are those of tests/test_gpu_viterbi.py (the numpy
Viterbi, logp within 1e-11 max(1, |optimum|); the paths here must be equal) and
tests/test_gpu_stream.py (stream_util.fixed_lag: rows 1e-12, ll 1e-11 max(1, |ll|)).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import nip_amd
from nip_amd import synth

import stream_util as su
import viterbi_util as vu
from textbook_util import chain_tables

import test_gpu_stream as tgs
import test_gpu_viterbi as tgv

CARDS = (2, 3, 4, 5)
B, T = 5, 7
# observed lists: children by index, "P" = the interface variable
LISTS = {"three-children": (2, 0, 3), "four-children": (0, 1, 2, 3), "three-and-interface": (3, 1, "P", 0)}


@functools.lru_cache(maxsize=None)
def star(N):
    nodes = [("P0", N, "P1"), ("P1", N, None)] + [("O%d" % k, c, None) for k, c in enumerate(CARDS)]
    pots = [("P1", ["P0"], synth.cpt(1 + N, N, N)), ("P0", [], synth.cpt(2 + N, N, 1))]
    pots += [("O%d" % k, ["P1"], synth.cpt(3 + N + k, c, N)) for k, c in enumerate(CARDS)]
    m = nip_amd.Model.from_spec(nodes, pots)
    kids = [m.variable("O%d" % k) for k in range(4)]
    return m, m.variable("P1"), kids, chain_tables(m, m.variable("P0"), m.variable("P1"), kids)


@functools.lru_cache(maxsize=None)
def case(N, which):
    """The model, the observed list, the observations [B, T, ncol] in its
    order, and the oracle's tables and columns: every child's table (column -1
    where the list leaves it out), then the identity for the interface."""
    m, P1, kids, (A, pi, Es) = star(N)
    lst = LISTS[which]
    ov = [P1 if k == "P" else kids[k] for k in lst]
    obs = tgv.gappy(B, T, [N if k == "P" else CARDS[k] for k in lst], 17 * N + len(which))
    cols = [obs[:, :, lst.index(k)] if k in lst else np.full((B, T), -1) for k in range(4)]
    Es = list(Es)
    if "P" in lst:
        Es.append(np.eye(N))
        cols.append(obs[:, :, lst.index("P")])
    return m, P1, ov, obs, (A, pi, Es), cols


@pytest.mark.parametrize("which", sorted(LISTS))
@pytest.mark.parametrize("N", [3, 17])
def test_most_likely_states(N, which):
    m, P1, ov, obs, (A, pi, Es), cols = case(N, which)
    path, logp, st = tgv.gpu_mlss(m, obs, ov, [P1])                  # asserts last_kernel()
    want, opt = vu.viterbi(A, pi, Es, cols)
    assert np.all(opt > -vu.DBL_MAX) and np.all(st == 0)
    print("max |logp - optimum| %.3g" % np.abs(logp - opt).max())
    assert np.array_equal(path[:, :, 0], want)
    assert np.all(np.abs(logp - opt) <= tgv.TOL * np.maximum(1.0, np.abs(opt)))


@pytest.mark.parametrize("L", [0, 2])
@pytest.mark.parametrize("which", sorted(LISTS))
@pytest.mark.parametrize("N", [3, 17])
def test_stream(N, which, L):
    m, P1, ov, obs, (A, pi, Es), cols = case(N, which)
    rows, ll, st = tgs.stream_rows(m, ov, [P1], obs, L, [3, 4])      # asserts last_kernel()
    want, want_ll = su.fixed_lag(A, pi, Es, cols, L)
    tgs.check_rows(rows, want, tgs.ROW_TOL)
    tgs.check_ll(ll, want_ll)
    assert np.all(st == 0)
