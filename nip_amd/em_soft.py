"""em_learn over the batched e_step under soft (likelihood) evidence.

em.py's driver loop on one GPU -- m_step first (entering the initial
parameters), pseudo-counts 1.0, the per-iteration average log-likelihood
appended to the learning curve, the same stopping rule with
MIN_EM_ITERATIONS -- with estep_partial_soft in place of estep_partial, so
that an upper model is trained on the posterior rows of the model below it
and not on their arg-max.  The reference has no EM over uncertain series:
its exit on a positive likelihood is not taken (weights above 1 make a
positive ll legitimate), and a sequence fails when its status word is
nonzero.  Data-parallel training is left out; the partial's format (the wide
chain slab, combined by the fixed-order tree) already allows it.
"""
from __future__ import annotations

import numpy as np

from .em import MIN_EM_ITERATIONS, NIP_ERROR_BAD_LUCK, NIP_NO_ERROR


def iteration_soft(model, params, obs, obs_vars, lik, soft_vars):
    """One iteration: m_step(params), the e_step of the batch with
    pseudo-counts 1.0, finalize.  Returns (new params (host), ll, number of
    failed sequences)."""
    from . import estep_finalize, estep_partial_soft, tree_sum
    model.m_step(params)
    partial, ll, status = estep_partial_soft(model, obs, obs_vars, lik, soft_vars)
    counts = estep_finalize(model, partial, None)         # pseudo-counts 1.0 + the families
    loglikelihood = float(tree_sum(ll).cpu()[0])
    n_bad = int((status != 0).sum().cpu())
    return counts.cpu().numpy(), loglikelihood, n_bad


def em_learn_soft(model, obs, obs_vars, lik, soft_vars, threshold, learning_curve=None, init=None,
                  max_iterations=None, seed=None):
    """em_learn for sequences with soft evidence.

    obs: CUDA int32 [B, T, len(obs_vars)] or None; lik: CUDA float64 [B, T, W],
    W = sum card(soft_vars), as forward_backward_inference_soft takes them.
    init: initial parameters in the em_learn layout (numpy's generator seeded
    by ``seed`` when None).  max_iterations: optional cap.  Returns
    NIP_NO_ERROR, or NIP_ERROR_BAD_LUCK when a status word is nonzero or the
    likelihood decreases by more than ts_steps * threshold; the model keeps
    the parameters of the last m_step.
    """
    if learning_curve is not None:
        del learning_curve[:]
    P = model.param_size()
    if init is None:
        init = np.random.default_rng(seed).random(P)
    params = np.array(init, dtype=np.float64).reshape(P)
    ref = lik if lik is not None else obs
    ts_steps = int(ref.shape[0]) * int(ref.shape[1])
    loglikelihood = -np.finfo(np.float64).max
    i = 0
    while True:
        old_loglikelihood = loglikelihood
        new, loglikelihood, n_bad = iteration_soft(model, params, obs, obs_vars, lik, soft_vars)
        if n_bad:
            return NIP_ERROR_BAD_LUCK
        params = new
        if learning_curve is not None:
            learning_curve.append(loglikelihood / ts_steps)
        if old_loglikelihood > loglikelihood + ts_steps * threshold or loglikelihood == -np.inf:
            return NIP_ERROR_BAD_LUCK
        i += 1
        if max_iterations is not None and i >= max_iterations:
            return NIP_NO_ERROR
        if not ((loglikelihood - old_loglikelihood) > ts_steps * threshold or i < MIN_EM_ITERATIONS):
            return NIP_NO_ERROR
