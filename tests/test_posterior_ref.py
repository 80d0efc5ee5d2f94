"""Posterior decoding, CPU side: the fp64 reference the GPU tests compare against, checked
against brute force and against the C oracle's E-step; and the new entry points at the C-ABI
boundary (no device).

posterior_ref is the 8-state Rabiner-rescaled forward-backward of oracle/pyref.estep8, in numpy
(vectorised over the 8 states and over independent chunks): per position the sum of gamma over
the four '+' states, and the log-likelihood per chunk.  tests/test_gpu_posterior.py imports it.
"""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import coracle as co
from oracle import families as fam
from oracle import pyref as pr

SEED = 20251015


def posterior_ref(model: np.ndarray, obs: np.ndarray):
    """obs: (nch, T) or (T,) symbols 0..3, every row an independent sequence.  Returns
    (P('+') per position, float64, same shape; log-likelihood per row).  A row with
    P(row | model) = 0 at its first position: posteriors 0, log-likelihood -inf."""
    pi, a, b = co.model_split(np.asarray(model, np.float64))
    o = np.atleast_2d(np.asarray(obs)).astype(np.int64)
    nch, T = o.shape
    bt = np.ascontiguousarray(b.T)                     # bt[symbol] = emission column
    al = np.empty((T, nch, 8))
    cs = np.empty((T, nch))
    x = pi[None, :] * bt[o[:, 0]]
    s = x.sum(axis=1)
    dead = s == 0.0
    s = np.where(dead, 1.0, s)
    cs[0] = 1.0 / s
    al[0] = x * cs[0][:, None]
    for t in range(1, T):
        x = (al[t - 1] @ a) * bt[o[:, t]]
        s = x.sum(axis=1)
        cs[t] = 1.0 / np.where(dead, 1.0, s)          # (a dead row stays all zero)
        al[t] = x * cs[t][:, None]
    ll = -np.log(cs).sum(axis=0)
    post = np.empty((nch, T))
    bc = np.ones((nch, 8))
    at = np.ascontiguousarray(a.T)
    for t in range(T - 1, -1, -1):
        g = al[t] * bc
        post[:, t] = g[:, :4].sum(axis=1) / np.where(dead, 1.0, g.sum(axis=1))
        if t:
            bc = ((bt[o[:, t]] * bc) @ at) * cs[t][:, None]
    post[dead] = 0.0
    ll = np.where(dead, -np.inf, ll)
    if np.ndim(obs) == 1:
        return post[0], ll[0]
    return post, ll


def brute_force(model: np.ndarray, obs):
    """All 2^T sign paths (state = base + (0 if '+' else 4): every other path emits with
    probability 0): P('+' at t | obs) and log P(obs)."""
    pi, a, _ = co.model_split(model)
    o = np.asarray(obs, np.int64)
    T = len(o)
    plus = (np.arange(1 << T)[:, None] >> np.arange(T)[None, :]) & 1      # [path, t]
    st = o[None, :] + np.where(plus == 1, 0, 4)
    p = pi[st[:, 0]].copy()
    for t in range(1, T):
        p = p * a[st[:, t - 1], st[:, t]]
    z = p.sum()
    return (p[:, None] * plus).sum(axis=0) / z, math.log(z)


def synth_obs(n: int, start: int = 0) -> np.ndarray:
    from cpgisland_amd import device as D
    packed, _ = D.synth_host(SEED, start, n)
    return pr.unpack(packed, n)


@pytest.mark.parametrize("name", ["initial", "random_norm0"])
@pytest.mark.parametrize("T", [1, 2, 5, 9, 12])
def test_reference_equals_brute_force(name, T):
    model = fam.family(name)
    obs = np.random.default_rng(1000 + T).integers(0, 4, T)
    want, wll = brute_force(model, obs)
    got, ll = posterior_ref(model, obs)
    assert np.max(np.abs(got - want)) <= 1e-12
    assert abs(ll - wll) <= 1e-12 * max(1.0, abs(wll))


def test_reference_rows_are_independent():
    model = fam.family("random_norm0")
    obs = np.random.default_rng(7).integers(0, 4, (3, 200))
    post, ll = posterior_ref(model, obs)
    for r in range(3):   # (the matrix products sum in another order: equal to rounding)
        p1, l1 = posterior_ref(model, obs[r])
        assert np.max(np.abs(p1 - post[r])) <= 1e-12 and abs(l1 - ll[r]) <= 1e-12 * abs(l1)


def test_reference_zero_probability_row():
    model = fam.family("initial").copy()
    model[[2, 6]] = 0.0                                # pi of G+ and G-
    post, ll = posterior_ref(model, np.array([[2, 0, 1, 3], [0, 2, 1, 3]]))
    assert ll[0] == -np.inf and not post[0].any()
    assert np.isfinite(ll[1]) and np.all(post[1] > 0)


def test_reference_matches_oracle_estep_sums():
    """Summed by base, the per-position posteriors are the E-step's emission counts of the '+'
    states; the log-likelihood is the E-step's."""
    T = 65536
    obs = synth_obs(T)
    model = co.initial_model()
    post, ll = posterior_ref(model, obs)
    est = co.estep(model, obs, T)
    for x in range(4):
        want = est[72 + 5 * x]                         # emit[x][x]
        got = post[obs == x].sum()
        assert abs(got - want) <= 1e-9 * want, (x, got, want)
    assert abs(ll - est[104]) <= 1e-9 * abs(est[104])


NEW_SYMBOLS = ["cpg_posterior_d", "cpg_island_confidence_d", "cpg_posterior_states"]


def test_new_symbols_exported_and_bound():
    from cpgisland_amd import _lib
    for n in NEW_SYMBOLS:
        assert n in _lib.SIGNATURES, n
        assert hasattr(_lib.lib, n), n
    from cpgisland_amd import HmmEvaluator
    from cpgisland_amd import device as D
    assert callable(D.posterior) and callable(D.island_confidence)
    assert callable(HmmEvaluator.posterior)


def test_null_context_is_invalid_without_a_device():
    from cpgisland_amd import _lib
    lib = _lib.lib
    assert lib.cpg_posterior_d(None, None, None, 0, 65536, None, None, None, None) == \
        _lib.CPG_E_INVALID
    assert b"null" in lib.cpg_last_error()
    assert lib.cpg_island_confidence_d(None, None, 0, 65536, 0, None, None, 0, None, None) == \
        _lib.CPG_E_INVALID
    ll = C.c_double()
    assert lib.cpg_posterior_states(None, None, None, 0, None, C.byref(ll)) == _lib.CPG_E_INVALID
