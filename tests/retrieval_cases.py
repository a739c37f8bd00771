"""Shared pieces of the retrieval tests: the fp64 restatement of the flat inner-product search, the derived
error bound, the validity check of a returned top-k, and the seeded case builders.

Restatement.  faiss.IndexFlatIP.search as the reference uses it (scripts/query_video.py:127,
scripts/eval_retrieval.py:40): every score in fp64, rows ordered by (score descending, id ascending), the
first k returned; a row whose score is NaN is left out, and a short list ends in id -1 / score -inf.

Bound.  An f32 accumulation of `dim` products in any order satisfies
    |s - s*| <= 2 * dim * 2^-24 * ||q|| * ||x|| = E
(the factor 2 covers a truncating accumulator, the convention of the lm_head screen bound in
include/vcap.h).  With unit vectors at dim 256, E = 3.05e-5.  For bf16 storage the restatement runs on the
bf16-rounded rows, so the same E applies; the rounding itself is pinned bit-exact by its own test.
"""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24


def error_bound(dim: int, qnorm, xnorm):
    return 2.0 * dim * U32 * np.asarray(qnorm, np.float64) * np.asarray(xnorm, np.float64)


def scores_fp64(db, q) -> np.ndarray:
    """[nq, n] fp64 inner products of the given (already storage-rounded) rows."""
    db = np.asarray(db, np.float64).reshape(-1, np.asarray(q).shape[-1])
    return np.asarray(q, np.float64) @ db.T


def rank_scores(s: np.ndarray, k: int):
    """One query's fp64 scores [n] -> (D [k], I [k]): (score desc, id asc), NaN rows left out, filler -inf / -1."""
    ids = np.flatnonzero(~np.isnan(s))
    order = ids[np.lexsort((ids, -s[ids]))][:k]
    D = np.full(k, -np.inf)
    I = np.full(k, -1, np.int64)
    D[:order.size], I[:order.size] = s[order], order
    return D, I


def flat_ip_reference(db, q, k: int):
    """fp64 flat-IP search -> (D [nq, k] f64, I [nq, k] int64)."""
    S = scores_fp64(db, q)
    out = [rank_scores(S[j], k) for j in range(S.shape[0])]
    return np.stack([d for d, _ in out]), np.stack([i for _, i in out])


def brute_force(db, q, k: int):
    """The same search as plain Python loops (tiny inputs only): the check of the restatement."""
    D, I = [], []
    for qv in q:
        scored = []
        for i, row in enumerate(db):
            s = 0.0
            for a, b in zip(row, qv):
                s += float(a) * float(b)
            if s == s:
                scored.append((-s, i))
        scored.sort()
        top = scored[:k]
        D.append([-s for s, _ in top] + [-np.inf] * (k - len(top)))
        I.append([i for _, i in top] + [-1] * (k - len(top)))
    return np.array(D, np.float64), np.array(I, np.int64)


def check_topk(D, I, db, q, k: int):
    """The validity of a returned top-k against the fp64 scores of (db, q); raises AssertionError.
    With t the k-th best fp64 score: every returned id has s* >= t - 2E, every row not returned has
    s* <= t + 2E, every returned score is within E of its id's s*, scores are non-increasing and equal
    scores have ascending ids; rows beyond the valid ones are id -1 / score -inf."""
    D, I = np.asarray(D, np.float64), np.asarray(I, np.int64)
    db = np.asarray(db, np.float64).reshape(-1, np.asarray(q).shape[-1])
    q = np.asarray(q, np.float64)
    n, dim = db.shape
    S = scores_fp64(db, q)
    xn, qn = np.linalg.norm(db, axis=1), np.linalg.norm(q, axis=1)
    assert D.shape == I.shape == (q.shape[0], k)
    for j in range(q.shape[0]):
        s = S[j]
        valid = np.flatnonzero(~np.isnan(s))
        want = min(k, valid.size)
        ids, sc = I[j, :want], D[j, :want]
        assert (I[j, want:] == -1).all() and np.isneginf(D[j, want:]).all(), f"query {j}: filler"
        assert ((ids >= 0) & (ids < n)).all() and np.unique(ids).size == want, f"query {j}: ids"
        assert not np.isnan(s[ids]).any(), f"query {j}: a NaN row was returned"
        E = error_bound(dim, qn[j], xn)
        Emax = float(np.nanmax(E[valid])) if valid.size else 0.0
        assert (np.abs(sc - s[ids]) <= E[ids]).all(), f"query {j}: score error {np.abs(sc - s[ids]).max()}"
        assert (np.diff(sc) <= 0).all(), f"query {j}: scores increase"
        same = np.diff(sc) == 0
        assert (np.diff(ids)[same] > 0).all(), f"query {j}: tied scores not by ascending id"
        if valid.size > k:
            t = np.sort(s[valid])[::-1][k - 1]
            assert (s[ids] >= t - 2 * Emax).all(), f"query {j}: a returned row is below the k-th best"
            rest = np.setdiff1d(valid, ids)
            assert (s[rest] <= t + 2 * Emax).all(), f"query {j}: a better row was not returned"


def bf16_round(x: np.ndarray) -> np.ndarray:
    """f32 -> bf16 (round to nearest even) -> f32, on finite values."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def orthonormal_queries(rng, nq: int, dim: int) -> np.ndarray:
    qm, _ = np.linalg.qr(rng.standard_normal((dim, nq)))
    return np.ascontiguousarray(qm.T)                      # [nq, dim] fp64, orthonormal rows


def separated_case(seed: int, n: int, dim: int, nq: int, k: int, positions=None, gap: float = 2e-3):
    """Unit rows x_i = sum_j a_ij q_j + sqrt(1 - sum_j a_ij^2) r_i over orthonormal queries q_j, r_i
    orthogonal to all of them, so row i scores a_ij against query j.  Per query, `w` winner rows carry
    a = 0.9, 0.9 - gap, ... (w = min(2k, n // nq); winners of different queries are different rows);
    every other a lies in [-0.05, 0.05].  positions[j]: the winner rows of query j in rank order
    (default: seeded random rows).  -> (db f32 [n, dim], q f32 [nq, dim], winners int64 [nq, w])."""
    rng = np.random.default_rng(seed)
    Q = orthonormal_queries(rng, nq, dim)
    w = min(2 * k, n // nq)
    A = rng.uniform(-0.05, 0.05, (n, nq))
    if positions is None:
        positions = rng.permutation(n)[:nq * w].reshape(nq, w)
    positions = np.asarray(positions, np.int64).reshape(nq, w)
    assert np.unique(positions).size == nq * w
    for j in range(nq):
        A[positions[j], j] = 0.9 - gap * np.arange(w)
    R = rng.standard_normal((n, dim))
    R -= (R @ Q.T) @ Q
    R /= np.linalg.norm(R, axis=1, keepdims=True)
    X = A @ Q + np.sqrt(1.0 - (A * A).sum(1, keepdims=True)) * R
    return X.astype(np.float32), Q.astype(np.float32), positions


def assert_separated(db, q, k: int, winners) -> None:
    """The input check before exact-id equality: on the fp64 scores, each query's winners are its best
    rows in order, and every gap among them and down to the best other row exceeds 4E."""
    db64 = np.asarray(db, np.float64)
    S = scores_fp64(db64, q)
    E = float(error_bound(db64.shape[1], np.linalg.norm(np.asarray(q, np.float64), axis=1).max(),
                          np.linalg.norm(db64, axis=1).max()))
    for j in range(S.shape[0]):
        top = S[j, winners[j]]
        assert (-np.diff(top) > 4 * E).all(), f"query {j}: winner gaps {(-np.diff(top)).min()} <= 4E = {4 * E}"
        rest = np.delete(S[j], winners[j])
        if rest.size:
            assert top[-1] - rest.max() > 4 * E, f"query {j}: background within 4E of the winners"
    assert winners.shape[1] >= k, "fewer separated winners than k"
