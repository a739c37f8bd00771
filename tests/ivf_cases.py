"""Shared pieces of the IVF-Flat tests: the fp64 restatement of the probe search, the spherical centroid
update in fp64 with its derived error bound, and the seeded case builders.  The scoring, the order and the
validity check of a top-k are retrieval_cases.py's (RC).

Probe search.  faiss.IndexIVFFlat.search with METRIC_INNER_PRODUCT as the reference's
scripts/build_index_with_captions.py builds it: the candidates of a query are the rows of the lists it
probes; among them the search is the flat one (RC.rank_scores: fp64 scores, (score desc, id asc), NaN rows
left out, filler -1 / -inf).

Update bound.  A centroid is c = s / ||s||, s the sum of its m member rows.  An f32 summation of m terms
in any order satisfies |s^_j - s_j| <= 2 m 2^-24 sum_i |x_ij| per component (the factor 2 as in RC's E), so
d = ||s^ - s|| <= 2 m 2^-24 S1 with S1 = sum_i ||x_i||.  Normalising moves the direction by at most
2 d / ||s||, and the f32 sum of squares (dim terms), square root and division scale every component by
1 + e, |e| <= 2 (dim + 2) 2^-24.  With |c_j| <= 1:
    |c^_j - c_j| <= 4 m 2^-24 S1 / ||s|| + 2 (dim + 2) 2^-24 = update_bound(m, dim, S1, ||s||),
which also bounds ||c^ - c||_2 when the last term is doubled (direction and scale errors add as vectors).
"""
from __future__ import annotations

import numpy as np

import retrieval_cases as RC

U32 = RC.U32


# ---------------------------------------------------------------------------------- probe search
def probed_rows(assign, probes_j) -> np.ndarray:
    """Positions (ascending) of the rows whose list one query probes; -1 probes name no list."""
    lists = np.asarray(probes_j, np.int64)
    return np.flatnonzero(np.isin(np.asarray(assign, np.int64), lists[lists >= 0]))


def probe_search_reference(db, assign, probes, q, k: int):
    """fp64 probe search over rows db [n, dim] (already storage-rounded; row i has id i and lies in list
    assign[i]) for queries q [nq, dim] probing probes [nq, nprobe] -> (D [nq, k] f64, I [nq, k] int64)."""
    db, q = np.asarray(db, np.float64), np.asarray(q, np.float64)
    D, I = np.full((q.shape[0], k), -np.inf), np.full((q.shape[0], k), -1, np.int64)
    for j in range(q.shape[0]):
        sub = probed_rows(assign, probes[j])
        d, i = RC.rank_scores(RC.scores_fp64(db[sub], q[j:j + 1])[0] if sub.size else np.zeros(0), k)
        D[j] = d
        I[j, i >= 0] = sub[i[i >= 0]]
    return D, I


def probe_search_loops(db, assign, probes, q, k: int):
    """The same search as plain Python loops (tiny inputs only): the check of the restatement."""
    D, I = [], []
    for qv, pl in zip(q, probes):
        scored = []
        for i, row in enumerate(db):
            if int(assign[i]) not in [int(p) for p in pl if int(p) >= 0]:
                continue
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


def check_probe_topk(D, I, db, assign, probes, q, k: int) -> None:
    """RC.check_topk of every query against the rows of exactly the lists it probes, the returned original
    ids mapped to positions among those rows (ascending ids stay ascending)."""
    D, I, db = np.asarray(D), np.asarray(I, np.int64), np.asarray(db)
    q = np.asarray(q)
    for j in range(q.shape[0]):
        sub = probed_rows(assign, probes[j])
        got = I[j][I[j] >= 0]
        assert np.isin(got, sub).all(), f"query {j}: a row outside the probed lists was returned"
        pos = np.where(I[j] >= 0, np.searchsorted(sub, np.where(I[j] >= 0, I[j], 0)), -1)
        RC.check_topk(D[j:j + 1], pos[None], db[sub].reshape(-1, db.shape[1]), q[j:j + 1], k)


def assign_reference(x, centroids) -> np.ndarray:
    """fp64 arg-max inner product, lowest id on ties, -1 where every score is NaN."""
    S = np.asarray(x, np.float64) @ np.asarray(centroids, np.float64).T
    best = np.where(np.isnan(S), -np.inf, S)
    out = best.argmax(1)
    out[np.isnan(S).all(1)] = -1
    return out


# ---------------------------------------------------------------------------------- centroid update
def spherical_update_fp64(x, assign, prev):
    """-> (centroids f64 [nlist, dim], m [nlist], S1 [nlist], snorm [nlist]): the normalised fp64 sum of each
    list's members (rows with assign -1 belong to none); an empty list keeps prev's row."""
    x, prev = np.asarray(x, np.float64), np.asarray(prev, np.float64)
    nlist = prev.shape[0]
    out, m, S1, sn = prev.copy(), np.zeros(nlist, np.int64), np.zeros(nlist), np.zeros(nlist)
    norms = np.linalg.norm(x, axis=1)
    for l in range(nlist):
        rows = np.flatnonzero(np.asarray(assign) == l)
        m[l] = rows.size
        if rows.size:
            s = x[rows].sum(0)
            S1[l], sn[l] = norms[rows].sum(), np.linalg.norm(s)
            out[l] = s / max(sn[l], 1e-12)
    return out, m, S1, sn


def update_bound(m, dim: int, S1, snorm):
    """Per-component bound on a computed centroid against spherical_update_fp64's (0 for an empty list)."""
    m, S1, snorm = np.asarray(m, np.float64), np.asarray(S1, np.float64), np.asarray(snorm, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        b = 4.0 * m * U32 * S1 / snorm + 2.0 * (dim + 2) * U32
    return np.where(m > 0, b, 0.0)


# ---------------------------------------------------------------------------------- builders
def unit(x) -> np.ndarray:
    x = np.asarray(x, np.float64)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def clustered_rows(seed: int, n: int, dim: int, ncenters: int, spread: float = 0.3):
    """n unit rows around ncenters random unit centres (row i around centre i % ncenters), f32."""
    rng = np.random.default_rng(seed)
    centres = unit(rng.standard_normal((ncenters, dim)))
    x = centres[np.arange(n) % ncenters] + spread * rng.standard_normal((n, dim)) / np.sqrt(dim)
    return unit(x).astype(np.float32), centres.astype(np.float32)


def rows_near(seed: int, centroids, lengths, spread: float = 0.05):
    """Unit rows that are small perturbations of chosen centroids: lengths[l] rows near centroids[l], the
    lists interleaved in a seeded order -> (rows f32 [sum, dim], the list each row was built for)."""
    rng = np.random.default_rng(seed)
    centroids = np.asarray(centroids, np.float64)
    want = rng.permutation(np.repeat(np.arange(len(lengths)), lengths))
    x = centroids[want] + spread * rng.standard_normal((want.size, centroids.shape[1])) / np.sqrt(centroids.shape[1])
    return unit(x).astype(np.float32), want


def integer_rows_case(seed: int, dim: int, lengths):
    """Rows of small integers (-2..3, none all zero) dealt to lists of the given lengths in a seeded order ->
    (rows f32 [n, dim], assign int [n]).  Every f32 sum of such rows is exact in any order (|sum| <= 3 n <
    2^24), so a centroid update over them must equal the normalised exact sum bit for bit, and losing any
    row, chunk tail or chunk changes the integer sum."""
    rng = np.random.default_rng(seed)
    assign = rng.permutation(np.repeat(np.arange(len(lengths)), lengths))
    x = rng.integers(-2, 4, (assign.size, dim)).astype(np.float32)
    x[(x == 0).all(1), 0] = 1.0
    return x, assign


def member_sums(x, assign, nlist: int, drop=None) -> np.ndarray:
    """fp64 sums [nlist, dim] of each list's members in row order; drop(l, m) -> the member positions
    (0 .. m - 1, in row order) a broken summation would lose for list l of m members."""
    x = np.asarray(x, np.float64)
    out = np.zeros((nlist, x.shape[1]))
    for l in range(nlist):
        rows = np.flatnonzero(np.asarray(assign) == l)
        if drop is not None and rows.size:
            rows = np.delete(rows, [p for p in drop(l, rows.size) if 0 <= p < rows.size])
        out[l] = x[rows].sum(0)
    return out


def truncations(chunk: int):
    """The summation errors the chunk-boundary lengths exist to catch, as drop(l, m) functions by name."""
    return {
        "last row": lambda l, m: [m - 1] if m > 1 else [],
        "first row": lambda l, m: [0] if m > 1 else [],
        "tail chunk": lambda l, m: range((m - 1) // chunk * chunk, m) if m > chunk else [],
        "first chunk": lambda l, m: range(0, chunk) if m > chunk else [],
        "middle chunk": lambda l, m: range(chunk, 2 * chunk) if m > 2 * chunk else [],
        "row at the chunk boundary": lambda l, m: [chunk - 1] if m >= chunk else [],
        "row past the chunk boundary": lambda l, m: [chunk] if m > chunk else [],
    }


def orthonormal_centroids(seed: int, nlist: int, dim: int) -> np.ndarray:
    """nlist <= dim orthonormal rows, f32: a row near one of them is far from every other."""
    return RC.orthonormal_queries(np.random.default_rng(seed), nlist, dim).astype(np.float32)
