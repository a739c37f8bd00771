"""IVF-Flat index on the GPU: vcap_ivf_assign against vcap_ip_search over the centroids (ids and score bits),
vcap_ivf_centroid_update against the fp64 spherical update within the bound derived in ivf_cases.py, training
(seeded, non-decreasing objective), vcap_ivf_search against the fp64 probe search (retrieval_cases.check_topk
over the rows of exactly the probed lists), bit equality with FlatIPIndex when every list is probed, the
determinism contract, self-queries, persistence and the scripts end to end.

Shapes are the smallest that reach every mechanism: row slabs of the assignment (64 rows at dim <= 256, 16 at
dim 1024) and their tails, centroid tiles of 16 and slabs of 128, update chunks and scan slices of 512 rows
and their neighbours, empty lists, every query-tile count of the coarse search."""
import ctypes as C
import json
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import pytest
import torch

import ivf_cases as IC
import retrieval_cases as RC
from vcap import _native as N
from vcap import retrieval as R

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


@contextmanager
def _masked_stream(device):
    """A stream restricted to 32 CUs, current inside the block."""
    h = C.c_void_p()
    N.check(N.lib().vcap_stream_create_cu_reserved(32, C.byref(h)), "masked stream")
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.ExternalStream(h.value, device=device)):
            yield
            torch.cuda.synchronize()
    finally:
        torch.cuda.synchronize()
        N.check(N.lib().vcap_stream_destroy(h), "stream destroy")


def _ip_top1(cent, x):
    """ids and scores of vcap_ip_search(db = centroids, queries = rows, k = 1), the rows in calls of <= 64."""
    per = min(R.MAX_NQ, R.MAX_QUERY_FLOATS // x.shape[1])
    out = [R.ip_search(cent, cent.shape[0], x[s:s + per].contiguous(), 1) for s in range(0, x.shape[0], per)]
    return torch.cat([d[:, 0] for d, _ in out]), torch.cat([i[:, 0] for _, i in out])


# ---------------------------------------------------------------------------------------------- assign
ASSIGN_SHAPES = [(64, 1, 1), (64, 3, 127), (64, 17, 129), (64, 50, 1), (64, 300, 128), (256, 3, 1), (256, 16, 128),
                 (256, 50, 193), (256, 300, 129), (1024, 1, 17), (1024, 17, 127), (1024, 300, 33)]


@pytest.mark.parametrize("dim, nlist, n", ASSIGN_SHAPES)
def test_assign_is_the_flat_search_over_the_centroids(device, dim, nlist, n):
    rng = np.random.default_rng(dim + nlist + n)
    cent, x = _dev(rng.standard_normal((nlist, dim)), device), _dev(rng.standard_normal((n, dim)), device)
    assign, score = R.ivf_assign(x, cent)
    D, I = _ip_top1(cent, x)
    assert torch.equal(assign.to(torch.int64), I) and np.array_equal(_bits(score), _bits(D))
    S = RC.scores_fp64(cent.cpu().numpy(), x.cpu().numpy())
    best = S.max(1)
    E = RC.error_bound(dim, np.linalg.norm(x.cpu().numpy().astype(np.float64), axis=1),
                       np.linalg.norm(cent.cpu().numpy().astype(np.float64), axis=1).max())
    assert (S[np.arange(n), assign.cpu().numpy()] >= best - 2 * E).all()
    assert torch.equal(R.ivf_assign(x, cent, want_scores=False)[0], assign)
    if n > 1:      # strided rows, and a row's result does not depend on the rows around it
        wide = torch.zeros(n, dim + 64, device=device)
        wide[:, :dim] = x
        a2, s2 = R.ivf_assign(wide[:, :dim], cent)
        assert torch.equal(a2, assign) and np.array_equal(_bits(s2), _bits(score))
        a1, s1 = R.ivf_assign(x[n // 2:n // 2 + 1].contiguous(), cent)
        assert int(a1[0]) == int(assign[n // 2]) and np.array_equal(_bits(s1), _bits(score[n // 2:n // 2 + 1]))


def test_assign_ties_go_to_the_lower_id_and_nan_never_wins(device):
    rng = np.random.default_rng(7)
    cent = IC.unit(rng.standard_normal((40, 64))).astype(np.float32)
    cent[33] = cent[2]                         # duplicated centroids: exact ties
    cent[17] = cent[20]
    x, want = IC.rows_near(8, cent, [0, 0, 30] + [0] * 17 + [30] + [2] * 19)
    a, s = R.ivf_assign(_dev(x, device), _dev(cent, device))
    a = a.cpu().numpy()
    assert not np.isin(a, [33, 20]).any() and (a[want == 2] == 2).all() and (a[want == 20] == 17).all()
    D, I = _ip_top1(_dev(cent, device), _dev(x, device))
    assert np.array_equal(a, I.cpu().numpy()) and np.array_equal(_bits(s), _bits(D))
    bad = cent.copy()
    bad[2, 5] = np.nan                          # the best centroid of a third of the rows
    a2, s2 = R.ivf_assign(_dev(x, device), _dev(bad, device))
    assert not (a2 == 2).any() and not torch.isnan(s2).any() and (a2[torch.from_numpy(want == 2).to(device)] == 33).all()
    assert np.array_equal(a2.cpu().numpy(), IC.assign_reference(x, bad))
    a3, s3 = R.ivf_assign(_dev(x, device), torch.full((5, 64), float("nan"), device=device))
    assert (a3 == -1).all() and torch.isneginf(s3).all()


# ---------------------------------------------------------------------------------------------- update
def _update_case(device, dim, lengths, nan_rows=0):
    nlist = len(lengths)
    cent = IC.orthonormal_centroids(3, nlist, dim)
    x, want = IC.rows_near(4, cent, lengths)
    if nan_rows:
        x = np.concatenate([x[:5], np.full((nan_rows, dim), np.nan, np.float32), x[5:]])
        want = np.concatenate([want[:5], np.full(nan_rows, -1), want[5:]])
    xt, ct = _dev(x, device), _dev(cent, device)
    assign, _ = R.ivf_assign(xt, ct)
    assert np.array_equal(assign.cpu().numpy(), want)                  # the device's own assignment is the built one
    return x, cent, xt, ct, assign


@pytest.mark.parametrize("dim, lengths, nan_rows", [
    (64, [0, 1, 511, 512, 513, 3 * 512 + 5, 7, 0], 0),
    (64, [3, 0, 513, 40], 2),                         # rows that belong to no list come first in the order
    (256, [0, 1, 513, 100], 0),
    (1024, [2, 0, 515], 0),
])
def test_update_matches_the_fp64_spherical_update(device, dim, lengths, nan_rows):
    assert R.ivf_chunk_rows() == 512
    x, cent, xt, ct, assign = _update_case(device, dim, lengths, nan_rows)
    order, offsets = R.ivf_group(assign, len(lengths))
    assert np.diff(offsets.cpu().numpy()).tolist() == lengths and int(offsets[0]) == nan_rows
    got = R.ivf_centroid_update(xt, order, offsets, ct)
    keep = np.nan_to_num(x.astype(np.float64))
    ref, m, S1, sn = IC.spherical_update_fp64(keep, assign.cpu().numpy(), cent)
    bound = IC.update_bound(m, dim, S1, sn)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref).max(1)
    print("update error / bound per list:", [f"{e:.2e}/{b:.2e}" for e, b in zip(err, bound)])
    assert (err <= bound).all()
    for l, length in enumerate(lengths):
        if length == 0:
            assert torch.equal(got[l], ct[l])                           # an empty list keeps its centroid
    assert (got.norm(dim=1) - 1).abs().max() < 1e-5
    # in place over the previous centroids
    same = ct.clone()
    ws = torch.empty(int(N.lib().vcap_ivf_centroid_update_workspace_bytes(xt.shape[0], len(lengths), dim)),
                     dtype=torch.uint8, device=device)
    N.check(N.lib().vcap_ivf_centroid_update(
        xt.data_ptr(), dim, xt.shape[0], dim, order.data_ptr(), offsets.data_ptr(), len(lengths), same.data_ptr(),
        same.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(device).cuda_stream), "update in place")
    assert torch.equal(same, got)


@pytest.mark.parametrize("dim", [64, 256, 1024])
def test_update_is_exact_on_integer_rows(device, dim):
    """Small-integer rows: every f32 sum is exact whatever its order, so each centroid must be vcap_l2_normalize
    of the exact member sum bit for bit - a lost row, chunk tail or chunk cannot hide inside a rounding bound.
    The sums a broken summation would give (IC.truncations) are shown to miss that equality."""
    C = R.ivf_chunk_rows()
    lengths = [0, 1, C - 1, C, C + 1, 3 * C + 5, 7, 0, 2 * C]
    nlist = len(lengths)
    x, assign = IC.integer_rows_case(dim, dim, lengths)
    xt, prev = _dev(x, device), _dev(IC.orthonormal_centroids(6, nlist, dim), device)
    order, offsets = R.ivf_group(torch.from_numpy(assign).to(device=device, dtype=torch.int32), nlist)
    assert np.diff(offsets.cpu().numpy()).tolist() == lengths
    got = R.ivf_centroid_update(xt, order, offsets, prev)
    sums = IC.member_sums(x, assign, nlist)
    assert np.abs(sums).max() < 2 ** 24 and (sums == np.round(sums)).all()
    want = R.l2_normalize(_dev(sums, device))
    for l, m in enumerate(lengths):
        assert torch.equal(got[l], want[l] if m else prev[l]), f"list {l} of {m} rows"
    for name, drop in IC.truncations(C).items():
        hit = [l for l, m in enumerate(lengths) if len(list(drop(l, m)))]
        bad = R.l2_normalize(_dev(IC.member_sums(x, assign, nlist, drop), device))
        assert hit and all(not torch.equal(bad[l], got[l]) for l in hit), name
        assert all(torch.equal(bad[l], got[l]) for l in range(nlist) if lengths[l] and l not in hit), name


def test_update_bits_depend_on_the_members_alone(device):
    lengths = [0, 1, 511, 512, 513, 3 * 512 + 5, 7, 0]
    x, cent, xt, ct, assign = _update_case(device, 64, lengths)
    order, offsets = R.ivf_group(assign, len(lengths))
    got = R.ivf_centroid_update(xt, order, offsets, ct)
    assert torch.equal(R.ivf_centroid_update(xt, order, offsets, ct), got)
    with _masked_stream(device):
        masked = R.ivf_centroid_update(xt, order, offsets, ct)
    assert torch.equal(masked, got)
    # the normalised sum is vcap_l2_normalize's arithmetic on the f32 sums (here: a list of one row)
    one = int(order[int(offsets[1])])
    assert torch.equal(got[1], R.l2_normalize(xt[one:one + 1].contiguous())[0])
    # other lists change (list 5 loses its rows, so every later offset moves): the rest keep their bits
    a2 = assign.clone()
    a2[assign == 5] = -1
    order2, offsets2 = R.ivf_group(a2, len(lengths))
    got2 = R.ivf_centroid_update(xt, order2, offsets2, ct)
    keep = [l for l in range(len(lengths)) if l != 5]
    assert torch.equal(got2[keep], got[keep]) and torch.equal(got2[5], ct[5])


# ---------------------------------------------------------------------------------------------- train
def test_train_is_seeded_and_its_objective_does_not_decrease(device):
    dim, nlist, niter = 64, 16, 6
    x, _ = IC.clustered_rows(5, 3000, dim, 24, spread=2.0)
    a = R.IVFFlatIPIndex(dim, nlist, device=device)
    a.train(x, niter=niter, seed=11)
    b = R.IVFFlatIPIndex(dim, nlist, device=device)
    b.train(x, niter=niter, seed=11)
    assert torch.equal(a.centroids, b.centroids) and a.train_objective == b.train_objective
    b.train(x, niter=niter, seed=12)
    assert not torch.equal(a.centroids, b.centroids)
    assert (a.centroids.norm(dim=1) - 1).abs().max() < 1e-5 and a.centroids.shape == (nlist, dim)
    # the same rounds from the public pieces, each step's allowed decrease derived from its own lists:
    # 2E (two f32 score evaluations) + the update's vector error 4 m u S1 / ||s|| + 4 (dim + 2) u
    xt, cent = a.training_set(x, seed=11)
    assert xt.shape[0] == 3000
    E = float(RC.error_bound(dim, 1 + 1e-6, 1 + 1e-6))
    objective, slack = [], []
    for _ in range(niter):
        assign, score = R.ivf_assign(xt, cent)
        objective.append(float(score.double().mean()))
        _, m, S1, sn = IC.spherical_update_fp64(x, assign.cpu().numpy(), cent.cpu().numpy())
        slack.append(2 * E + float(np.max(np.where(m > 0, 4 * m * IC.U32 * S1 / np.maximum(sn, 1e-30), 0)))
                     + 4 * (dim + 2) * IC.U32)
        order, offsets = R.ivf_group(assign, nlist)
        cent = R.ivf_centroid_update(xt, order, offsets, cent)
    assert torch.equal(cent, a.centroids)
    assert np.allclose(objective, a.train_objective, rtol=0, atol=1e-9)
    print("objective:", objective, "slack:", slack)
    for t in range(niter - 1):
        assert objective[t + 1] >= objective[t] - slack[t], (t, objective[t], objective[t + 1], slack[t])
    assert objective[-1] > objective[0]
    # a subsample: 2 points per centroid -> 32 rows, the same twice
    c = R.IVFFlatIPIndex(dim, nlist, device=device)
    rows, first = c.training_set(x, seed=3, max_points_per_centroid=2)
    rows2, first2 = c.training_set(x, seed=3, max_points_per_centroid=2)
    assert rows.shape == (32, dim) and torch.equal(rows, rows2) and torch.equal(first, first2)
    assert torch.unique(first, dim=0).shape[0] == nlist
    with pytest.raises(ValueError):
        R.IVFFlatIPIndex(dim, 64, device=device).train(x[:63])


# ---------------------------------------------------------------------------------------------- search
@lru_cache(maxsize=1)
def _rows(dim=64, n=3000):
    x, _ = IC.clustered_rows(21, n, dim, 40, spread=2.5)
    q, _ = IC.clustered_rows(22, 65, dim, 40, spread=2.5)
    return x, q


@lru_cache(maxsize=4)
def _trained(nlist, seed=5):
    """Centroids trained once per nlist (host copy), shared by the tests that need an index over _rows()."""
    x, _ = _rows()
    idx = R.IVFFlatIPIndex(x.shape[1], nlist, device="cuda:0")
    idx.train(x, niter=3, seed=seed)
    return idx.centroids.cpu().numpy()


def _index(device, nlist, storage, nprobe, x=None, pieces=None):
    x = _rows()[0] if x is None else x
    idx = R.IVFFlatIPIndex(x.shape[1], nlist, storage, device, nprobe=nprobe)
    idx.set_centroids(_trained(nlist))
    for a, b in pieces or [(0, len(x))]:
        idx.add(x[a:b])
    return idx


def _by_id(idx):
    """(stored rows as f32 numpy in id order, the list of every id)."""
    order = torch.argsort(idx.ids)
    lists = np.repeat(np.arange(idx.nlist), idx.list_sizes())
    return idx.vectors[order].float().cpu().numpy(), lists[order.cpu().numpy()]


SEARCH_SHAPES = [(3, 1, 1, 1), (3, 2, 5, 16), (16, 2, 5, 17), (16, 16, 128, 65), (50, 8, 128, 17), (50, 1, 5, 64),
                 (128, 8, 5, 65), (128, 128, 5, 16)]


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("nlist, nprobe, k, nq", SEARCH_SHAPES)
def test_search_is_exact_over_the_probed_lists(device, nlist, nprobe, k, nq, storage):
    x, q = _rows()
    q = q[:nq]
    idx = _index(device, nlist, storage, nprobe)
    assert idx.ntotal == len(x) and idx.list_sizes().sum() == len(x) and torch.equal(torch.sort(idx.ids).values,
                                                                                   torch.arange(len(x), device=device))
    probes = idx.probe_lists(q)
    assert probes.shape == (nq, nprobe) and probes.dtype == torch.int64
    Dc, Ic = _centroid_index(idx).search(q, nprobe)
    assert torch.equal(Ic, probes)
    RC.check_topk(Dc.cpu().numpy(), probes.cpu().numpy(), idx.centroids.cpu().numpy(), q, nprobe)
    D, I = idx.search(q, k)
    torch.cuda.synchronize()
    db, lists = _by_id(idx)
    assert np.array_equal(lists, R.ivf_assign(_dev(db, device), idx.centroids)[0].cpu().numpy())
    IC.check_probe_topk(D.cpu().numpy(), I.cpu().numpy(), db, lists, probes.cpu().numpy(), q, k)


def _centroid_index(idx):
    flat = R.FlatIPIndex(idx.dim, "f32", idx.device)
    flat.add(idx.centroids)
    return flat


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_list_lengths_around_the_tile_and_the_slice(device, storage):
    S = R.ivf_slice_rows()
    lengths = [0, 1, 15, 16, 17, S + 1, S - 1, S, 2 * S + 3, 40, 0, 5]
    cent = IC.orthonormal_centroids(9, len(lengths), 64)
    x, want = IC.rows_near(10, cent, lengths)
    idx = R.IVFFlatIPIndex(64, len(lengths), storage, device, nprobe=1)
    idx.set_centroids(cent)
    idx.add(x)
    assert idx.list_sizes().tolist() == lengths
    q, target = IC.rows_near(11, cent, [2] * len(lengths))
    probes = idx.probe_lists(q)
    assert probes[:, 0].tolist() == target.tolist()
    db, lists = _by_id(idx)
    assert np.array_equal(lists, want)
    for k in (1, 20, 128):
        D, I = idx.search(q, k)
        D, I = D.cpu().numpy(), I.cpu().numpy()
        IC.check_probe_topk(D, I, db, lists, probes.cpu().numpy(), q, k)
        for j, t in enumerate(target):        # k above the probed rows: the filler
            have = min(k, lengths[t])
            assert (I[j, :have] >= 0).all() and (I[j, have:] == -1).all() and np.isneginf(D[j, have:]).all()
    idx.nprobe = 3
    probes = idx.probe_lists(q)
    D, I = idx.search(q, 128)
    IC.check_probe_topk(D.cpu().numpy(), I.cpu().numpy(), db, lists, probes.cpu().numpy(), q, 128)
    idx.reset()
    assert idx.ntotal == 0 and idx.is_trained and (idx.search(q[:2], 3)[1] == -1).all()


def test_nprobe_above_nlist_clamps(device):
    x, q = _rows()
    idx = _index(device, 3, "f32", 500)
    assert idx.probe_lists(q[:4]).shape == (4, 3)
    flat = R.FlatIPIndex(64, "f32", device)
    flat.add(x)
    D, I = idx.search(q[:4], 10)
    Df, If = flat.search(q[:4], 10)
    assert torch.equal(I, If) and np.array_equal(_bits(D), _bits(Df))


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_exact_ids_when_the_winners_lie_in_a_probed_list(device, storage):
    dim, nq, k = 64, 4, 5
    db, q, win = RC.separated_case(31, 2000, dim, nq, k)
    stored = RC.bf16_round(db) if storage == "bf16" else db
    RC.assert_separated(stored, q, k, win)                               # input check, on the CPU restatement
    rest = RC.orthonormal_queries(np.random.default_rng(32), 8, dim)[4:]
    rest = IC.unit(rest - (rest @ q.T.astype(np.float64)) @ q)
    idx = R.IVFFlatIPIndex(dim, 8, storage, device, nprobe=2)
    idx.set_centroids(np.concatenate([q, rest]).astype(np.float32))      # list j is built around query j
    idx.add(db)
    probes = idx.probe_lists(q).cpu().numpy()
    _, lists = _by_id(idx)
    for j in range(nq):
        assert probes[j, 0] == j and np.isin(lists[win[j, :k]], probes[j]).all()     # the winners are probed
    D, I = idx.search(q, k)
    assert np.array_equal(I.cpu().numpy(), win[:, :k])
    assert np.array_equal(I.cpu().numpy(), RC.flat_ip_reference(stored, q, k)[1])


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("nlist", [3, 50, 128])
def test_probing_every_list_is_the_flat_search_bit_for_bit(device, nlist, storage):
    x, q = _rows()
    idx = _index(device, nlist, storage, nlist)
    flat = R.FlatIPIndex(64, storage, device)
    flat.add(x)
    for k, nq in ((100, 17), (1, 65), (128, 1)):
        D, I = idx.search(q[:nq], k)
        Df, If = flat.search(q[:nq], k)
        assert torch.equal(I, If) and np.array_equal(_bits(D), _bits(Df))


def test_flat_equivalence_at_dim_256_and_1024_with_normalisation(device):
    for dim, n in ((256, 1500), (1024, 700)):
        x, _ = IC.clustered_rows(41, n, dim, 12, spread=2.0)
        x = x * np.linspace(0.5, 2.0, n, dtype=np.float32)[:, None]
        for storage in ("f32", "bf16"):
            idx = R.IVFFlatIPIndex(dim, 7, storage, device, normalize=True, nprobe=7)
            idx.train(x, niter=2)
            idx.add(x)
            flat = R.FlatIPIndex(dim, storage, device, normalize=True)
            flat.add(x)
            D, I = idx.search(x[:20], 10)
            Df, If = flat.search(x[:20], 10)
            assert torch.equal(I, If) and np.array_equal(_bits(D), _bits(Df))


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_results_are_a_function_of_the_rows_alone(device, storage):
    """One add or several, max_blocks 0 / 32, a CU-masked stream, queries alone or batched, a repeat: the same bits."""
    x, q = _rows()
    k = 50
    one = _index(device, 16, storage, 4)
    D, I = one.search(q, k)
    D2, I2 = one.search(q, k)
    assert torch.equal(I, I2) and np.array_equal(_bits(D), _bits(D2))
    parts = _index(device, 16, storage, 4, pieces=[(0, 1), (1, 700), (700, 701), (701, 3000)])
    assert torch.equal(parts.vectors.view(torch.uint8), one.vectors.view(torch.uint8)) and torch.equal(parts.ids, one.ids)
    Dp, Ip = parts.search(q, k)
    assert torch.equal(I, Ip) and np.array_equal(_bits(D), _bits(Dp))
    D32, I32 = one.search(q, k, max_blocks=32)
    assert torch.equal(I, I32) and np.array_equal(_bits(D), _bits(D32))
    for j in (0, 15, 16, 63, 64):
        D1, I1 = one.search(q[j:j + 1], k)
        assert torch.equal(I1[0], I[j]) and np.array_equal(_bits(D1[0]), _bits(D[j]))
    with _masked_stream(device):
        Dm, Im = one.search(q, k)
    assert torch.equal(I, Im) and np.array_equal(_bits(D), _bits(Dm))


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_every_stored_vector_finds_itself_first(device, storage):
    x, _ = IC.clustered_rows(51, 600, 64, 20, spread=2.0)
    idx = R.IVFFlatIPIndex(64, 16, storage, device, nprobe=1)
    idx.train(x, niter=3)
    idx.add(x)
    db, lists = _by_id(idx)                                              # the rows as stored, in id order
    S = RC.scores_fp64(db, db)
    E = float(RC.error_bound(64, np.linalg.norm(db, axis=1).max(), np.linalg.norm(db, axis=1).max()))
    off = S - np.diag(np.full(len(db), np.inf))
    assert (np.diag(S) - off.max(1) > 4 * E).all()                       # input check: every row beats every other by > 4E
    assert np.array_equal(idx.probe_lists(db)[:, 0].cpu().numpy(), lists)   # a stored vector probes its own list first
    D, I = idx.search(db, 1)
    assert np.array_equal(I[:, 0].cpu().numpy(), np.arange(len(db)))
    assert (np.abs(D[:, 0].cpu().numpy() - np.diag(S)) <= E).all()


# ---------------------------------------------------------------------------------------------- persistence, scripts
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_save_and_load_index_give_the_same_bits(device, storage, tmp_path):
    x, q = _rows()
    idx = _index(device, 16, storage, 3)
    idx.metadata = [{"video_id": f"v{i}", "caption": f"c{i}"} for i in range(len(x))]
    D, I = idx.search(q, 10)
    idx.save(tmp_path / "ivf")
    back = R.load_index(tmp_path / "ivf", device)
    assert isinstance(back, R.IVFFlatIPIndex) and (back.ntotal, back.nlist, back.nprobe) == (len(x), 16, 3)
    assert torch.equal(back.vectors.view(torch.uint8), idx.vectors.view(torch.uint8)) and back.metadata[5] == idx.metadata[5]
    Db, Ib = back.search(q, 10)
    assert torch.equal(I, Ib) and np.array_equal(_bits(D), _bits(Db))
    back.add(x[:10])                                                     # a loaded index keeps growing
    assert back.ntotal == len(x) + 10 and int(back.ids.max()) == len(x) + 9
    flat = R.FlatIPIndex(64, storage, device)
    flat.add(x)
    flat.save(tmp_path / "flat")
    assert isinstance(R.load_index(tmp_path / "flat", device), R.FlatIPIndex)


def test_scripts_build_and_query_an_ivf_index(device, tmp_path, capsys):
    from scripts import build_index, build_index_with_captions, extract_features, query_video
    from test_gpu_retrieval import _clips
    anns, ann_path = _clips(tmp_path)
    model = ["--weights_seed", "3", "--precision", "fp32", "--device", str(device), "--vit_name", "vit_tiny_test"]
    ivf, flat = tmp_path / "ivf", tmp_path / "flat"
    common = ["--ann_path", str(ann_path), "--num_frame", "8", "--image_size", "224"] + model
    assert build_index_with_captions.main(common + ["--out_dir", str(ivf), "--index_type", "IVF_FLAT", "--nlist", "2"]) == 5
    assert build_index_with_captions.main(common + ["--out_dir", str(flat)]) == 5
    info = json.loads((ivf / "index.json").read_text())
    assert (info["type"], info["nlist"], info["nprobe"], info["ntotal"]) == ("IVF_FLAT", 2, 1, 5)
    assert "type" not in json.loads((flat / "index.json").read_text())
    meta = json.loads((ivf / "meta.json").read_text("utf-8"))
    assert meta == [{"video_id": a["video_id"], "caption": a["captions"][0]} for a in anns]
    assert meta == json.loads((flat / "meta.json").read_text("utf-8"))
    for c, a in enumerate(anns):
        out = []
        for d, extra in ((ivf, ["--nprobe", "2"]), (flat, [])):
            capsys.readouterr()
            res = query_video.main(["--frames_dir", a["frames_dir"], "--k", "5", "--index", str(d)] + extra + model)
            out.append((res, [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[") and "score=" in ln]))
        assert out[0] == out[1] and len(out[0][1]) == 5 and out[0][0][0][0] == c
    # the feature-file route: build_index --index_type IVF_FLAT
    feats = tmp_path / "features"
    assert extract_features.main(["--annotations", str(ann_path), "--out_dir", str(feats)] + model) == 5
    assert build_index.main(["--features", str(feats), "--annotations", str(ann_path), "--out_dir", str(tmp_path / "ivf2"),
                             "--device", str(device), "--index_type", "IVF_FLAT", "--nlist", "2"]) == 5
    assert isinstance(R.load_index(tmp_path / "ivf2", device), R.IVFFlatIPIndex)
