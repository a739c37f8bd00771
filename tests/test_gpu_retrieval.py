"""Video retrieval on the GPU: vcap_ip_search against the fp64 restatement (tests/retrieval_cases.py) at the
smallest shapes that reach every mechanism (slab and workgroup boundaries, every query-tile count, k up to
128, k > n), its determinism contract, 64-bit offsets, vcap_l2_normalize and vcap_ip_index_convert against
torch, FlatIPIndex chunking / growth / persistence, HipVideoEmbedder against the reference's recorded
encoder outputs, and the four scripts end to end on synthetic JPEG frame directories.

Error bound (derived in retrieval_cases.py): |s - s*| <= 2 * dim * 2^-24 * ||q|| ||x|| = E; a returned top-k
is valid when every returned row is within 2E of the k-th best fp64 score, no better row was left out,
every returned score is within E of its row's, and the order is (score desc, id asc).  Exact id equality is
asserted on inputs whose fp64 gaps were first checked to exceed 4E."""
import ctypes as C
import json
from functools import lru_cache

import numpy as np
import pytest
import torch

import retrieval_cases as RC
from helpers import case
from vcap import _native as N
from vcap import retrieval as R

pytestmark = pytest.mark.gpu


def _search(db, n, q, k, device, storage="f32", **kw):
    """(D, I) numpy of one vcap_ip_search call over host f32 rows stored as `storage`."""
    t = torch.from_numpy(np.ascontiguousarray(db, np.float32)).to(device)
    if storage == "bf16":
        t = t.to(torch.bfloat16)
    if t.shape[0] == 0:
        t = torch.zeros(1, q.shape[1], dtype=t.dtype, device=device)
    D, I = R.ip_search(t.contiguous(), n, torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(device), k, **kw)
    torch.cuda.synchronize()
    return D.cpu().numpy(), I.cpu().numpy()


def _stored(db, storage):
    return RC.bf16_round(db) if storage == "bf16" else db


# n as a function of (slab rows S, default scan grid G); max_blocks; which rows carry query 0's winners
SHAPES = {
    # n around the slab at dim 256 (one query tile), k = 5
    "n0": (lambda S, G: 0, 256, 3, 5, 0, None),
    "n1": (lambda S, G: 1, 256, 3, 5, 0, None),
    "n_k-1": (lambda S, G: 4, 256, 3, 5, 0, None),
    "slab-1": (lambda S, G: S - 1, 256, 3, 5, 0, None),
    "slab": (lambda S, G: S, 256, 3, 5, 0, "edges"),
    "slab+1": (lambda S, G: S + 1, 256, 3, 5, 0, "edges"),
    "n70001": (lambda S, G: 70001, 256, 3, 5, 0, "edges"),
    # k
    "k1": (lambda S, G: S + 1, 256, 3, 1, 0, "edges"),
    "k100_nq16": (lambda S, G: 70001, 256, 16, 100, 0, "edges"),
    "k128_nq1": (lambda S, G: 70001, 256, 1, 128, 0, "edges"),
    "k>n": (lambda S, G: 50, 256, 3, 100, 0, None),
    # dim and query tiles
    "dim64": (lambda S, G: 2 * S + 1, 64, 3, 5, 0, "edges"),
    "dim64_nq48_k100": (lambda S, G: 30011, 64, 48, 100, 0, None),
    "dim768": (lambda S, G: 4097, 768, 3, 5, 0, "edges"),
    "dim768_nq21_two_passes": (lambda S, G: 4097, 768, 21, 5, 0, None),
    "dim1024_nq16": (lambda S, G: 4097, 1024, 16, 5, 0, "edges"),
    "dim256_nq64": (lambda S, G: 9001, 256, 64, 5, 0, None),
    "dim256_nq33": (lambda S, G: 9001, 256, 33, 5, 0, None),
    # more slabs than workgroups: every workgroup takes >= 2
    "2slabs_per_wg": (lambda S, G: 2 * G * S + 77, 64, 3, 5, 0, "edges"),
    "2slabs_per_wg_mb8": (lambda S, G: 2 * 8 * S + 5, 256, 3, 5, 8, "edges"),
    # all winners inside one workgroup's slab: the merge takes a whole list from one producer
    "one_slab_holds_all": (lambda S, G: 20 * S, 256, 1, 5, 4, "slab3"),
}


@lru_cache(maxsize=2)
def _case(name):
    nfn, dim, nq, k, mb, plant = SHAPES[name]
    S, G = R.slab_rows(), R.scan_workgroups(10 ** 9, 0)
    n = nfn(S, G)
    w = min(2 * k, n // nq)
    positions = None
    if plant and w:
        rng = np.random.default_rng(99)
        if plant == "edges":      # query 0: first row, last row, last row of a slab (first and last slab)
            first = [r for r in dict.fromkeys([0, n - 1, S - 1, (n // S) * S - 1]) if 0 <= r < n][:w]
        else:                     # every winner of the only query inside slab 3
            first = list(range(3 * S + 7, 3 * S + 7 + w))
        rest = np.setdiff1d(np.arange(n), first)
        rest = rng.permutation(rest)[:nq * w - len(first)]
        positions = np.concatenate([np.array(first, np.int64), rest]).reshape(nq, w)
    db, q, win = RC.separated_case(11, n, dim, nq, k, positions)
    return n, dim, nq, k, mb, db, q, win


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_search_matches_the_fp64_restatement(device, name, storage):
    n, dim, nq, k, mb, db, q, win = _case(name)
    ref_db = _stored(db, storage)
    D, I = _search(db, n, q, k, device, storage, max_blocks=mb)
    RC.check_topk(D, I, ref_db, q, k)
    if win.shape[1] >= k:
        RC.assert_separated(ref_db, q, k, win)                      # input check, on the CPU restatement
        assert np.array_equal(I, RC.flat_ip_reference(ref_db, q, k)[1])
        assert np.array_equal(I, win[:, :k])


def test_short_list_filler(device):
    n, dim, nq, k, mb, db, q, win = _case("k>n")
    D, I = _search(db, n, q, k, device)
    assert (I[:, n:] == -1).all() and np.isneginf(D[:, n:]).all() and (I[:, :n] >= 0).all()
    D0, I0 = _search(db, 0, q, 3, device)
    assert (I0 == -1).all() and np.isneginf(D0).all()


def test_nan_rows_are_never_returned(device):
    n, dim, nq, k, mb, db, q, win = _case("slab+1")
    db = db.copy()
    bad = [int(win[0, 0]), 5, n - 1]
    db[bad[0], 3] = np.nan
    db[bad[1]] = np.nan
    db[bad[2], dim - 1] = np.nan
    for storage in ("f32", "bf16"):
        D, I = _search(db, n, q, 128, device, storage)
        assert not np.isin(I, bad).any() and not np.isnan(D).any()
        assert (I[:, :n - 3] >= 0).all() and (I[:, n - 3:] == -1).all()      # 129 rows, 3 of them NaN
        RC.check_topk(D, I, _stored(db, storage), q, 128)


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_results_are_a_function_of_the_rows_alone(device, storage):
    """Row determinism + total order: the same bits from a permuted database (ids permuted with it), from
    max_blocks 0 and 32, from a CU-masked stream, from nq = 1 calls against an nq = 16 call, and from a repeat."""
    n, dim, nq, k, mb, db, q, win = _case("k100_nq16")
    D, I = _search(db, n, q, k, device, storage)
    D2, I2 = _search(db, n, q, k, device, storage)
    assert np.array_equal(D.view(np.uint32), D2.view(np.uint32)) and np.array_equal(I, I2)
    D32, I32 = _search(db, n, q, k, device, storage, max_blocks=32)
    assert np.array_equal(D.view(np.uint32), D32.view(np.uint32)) and np.array_equal(I, I32)
    perm = np.random.default_rng(3).permutation(n)
    Dp, Ip = _search(db[perm], n, q, k, device, storage)
    assert np.array_equal(D.view(np.uint32), Dp.view(np.uint32)) and np.array_equal(I, perm[Ip])
    for j in (0, 7, 15):
        D1, I1 = _search(db, n, q[j:j + 1], k, device, storage)
        assert np.array_equal(D[j].view(np.uint32), D1[0].view(np.uint32)) and np.array_equal(I[j], I1[0])
    h = C.c_void_p()
    N.check(N.lib().vcap_stream_create_cu_reserved(32, C.byref(h)), "masked stream")
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.ExternalStream(h.value, device=device)):
            Dm, Im = _search(db, n, q, k, device, storage)
    finally:
        torch.cuda.synchronize()
        N.check(N.lib().vcap_stream_destroy(h), "stream destroy")
    assert np.array_equal(D.view(np.uint32), Dm.view(np.uint32)) and np.array_equal(I, Im)


def test_exact_ties_come_back_by_ascending_id(device):
    """Every row stored twice (ids i and i + n): each pair ties exactly and comes back lower id first."""
    n, dim, nq, k, mb, db, q, win = _case("slab+1")
    dup = np.concatenate([db, db])
    for storage in ("f32", "bf16"):
        D, I = _search(dup, 2 * n, q, 12, device, storage)
        RC.check_topk(D, I, _stored(dup, storage), q, 12)
        assert np.array_equal(I, RC.flat_ip_reference(_stored(dup, storage), q, 12)[1])
        assert np.array_equal(I[:, 0::2], win[:, :6]) and np.array_equal(I[:, 1::2], win[:, :6] + n)
        assert np.array_equal(D[:, 0::2].view(np.uint32), D[:, 1::2].view(np.uint32))


def test_offsets_past_2_to_the_31(device):
    """bf16 rows, dim 1024, n = 2^21 + 5 (4.3 GB; element offsets pass 2^31).  Background rows have norm about
    0.1 (asserted < 0.15), so by Cauchy-Schwarz none scores above 0.15 against a unit query; unit winners
    scoring 0.9 / 0.8 / 0.7 sit in the last five rows."""
    dim, n = 1024, (1 << 21) + 5
    g = torch.Generator(device=device).manual_seed(5)
    db = torch.empty(n, dim, dtype=torch.bfloat16, device=device)
    step = 1 << 18
    top = 0.0
    for s in range(0, n, step):
        blk = torch.randn(min(step, n - s), dim, generator=g, device=device) * (0.1 / 32.0)
        db[s:s + step] = blk.to(torch.bfloat16)
        top = max(top, float(db[s:s + step].float().norm(dim=1).max()))
        del blk
    assert top < 0.15
    rng = np.random.default_rng(8)
    Q = RC.orthonormal_queries(rng, 2, dim)
    q = Q[:1].astype(np.float32)
    rows, alpha = [n - 1, n - 3, n - 5], [0.9, 0.8, 0.7]
    plant = np.stack([a * Q[0] + np.sqrt(1 - a * a) * Q[1] for a in alpha]).astype(np.float32)
    db[rows] = torch.from_numpy(plant).to(device).to(torch.bfloat16)
    D, I = R.ip_search(db, n, torch.from_numpy(q).to(device), 5)
    torch.cuda.synchronize()
    D, I = D.cpu().numpy(), I.cpu().numpy()
    del db
    torch.cuda.empty_cache()
    assert I[0, :3].tolist() == rows
    s_star = RC.scores_fp64(RC.bf16_round(plant), q)[0]
    E = RC.error_bound(dim, np.linalg.norm(q), np.linalg.norm(RC.bf16_round(plant).astype(np.float64), axis=1))
    assert (np.abs(D[0, :3] - s_star) <= E).all()
    assert (I[0, 3:] >= 0).all() and (D[0, 3:] < 0.15).all() and (np.diff(D[0]) <= 0).all()


def _ulp_diff(a: torch.Tensor, b: torch.Tensor) -> int:
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a) - key(b)).abs().max()) if a.numel() else 0


@pytest.mark.parametrize("mode, eps", [(0, 1e-12), (1, 1e-8)])
def test_l2_normalize_matches_torch(device, mode, eps):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(37, 256, generator=g)
    x[3] = 0.0                                   # zero row
    x[5] *= 1e-20                                # the eps path
    x[7] *= 1e4
    x = x.to(device)

    def ref(t):
        nrm = t.norm(dim=1, keepdim=True)
        return t / nrm.clamp_min(eps) if mode == 0 else t / (nrm + eps)

    want = torch.nn.functional.normalize(x, dim=1, eps=eps) if mode == 0 else ref(x)
    got = R.l2_normalize(x, eps, mode)
    assert _ulp_diff(got, want) <= 2
    assert torch.equal(got[3], torch.zeros(256, device=device))
    # a row's result does not depend on the number of rows
    assert torch.equal(R.l2_normalize(x[6:9].contiguous(), eps, mode), got[6:9])
    # in place
    y = x.clone()
    assert R.l2_normalize(y, eps, mode, out=y) is y and torch.equal(y, got)
    # strided rows (ldx > dim), other dims
    for dim in (64, 100, 768):
        wide = torch.randn(9, dim + 24, generator=g).to(device)
        view = wide[:, :dim]
        assert _ulp_diff(R.l2_normalize(view, eps, mode), ref(view)) <= 2


def test_index_convert_is_torchs_bf16_rounding(device):
    bits = [0x3F800000, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F80FFFF,     # ties to even, both sides
            0x7F7FFFFF, 0xFF7FFFFF,                                                     # rounds to +-inf
            0x7F800000, 0xFF800000, 0x00000000, 0x80000000,                             # +-inf, +-0
            0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80008001,                 # subnormals
            0x7FC00000, 0x7F800001, 0xFFC00001]                                         # NaNs
    g = np.random.default_rng(4)
    x = np.concatenate([np.array(bits, np.uint32), g.integers(0, 1 << 32, 64 * 5 - len(bits), dtype=np.uint64)
                        .astype(np.uint32)]).view(np.float32).reshape(5, 64)
    xt = torch.from_numpy(x).to(device)
    for storage, tdt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        idx = R.FlatIPIndex(64, storage, device)
        idx.add(xt)
        want = xt.to(tdt)
        raw = torch.int16 if storage == "bf16" else torch.int32
        assert torch.equal(idx.vectors.view(raw), want.view(raw))
    wide = torch.randn(6, 256 + 64, device=device)      # strided source rows
    dst = torch.empty(6, 256, dtype=torch.bfloat16, device=device)
    N.check(N.lib().vcap_ip_index_convert(wide.data_ptr(), wide.stride(0), 6, 256, N.DT_BF16, dst.data_ptr(), 0), "convert")
    torch.cuda.synchronize()
    assert torch.equal(dst, wide[:, :256].to(torch.bfloat16))


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_index_chunks_grows_and_persists(device, storage, tmp_path):
    rng = np.random.default_rng(6)
    x = rng.standard_normal((1000, 256)).astype(np.float32)
    q = rng.standard_normal((200, 256)).astype(np.float32)
    one = R.FlatIPIndex(256, storage, device, normalize=True)
    one.add(x)
    pieces = R.FlatIPIndex(256, storage, device, normalize=True)
    for a, b in ((0, 1), (1, 70), (70, 71), (71, 640), (640, 1000)):
        pieces.add(torch.from_numpy(x[a:b]))
    assert one.ntotal == pieces.ntotal == 1000 and torch.equal(one.vectors.view(torch.uint8),
                                                               pieces.vectors.view(torch.uint8))
    assert (one.vectors.float().norm(dim=1) - 1).abs().max() < (1e-2 if storage == "bf16" else 1e-6)
    D, I = one.search(q, 10)                     # numpy queries, nq = 200: four kernel calls
    assert D.shape == (200, 10) and D.device == torch.device(device) and I.dtype == torch.int64
    for j in (0, 63, 64, 127, 128, 199):
        d, i = one.search(torch.from_numpy(q[j]).to(device), 10)
        assert torch.equal(d[0], D[j]) and torch.equal(i[0], I[j])
    RC.check_topk(D.cpu().numpy(), I.cpu().numpy(), one.vectors.float().cpu().numpy(), q, 10)
    one.metadata = [{"video_id": f"v{i}", "caption": f"c{i}"} for i in range(1000)]
    one.save(tmp_path / "idx")
    back = R.FlatIPIndex.load(tmp_path / "idx", device)
    assert (back.ntotal, back.storage, back.normalize, back.metadata[7]) == (1000, storage, True, one.metadata[7])
    assert torch.equal(back.vectors.view(torch.uint8), one.vectors.view(torch.uint8))
    Db, Ib = back.search(q[:5], 10)
    assert torch.equal(Db, D[:5]) and torch.equal(Ib, I[:5])
    one.reset()
    assert one.ntotal == 0 and (one.search(q[:2], 3)[1] == -1).all()


# ---------------------------------------------------------------------------- against the reference's numbers
BF16_ENCODER_TOL = 3e-2      # test_gpu_parity.py::test_bf16_encoder_close


@pytest.mark.parametrize("name", ["b16_b2", "b16_b8"])
def test_embedder_fp32_matches_the_normalised_reference_output(device, name):
    meta, g, va, ga, sd, frames = case(name)
    ref = torch.from_numpy(g["encoder_out"])
    assert float(ref.norm(dim=1).min()) > 0.1
    want = torch.nn.functional.normalize(ref, dim=1).numpy()
    emb = R.HipVideoEmbedder.from_state_dict(sd, va, "fp32", device)
    got = emb.encode_video(torch.from_numpy(frames).to(device))
    torch.cuda.synchronize()
    assert got.shape == (meta["B"], 256)
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=1e-4)


def test_embedder_bf16_and_the_alignment_layout(device):
    meta, g, va, ga, sd, frames = case("b16_b8")
    ref = torch.from_numpy(g["encoder_out"])
    nmin = float(ref.norm(dim=1).min())
    assert nmin > 0.1
    want = torch.nn.functional.normalize(ref, dim=1).numpy()
    align = {"model_state": {("vit." + k[len("encoder.backbone."):] if k.startswith("encoder.backbone.") else
                              "vid_proj." + k[len("encoder.proj."):]): v
                             for k, v in sd.items() if k.startswith("encoder.")}}
    align["model_state"]["txt_proj.weight"] = np.zeros((4, 4), np.float32)
    video = torch.from_numpy(frames).to(device)
    got = R.HipVideoEmbedder.from_state_dict(align, va, "bf16", device).encode_video(video)
    same = R.HipVideoEmbedder.from_state_dict(sd, va, "bf16", device).encode_video(video)
    torch.cuda.synchronize()
    assert torch.equal(got, same)
    assert np.abs(got.cpu().numpy() - want).max() <= BF16_ENCODER_TOL / nmin
    assert (got.norm(dim=1) - 1).abs().max() < 1e-5


# ---------------------------------------------------------------------------- end to end
def _clips(tmp_path, count=5, frames=10, h=120, w=160):
    """Seeded synthetic clips as frames_dir/frame_*.jpg (the layout tests/test_gpu_cli.py writes)."""
    from PIL import Image
    anns = []
    for c in range(count):
        d = tmp_path / f"clip{c}"
        d.mkdir()
        g = np.random.default_rng(100 + c)
        base = g.integers(0, 256, (h // 8, w // 8, 3), dtype=np.uint8)
        for i in range(frames):
            img = np.kron(np.roll(base, i, axis=1), np.ones((8, 8, 1), dtype=np.uint8))
            img = np.clip(img.astype(np.int16) + g.integers(-8, 9, img.shape), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(d / f"frame_{i:06d}.jpg", quality=90)
        anns.append({"video_id": f"vid{c}", "frames_dir": str(d), "captions": [f"caption of clip {c}", "another"]})
    path = tmp_path / "annotations.json"
    path.write_text(json.dumps(anns))
    return anns, path


def test_scripts_end_to_end(device, tmp_path, capsys):
    import re

    from scripts import build_index, eval_retrieval, extract_features, query_video
    anns, ann_path = _clips(tmp_path)
    model = ["--weights_seed", "3", "--precision", "fp32", "--device", str(device), "--vit_name", "vit_tiny_test"]
    feats, idx = tmp_path / "features", tmp_path / "index"
    assert extract_features.main(["--annotations", str(ann_path), "--out_dir", str(feats)] + model) == len(anns)
    f0 = np.load(feats / "vid0.npy")
    assert f0.shape == (256,) and f0.dtype == np.float32 and abs(float(np.linalg.norm(f0)) - 1) < 1e-5
    assert build_index.main(["--features", str(feats), "--annotations", str(ann_path), "--out_dir", str(idx),
                             "--device", str(device)]) == len(anns)
    meta = json.loads((idx / "meta.json").read_text("utf-8"))
    assert meta == [{"video_id": a["video_id"], "caption": a["captions"][0]} for a in anns]
    E = float(RC.error_bound(256, 1.0 + 1e-5, 1.0 + 1e-5))
    for c, a in enumerate(anns):
        capsys.readouterr()
        res = query_video.main(["--frames_dir", a["frames_dir"], "--k", "5", "--index", str(idx)] + model)
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[") and "score=" in ln]
        assert res[0][0] == c and abs(res[0][1] - 1.0) <= E + 1e-6, res      # 1e-6: the unit norms' own rounding
        assert len(lines) == 5
        for rank, (ln, (i, s)) in enumerate(zip(lines, res), start=1):
            assert ln == f"[{rank}] score={s:.4f} | id={meta[i]['video_id']} | caption={meta[i]['caption']}"
            assert re.fullmatch(r"\[\d+\] score=-?\d+\.\d{4} \| id=\S+ \| caption=.*", ln)
    capsys.readouterr()
    m = eval_retrieval.main(["--annotations", str(ann_path), "--index", str(idx)] + model)
    out = capsys.readouterr().out
    assert m["recall@1"] == m["recall@5"] == m["mrr"] == 1.0 and m["n"] == len(anns)
    assert "[VAL] N=5" in out and "Recall@1: 1.000" in out and "Recall@5: 1.000" in out and "MRR: 1.000" in out
    with pytest.raises(SystemExit, match="--video needs a frame extractor"):
        query_video.main(["--video", str(tmp_path / "clip.mp4"), "--index", str(idx)] + model)
