"""CPU suite of the IVF-Flat index: the fp64 restatement of the probe search against plain Python loops, the
fp64 spherical update and its bound, the new ABI symbols (header, binding, exports; ABI still 16), every
argument refusal of the new entry points (returned before any launch: the library loads without a GPU), the
pinned workspace sizes, load_index over both directory layouts, and the scripts' argument parsing."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

import ivf_cases as IC
import retrieval_cases as RC
from vcap import _native as N

ROOT = Path(__file__).resolve().parents[1]
ARG, WS, UNSUP = N.E_ARG, N.E_WORKSPACE, N.E_UNSUPPORTED
NEW_SYMBOLS = ("vcap_ivf_assign", "vcap_ivf_centroid_update", "vcap_ivf_centroid_update_workspace_bytes",
               "vcap_ivf_search", "vcap_ivf_search_workspace_bytes", "vcap_ivf_slice_rows", "vcap_ivf_chunk_rows")

_BUF = C.create_string_buffer(4096)
P = (C.addressof(_BUF) + 255) & ~255      # a non-null, aligned address no refused call reads


# ---------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("seed, n, dim, nlist, nprobe, nq, k", [(0, 9, 4, 3, 1, 2, 3), (1, 12, 8, 4, 2, 3, 5),
                                                                 (2, 6, 4, 3, 3, 1, 8), (3, 5, 4, 4, 2, 2, 2)])
def test_restatement_matches_plain_loops(seed, n, dim, nlist, nprobe, nq, k):
    rng = np.random.default_rng(seed)
    db = rng.integers(-3, 4, (n, dim)).astype(np.float32)     # small integers: exact sums, many ties
    q = rng.integers(-3, 4, (nq, dim)).astype(np.float32)
    assign = rng.integers(0, nlist, n)
    probes = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)])
    D, I = IC.probe_search_reference(db, assign, probes, q, k)
    Dl, Il = IC.probe_search_loops(db, assign, probes, q, k)
    assert np.array_equal(I, Il) and np.array_equal(D, Dl)
    IC.check_probe_topk(D, I, db, assign, probes, q, k)
    if nprobe == nlist:                                       # every list probed: the flat search
        Df, If = RC.flat_ip_reference(db, q, k)
        assert np.array_equal(I, If) and np.array_equal(D, Df)


def test_restatement_skips_filler_probes_and_unprobed_rows():
    db = np.array([[3, 0], [2, 0], [1, 0], [np.nan, 0], [5, 0]], np.float32)
    assign = np.array([0, 1, 1, 1, 2])
    q = np.array([[1, 0]], np.float32)
    D, I = IC.probe_search_reference(db, assign, np.array([[1, -1]]), q, 4)
    assert I.tolist() == [[1, 2, -1, -1]] and D.tolist() == [[2, 1, -np.inf, -np.inf]]
    IC.check_probe_topk(D, I, db, assign, np.array([[1, -1]]), q, 4)
    with pytest.raises(AssertionError):                       # id 4 lies in list 2, which is not probed
        IC.check_probe_topk(np.array([[5.0, 2, 1, -np.inf]]), np.array([[4, 1, 2, -1]]), db, assign, np.array([[1, -1]]), q, 4)
    with pytest.raises(AssertionError):                       # the best probed row left out
        IC.check_probe_topk(np.array([[1.0, -np.inf]]), np.array([[2, -1]]), db, assign, np.array([[1, -1]]), q, 2)


def test_assign_reference_ties_and_nan():
    cent = np.array([[1, 0], [1, 0], [np.nan, 0], [0, 1]], np.float32)
    x = np.array([[2, 0], [0, 3], [-1, -1]], np.float32)
    assert IC.assign_reference(x, cent).tolist() == [0, 3, 0]
    assert IC.assign_reference(x, np.full((2, 2), np.nan)).tolist() == [-1, -1, -1]


def test_spherical_update_and_its_bound():
    x = np.array([[1, 0], [0, 1], [3, 4], [0, 2], [7, 7]], np.float64)
    prev = np.array([[1, 0], [0, 1], [0.6, 0.8]])
    c, m, S1, sn = IC.spherical_update_fp64(x, [0, 0, 2, 2, -1], prev)
    assert np.allclose(c[0], [2 ** -0.5, 2 ** -0.5]) and np.array_equal(c[1], prev[1])      # list 1 is empty
    assert np.allclose(c[2], np.array([3, 6]) / np.sqrt(45)) and m.tolist() == [2, 0, 2]
    assert np.allclose(S1, [2, 0, 7]) and np.allclose(sn, [np.sqrt(2), 0, np.sqrt(45)])
    b = IC.update_bound(m, 2, S1, sn)
    assert b[1] == 0 and b[0] == pytest.approx(4 * 2 * 2.0 ** -24 * 2 / np.sqrt(2) + 2 * 4 * 2.0 ** -24)
    # an f32 sum of 512 unit rows at dim 256 against the fp64 one stays inside the bound
    rows, _ = IC.clustered_rows(0, 512, 256, 1)
    s32 = np.zeros(256, np.float32)
    for r in rows:
        s32 = s32 + r
    c32 = s32 / np.sqrt(np.float32((s32 * s32).sum(dtype=np.float32)))
    c64, m, S1, sn = IC.spherical_update_fp64(rows, np.zeros(512, int), np.zeros((1, 256)))
    assert (np.abs(c32 - c64[0]) <= IC.update_bound(m, 256, S1, sn)[0]).all()


def test_integer_rows_expose_every_truncated_sum():
    """The exact-sum case of the GPU suite, replayed on the CPU: f32 sums of the integer rows are exact in any
    order, and each summation error the chunk-boundary lengths exist to catch (a lost row, chunk tail or chunk)
    moves the normalised centroid by far more than any f32 rounding, so bit equality with the exact sum fails."""
    chunk = 512
    lengths = [0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 7, 0, 2 * chunk]
    x, assign = IC.integer_rows_case(64, 64, lengths)
    assert np.bincount(assign, minlength=len(lengths)).tolist() == lengths and (np.abs(x).sum(1) > 0).all()
    full = IC.member_sums(x, assign, len(lengths))
    fwd, rev = np.zeros_like(full, dtype=np.float32), np.zeros_like(full, dtype=np.float32)
    for i in range(len(x)):                                   # two f32 summation orders: both exact
        fwd[assign[i]] += x[i]
        rev[assign[-1 - i]] += x[-1 - i]
    assert np.array_equal(fwd, full) and np.array_equal(rev, full)
    filled = [l for l, m in enumerate(lengths) if m]
    for name, drop in IC.truncations(chunk).items():
        cut = IC.member_sums(x, assign, len(lengths), drop)
        hit = [l for l, m in enumerate(lengths) if len(list(drop(l, m)))]
        assert hit, name
        moved = np.abs(IC.unit(cut[filled]) - IC.unit(full[filled])).max(1)
        for l, d in zip(filled, moved):
            assert (d > 1e-4) if l in hit else (d == 0), (name, l, d)     # f32 rounding of a unit vector: 6e-8
    assert set().union(*[{l for l, m in enumerate(lengths) if len(list(d(l, m)))}
                         for d in IC.truncations(chunk).values()]) == {2, 3, 4, 5, 6, 8}


def test_builders_place_rows_in_their_lists():
    cent = IC.orthonormal_centroids(0, 16, 64)
    rows, want = IC.rows_near(1, cent, [0, 1, 15, 16, 17, 513] + [3] * 10)
    assert np.array_equal(IC.assign_reference(rows, cent), want)
    assert np.abs(np.linalg.norm(rows.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert np.bincount(want, minlength=16)[:6].tolist() == [0, 1, 15, 16, 17, 513]


# ---------------------------------------------------------------------------------- ABI
def test_new_symbols_in_header_binding_and_exports_within_abi_16():
    header = (ROOT / "include" / "vcap.h").read_text()
    assert re.search(r"#define VCAP_ABI_VERSION 16\b", header) and N.ABI_VERSION == 16
    lib = N.lib()
    assert lib.vcap_abi_version() == 16
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in N.SIGNATURES and hasattr(lib, name), name
    assert "scripts/build_index_with_captions.py" in header and "IndexIVFFlat" in header
    assert lib.vcap_ivf_slice_rows() == 512 and lib.vcap_ivf_chunk_rows() == 512


AS, UP, SE = "vcap_ivf_assign", "vcap_ivf_centroid_update", "vcap_ivf_search"
GOOD = {
    AS: dict(x=P, ldx=256, n=100, cent=P, nlist=16, dim=256, assign=P, score=P, stream=None),
    UP: dict(x=P, ldx=256, n=100, dim=256, order=P, offsets=P, nlist=16, prev=P, out=P, ws=P, ws_bytes=1 << 30,
             stream=None),
    SE: dict(dtype=N.DT_F32, rows=P, ids=P, offsets=P, ntotal=1000, cent=P, nlist=16, longest=100, dim=256, q=P, nq=4,
             nprobe=2, k=5, scores=P, out_ids=P, probes=None, ws=P, ws_bytes=1 << 30, max_blocks=0, stream=None),
}
DIM = ": dim must be a multiple of 64 in 64..1024"
NLIST = ": nlist must be in 1..1048576"
ROWS = [
    (AS, dict(x=None), ARG, AS + ": null pointer"),
    (AS, dict(cent=None), ARG, AS + ": null pointer"),
    (AS, dict(assign=None), ARG, AS + ": null pointer"),
    (AS, dict(n=-1), ARG, AS + ": bad sizes"),
    (AS, dict(nlist=-1), ARG, AS + ": bad sizes"),
    (AS, dict(ldx=128), ARG, AS + ": bad sizes"),
    (AS, dict(dim=96, ldx=96), UNSUP, AS + DIM),
    (AS, dict(dim=1088, ldx=1088), UNSUP, AS + DIM),
    (AS, dict(nlist=0), UNSUP, AS + NLIST),
    (AS, dict(nlist=(1 << 20) + 1), UNSUP, AS + NLIST),
    (AS, dict(n=1 << 31), UNSUP, AS + ": n must be below 2^31 rows"),
    (AS, dict(ldx=258), UNSUP, AS + ": ldx in whole 16-byte vectors; x and centroids 16-byte aligned"),
    (AS, dict(x=P + 4), UNSUP, AS + ": ldx in whole 16-byte vectors; x and centroids 16-byte aligned"),
    (UP, dict(x=None), ARG, UP + ": null pointer"),
    (UP, dict(order=None), ARG, UP + ": null pointer"),
    (UP, dict(offsets=None), ARG, UP + ": null pointer"),
    (UP, dict(prev=None), ARG, UP + ": null pointer"),
    (UP, dict(out=None), ARG, UP + ": null pointer"),
    (UP, dict(ws=None), ARG, UP + ": null pointer"),
    (UP, dict(n=-1), ARG, UP + ": bad sizes"),
    (UP, dict(ldx=255), ARG, UP + ": bad sizes"),
    (UP, dict(dim=32, ldx=32), UNSUP, UP + DIM),
    (UP, dict(nlist=0), UNSUP, UP + NLIST),
    (UP, dict(n=1 << 31), UNSUP, UP + ": n must be below 2^31 rows"),
    (UP, dict(x=P + 8), UNSUP, UP + ": ldx in whole 16-byte vectors; x and the workspace 16-byte aligned"),
    (UP, dict(ws_bytes=1024), WS, UP + ": workspace too small (vcap_ivf_centroid_update_workspace_bytes)"),
    (SE, dict(rows=None), ARG, SE + ": null pointer"),
    (SE, dict(ids=None), ARG, SE + ": null pointer"),
    (SE, dict(offsets=None), ARG, SE + ": null pointer"),
    (SE, dict(cent=None), ARG, SE + ": null pointer"),
    (SE, dict(q=None), ARG, SE + ": null pointer"),
    (SE, dict(scores=None), ARG, SE + ": null pointer"),
    (SE, dict(out_ids=None), ARG, SE + ": null pointer"),
    (SE, dict(ws=None), ARG, SE + ": null pointer"),
    (SE, dict(max_blocks=-1), ARG, SE + ": negative size"),
    (SE, dict(ntotal=-1), ARG, SE + ": negative size"),
    (SE, dict(nlist=-1), ARG, SE + ": negative size"),
    (SE, dict(longest=-1), ARG, SE + ": negative size"),
    (SE, dict(nprobe=-1), ARG, SE + ": negative size"),
    (SE, dict(k=-1), ARG, SE + ": negative size"),
    (SE, dict(dtype=N.DT_F16), ARG, SE + ": storage_dtype must be VCAP_DT_F32 or VCAP_DT_BF16"),
    (SE, dict(longest=1001), ARG, SE + ": max_list_len exceeds ntotal"),
    (SE, dict(dim=96), UNSUP, SE + DIM),
    (SE, dict(dim=1088, nq=1), UNSUP, SE + DIM),
    (SE, dict(k=0), UNSUP, SE + ": k must be in 1..128"),
    (SE, dict(k=129), UNSUP, SE + ": k must be in 1..128"),
    (SE, dict(nprobe=0), UNSUP, SE + ": nprobe must be in 1..128"),
    (SE, dict(nprobe=129), UNSUP, SE + ": nprobe must be in 1..128"),
    (SE, dict(nq=0), UNSUP, SE + ": nq must be in 1..64 with nq * dim <= 16384"),
    (SE, dict(nq=65, dim=64), UNSUP, SE + ": nq must be in 1..64 with nq * dim <= 16384"),
    (SE, dict(nq=17, dim=1024), UNSUP, SE + ": nq must be in 1..64 with nq * dim <= 16384"),
    (SE, dict(ntotal=1 << 31), UNSUP, SE + ": n must be below 2^31 rows"),
    (SE, dict(nlist=0), UNSUP, SE + NLIST),
    (SE, dict(nlist=(1 << 20) + 1), UNSUP, SE + NLIST),
    (SE, dict(rows=P + 8), UNSUP, SE + ": rows, centroids, queries and the workspace must be 16-byte aligned"),
    (SE, dict(ws_bytes=1024), WS, SE + ": workspace too small (vcap_ivf_search_workspace_bytes)"),
]


def _val(v):
    # an address inside _BUF is named by its offset from P: the id must not change from run to run
    if isinstance(v, int) and P <= v < P + 2048:
        return "ptr" if v == P else f"ptr+{v - P}"
    return str(v)


def _id(row):
    return "-".join([row[0][5:]] + [f"{k}={_val(v)}" for k, v in row[1].items()])


@pytest.mark.parametrize("row", ROWS, ids=_id)
def test_refused_before_any_launch(row):
    name, bad, code, text = row
    args = dict(GOOD[name])
    args.update(bad)
    lib = N.lib()
    assert (int(getattr(lib, name)(*args.values())), lib.vcap_last_error().decode()) == (code, text)


def test_every_new_entry_point_has_refusal_rows():
    assert {r[0] for r in ROWS} == set(GOOD)
    assert N.lib().vcap_ivf_search_workspace_bytes(65536, 1000, 256, 1, 1, 5) > 0      # nlist 65536 is inside the bound


# coarse: vcap_ip_search_workspace_bytes(nlist, dim, nq, nprobe); probes nq * nprobe * 8; their scores * 4;
# keys ceil(longest / 512) * nprobe * nq * k * 8 (one slice at least); each piece rounded up to 256 bytes
@pytest.mark.parametrize("args, expected", [
    ((1024, 10000, 256, 16, 8, 10), 270336 + 1024 + 512 + 204800),     # 8 * 16 * (8 + 256) * 8 | 20 slices
    ((50, 0, 64, 1, 1, 1), 2304 + 256 + 256 + 256),
    ((4096, 513, 1024, 16, 128, 128), 32 * 16 * 384 * 8 + 16384 + 8192 + 2 * 128 * 16 * 128 * 8),   # 32 coarse slabs
])
def test_search_workspace_sizes_are_pinned(args, expected):
    lib = N.lib()
    got = int(lib.vcap_ivf_search_workspace_bytes(*args))
    assert got == expected and got % 256 == 0
    nlist, _, dim, nq, nprobe, _ = args
    assert got > int(lib.vcap_ip_search_workspace_bytes(nlist, dim, nq, nprobe))


def test_workspace_queries_are_zero_outside_the_limits():
    lib = N.lib()
    for args in ((16, 100, 96, 1, 1, 5), (16, 100, 256, 65, 1, 5), (16, 100, 256, 1, 129, 5), (16, 100, 256, 1, 1, 129),
                 (0, 100, 256, 1, 1, 5), (16, -1, 256, 1, 1, 5), ((1 << 20) + 1, 100, 256, 1, 1, 5)):
        assert int(lib.vcap_ivf_search_workspace_bytes(*args)) == 0, args
    # (n / 512 + nlist + 1) partial rows of dim f32
    assert int(lib.vcap_ivf_centroid_update_workspace_bytes(1000, 16, 64)) == 18 * 64 * 4
    assert int(lib.vcap_ivf_centroid_update_workspace_bytes(1_000_000, 4096, 256)) == 6050 * 1024
    for args in ((-1, 16, 64), (1000, 0, 64), (1000, 16, 96), (1 << 31, 16, 64)):
        assert int(lib.vcap_ivf_centroid_update_workspace_bytes(*args)) == 0, args


# ---------------------------------------------------------------------------------- python surface
def _cpu_ivf(storage="f32"):
    """An IVF index assembled on the host (no device work): 3 lists over 5 rows."""
    import torch
    from vcap.retrieval import IVFFlatIPIndex
    idx = IVFFlatIPIndex(64, 3, storage, device="cpu", nprobe=2)
    rng = np.random.default_rng(0)
    idx.set_centroids(IC.unit(rng.standard_normal((3, 64))).astype(np.float32))
    rows = torch.from_numpy(rng.standard_normal((5, 64)).astype(np.float32))
    idx._rows = rows if storage == "f32" else rows.to(torch.bfloat16)
    idx._ids = torch.tensor([3, 0, 4, 1, 2])
    idx._host_offsets = np.array([0, 1, 1, 5], np.int64)
    idx._offsets = torch.from_numpy(idx._host_offsets)
    idx._lists = torch.tensor([0, 2, 2, 2, 2], dtype=torch.int32)
    idx.ntotal = 5
    idx.metadata = [{"video_id": f"v{i}", "caption": f"c{i}"} for i in range(5)]
    return idx


@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_save_load_round_trip_of_the_files(tmp_path, storage):
    import torch
    from vcap.retrieval import IVFFlatIPIndex, load_index
    idx = _cpu_ivf(storage)
    idx.save(tmp_path / "ivf")
    assert json.loads((tmp_path / "ivf" / "index.json").read_text()) == {
        "type": "IVF_FLAT", "dim": 64, "storage": storage, "ntotal": 5, "normalize": False, "nlist": 3, "nprobe": 2}
    assert {p.name for p in (tmp_path / "ivf").iterdir()} == {"index.json", "centroids.npy", "vectors.npy", "ids.npy",
                                                              "offsets.npy", "meta.json"}
    assert np.load(tmp_path / "ivf" / "vectors.npy").dtype == (np.float32 if storage == "f32" else np.uint16)
    back = load_index(tmp_path / "ivf", "cpu")
    assert isinstance(back, IVFFlatIPIndex) and back.is_trained
    assert (back.ntotal, back.nlist, back.nprobe, back.storage, back.metadata[4]) == (5, 3, 2, storage, idx.metadata[4])
    raw = torch.int32 if storage == "f32" else torch.int16
    assert torch.equal(back.vectors.view(raw), idx.vectors.view(raw)) and torch.equal(back.ids, idx.ids)
    assert torch.equal(back.centroids, idx.centroids) and back.list_sizes().tolist() == [1, 0, 4]
    assert back._lists.tolist() == [0, 2, 2, 2, 2]
    np.save(tmp_path / "ivf" / "ids.npy", np.array([3, 0, 4, 1, 1]))
    with pytest.raises(ValueError, match="permutation"):
        load_index(tmp_path / "ivf", "cpu")


def test_load_index_reads_a_flat_directory_without_a_type_key(tmp_path):
    """Today's FlatIPIndex.save layout: index.json has no "type"."""
    from vcap.retrieval import FlatIPIndex, load_index
    d = tmp_path / "flat"
    d.mkdir()
    np.save(d / "vectors.npy", np.zeros((0, 256), np.float32))
    (d / "index.json").write_text(json.dumps({"dim": 256, "storage": "f32", "ntotal": 0, "normalize": True}))
    (d / "meta.json").write_text("[]")
    idx = load_index(d, "cpu")
    assert isinstance(idx, FlatIPIndex) and (idx.dim, idx.ntotal, idx.normalize, idx.metadata) == (256, 0, True, [])
    FlatIPIndex(64, "bf16", device="cpu").save(tmp_path / "flat2")
    assert "type" not in json.loads((tmp_path / "flat2" / "index.json").read_text())       # FlatIPIndex is untouched
    assert isinstance(load_index(tmp_path / "flat2", "cpu"), FlatIPIndex)
    (d / "index.json").write_text(json.dumps({"type": "HNSW", "dim": 256}))
    with pytest.raises(ValueError, match="unknown index type"):
        load_index(d, "cpu")


def test_index_argument_checks_need_no_device():
    from vcap.retrieval import IVFFlatIPIndex
    with pytest.raises(ValueError):
        IVFFlatIPIndex(96, 4, device="cpu")
    with pytest.raises(ValueError):
        IVFFlatIPIndex(64, 0, device="cpu")
    with pytest.raises(ValueError):
        IVFFlatIPIndex(64, 4, "f16", device="cpu")
    idx = IVFFlatIPIndex(64, 8, device="cpu")
    assert not idx.is_trained and idx.ntotal == 0 and idx.nprobe == 1 and idx.list_sizes().tolist() == [0] * 8
    with pytest.raises(ValueError, match="at least nlist"):
        idx.train(np.zeros((7, 64), np.float32))
    with pytest.raises(RuntimeError):
        idx.add(np.zeros((1, 64), np.float32))
    with pytest.raises(RuntimeError):
        idx.search(np.zeros((1, 64), np.float32), 1)
    with pytest.raises(RuntimeError):
        idx.save("unused")
    with pytest.raises(ValueError):
        idx.set_centroids(np.zeros((7, 64), np.float32))


def test_scripts_parse_the_index_flags():
    from scripts import build_index, build_index_with_captions, eval_retrieval, query_text, query_video
    a = build_index_with_captions.parse(["--ann_path", "a.json", "--out_dir", "o", "--ckpt", "c.pt", "--num_frame", "4",
                                         "--image_size", "112", "--index_type", "IVF_FLAT", "--nlist", "7"])
    assert (a.ann_path, a.out_dir, a.ckpt, a.num_frame, a.num_frames, a.image_size, a.index_type, a.nlist) == \
        ("a.json", "o", "c.pt", 4, 4, 112, "IVF_FLAT", 7)
    d = build_index_with_captions.parse(["--ann_path", "a.json", "--out_dir", "o"])
    assert (d.index_type, d.nlist, d.num_frame, d.image_size, d.storage, d.precision, d.weights_seed, d.device) == \
        ("Flat", 50, 8, 224, "f32", "bf16", None, "cuda")
    with pytest.raises(SystemExit):
        build_index_with_captions.parse(["--ann_path", "a", "--out_dir", "o", "--index_type", "HNSW"])
    assert build_index_with_captions.caption_of({"captions": ["x", "y"]}) == "x"
    assert build_index_with_captions.caption_of({"caption": "z"}) == "z" and build_index_with_captions.caption_of({}) == ""
    b = build_index.parse(["--features", "f", "--annotations", "a", "--out_dir", "o"])
    assert (b.index_type, b.nlist, b.storage) == ("Flat", 50, "f32")
    assert build_index.parse(["--features", "f", "--annotations", "a", "--out_dir", "o", "--index_type", "IVF_FLAT",
                              "--nlist", "4"]).nlist == 4
    assert query_video.parse(["--frames_dir", "c", "--index", "i"]).nprobe == 0
    assert query_video.parse(["--frames_dir", "c", "--index", "i", "--nprobe", "8"]).nprobe == 8
    assert eval_retrieval.parse(["--annotations", "a", "--index", "i", "--nprobe", "3"]).nprobe == 3
    assert query_text.parse(["--index_dir", "i", "--ckpt", "c", "--pad_id", "0", "--nprobe", "2"]).nprobe == 2
