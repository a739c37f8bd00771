"""CPU suite of the video-retrieval feature: the fp64 restatement of the flat-IP search against a
brute-force loop, retrieval_metrics on hand-worked rankings, the alignment-model key remap, the index
directory's meta.json schema, the new ABI symbols (header, binding, exports; ABI still 16), every
argument refusal of the new entry points (returned before any launch: the library loads without a GPU),
and the pinned workspace sizes."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest

import retrieval_cases as RC
from vcap import _native as N

ROOT = Path(__file__).resolve().parents[1]
ARG, WS, UNSUP = N.E_ARG, N.E_WORKSPACE, N.E_UNSUPPORTED
NEW_SYMBOLS = ("vcap_l2_normalize", "vcap_ip_index_convert", "vcap_ip_search", "vcap_ip_search_workspace_bytes",
               "vcap_ip_search_slab_rows", "vcap_ip_search_workgroups")

_BUF = C.create_string_buffer(4096)
P = (C.addressof(_BUF) + 255) & ~255      # a non-null, aligned address no refused call reads


# ---------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("seed, n, dim, nq, k", [(0, 7, 4, 2, 3), (1, 5, 8, 3, 5), (2, 3, 4, 1, 6), (3, 0, 4, 2, 2)])
def test_restatement_matches_brute_force(seed, n, dim, nq, k):
    rng = np.random.default_rng(seed)
    db = rng.integers(-3, 4, (n, dim)).astype(np.float32)     # small integers: exact sums, many ties
    q = rng.integers(-3, 4, (nq, dim)).astype(np.float32)
    D, I = RC.flat_ip_reference(db, q, k)
    Db, Ib = RC.brute_force(db, q, k)
    assert np.array_equal(I, Ib) and np.array_equal(D, Db)
    RC.check_topk(D, I, db, q, k)


def test_restatement_orders_ties_by_id_and_drops_nan():
    db = np.array([[1, 0], [2, 0], [1, 0], [np.nan, 0], [2, 0]], np.float32)
    D, I = RC.flat_ip_reference(db, np.array([[1, 0]], np.float32), 5)
    assert I.tolist() == [[1, 4, 0, 2, -1]]
    assert D.tolist() == [[2, 2, 1, 1, -np.inf]]


def test_check_topk_rejects_a_wrong_answer():
    db, q, _ = RC.separated_case(0, 64, 64, 1, 3)
    D, I = RC.flat_ip_reference(db, q, 3)
    RC.check_topk(D, I, db, q, 3)
    bad = I.copy()
    bad[0, 2] = int(np.setdiff1d(np.arange(64), I[0])[0])
    with pytest.raises(AssertionError):
        RC.check_topk(D, bad, db, q, 3)
    with pytest.raises(AssertionError):
        RC.check_topk(D[:, ::-1], I[:, ::-1], db, q, 3)


def test_separated_case_is_separated_and_bound_value():
    assert float(RC.error_bound(256, 1.0, 1.0)) == pytest.approx(3.05e-5, rel=2e-3)
    db, q, win = RC.separated_case(5, 700, 256, 3, 5)
    RC.assert_separated(db, q, 5, win)
    RC.assert_separated(RC.bf16_round(db), q, 5, win)
    assert np.array_equal(RC.flat_ip_reference(db, q, 5)[1], win[:, :5])


def test_bf16_round_matches_torch():
    import torch
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    assert np.array_equal(RC.bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())


# ---------------------------------------------------------------------------------- python surface
def test_retrieval_metrics_hand_worked():
    from vcap.retrieval import retrieval_metrics
    ranked = [[4, 1, 2, 3, 0],     # gold 4: rank 1
              [9, 8, 7, 6, 5],     # gold 7: rank 3
              [0, 1, 2, 3, 4],     # gold 4: rank 5
              [0, 1, 2, 3, -1]]    # gold 11: absent -> contributes 0
    m = retrieval_metrics(np.array(ranked), [4, 7, 4, 11], ks=(1, 5))
    assert m["n"] == 4
    assert m["recall@1"] == pytest.approx(1 / 4)
    assert m["recall@5"] == pytest.approx(3 / 4)
    assert m["mrr"] == pytest.approx((1 + 1 / 3 + 1 / 5 + 0) / 4)
    assert retrieval_metrics([], [], ks=(1,)) == {"recall@1": 0.0, "mrr": 0.0, "n": 0}
    with pytest.raises(ValueError):
        retrieval_metrics([[1]], [1, 2])


def test_alignment_layout_maps_onto_the_caption_layout():
    import torch
    from vcap.retrieval import remap_alignment_state_dict
    w = np.arange(6, dtype=np.float32).reshape(2, 3)
    align = {"model_state": {"vit.blocks.0.norm1.weight": torch.from_numpy(w), "vit.cls_token": w,
                             "vid_proj.weight": w, "vid_proj.bias": w[0], "txt_embed.weight": w, "txt_proj.bias": w[0]}}
    sd = remap_alignment_state_dict(align)
    assert set(sd) == {"encoder.backbone.blocks.0.norm1.weight", "encoder.backbone.cls_token", "encoder.proj.weight",
                       "encoder.proj.bias"}
    assert all(v.dtype == np.float32 for v in sd.values()) and np.array_equal(sd["encoder.proj.weight"], w)
    caption = {"encoder.backbone.norm.weight": w, "encoder.proj.bias": w[0], "decoder.mapper.0.bias": w[0]}
    assert set(remap_alignment_state_dict(caption)) == set(caption)     # the caption layout passes through


def test_index_save_writes_the_reference_meta_schema(tmp_path):
    """FlatIPIndex.save on an empty index (no device work) with metadata attached: vectors.npy,
    index.json and meta.json as build_index.py:31-34, 45-46 writes it."""
    from vcap.retrieval import FlatIPIndex, check_meta, first_caption, meta_caption
    anns = [{"video_id": "vid_a", "captions": ["a man rides", "second"]}, {"video_id": "vid_b", "captions": []},
            {"video_id": "vid_c", "captions": "not a list"}]
    idx = FlatIPIndex(256, "bf16", device="cpu")
    idx.metadata = [{"video_id": r["video_id"], "caption": first_caption(r)} for r in anns]
    idx.save(tmp_path / "index")
    meta = json.loads((tmp_path / "index" / "meta.json").read_text("utf-8"))
    assert meta == [{"video_id": "vid_a", "caption": "a man rides"}, {"video_id": "vid_b", "caption": ""},
                    {"video_id": "vid_c", "caption": ""}]
    assert check_meta(meta) is meta and [meta_caption(m) for m in meta] == ["a man rides", "", ""]
    assert meta_caption({"captions": ["x", "y"]}) == "x" and meta_caption({}) == "(no caption)"
    assert json.loads((tmp_path / "index" / "index.json").read_text()) == {"dim": 256, "storage": "bf16", "ntotal": 0,
                                                                           "normalize": False}
    v = np.load(tmp_path / "index" / "vectors.npy")
    assert v.shape == (0, 256) and v.dtype == np.uint16
    with pytest.raises(ValueError):
        idx.metadata = [{"video_id": "x", "captions": ["list form is not the index schema"]}]
        idx.save(tmp_path / "bad")


def test_scripts_parse_and_refuse_a_video_file():
    from scripts import build_index, eval_retrieval, extract_features, query_video
    a = query_video.parse(["--frames_dir", "clip", "--index", "idx", "--k", "3"])
    assert (a.frames_dir, a.k, a.index, a.num_frames, a.image_size) == ("clip", 3, "idx", 8, 224)
    with pytest.raises(SystemExit, match="--video needs a frame extractor"):
        query_video.main(["--video", "clip.mp4", "--index", "idx"])
    assert build_index.parse(["--features", "f", "--annotations", "a", "--out_dir", "o"]).storage == "f32"
    assert extract_features.parse(["--annotations", "a", "--out_dir", "o"]).precision == "bf16"
    assert eval_retrieval.KS == (1, 5)


# ---------------------------------------------------------------------------------- ABI
def test_new_symbols_in_header_binding_and_exports_within_abi_16():
    header = (ROOT / "include" / "vcap.h").read_text()
    assert re.search(r"#define VCAP_ABI_VERSION 16\b", header) and N.ABI_VERSION == 16
    lib = N.lib()
    assert lib.vcap_abi_version() == 16
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in N.SIGNATURES and hasattr(lib, name), name
    for cite in ("scripts/build_index.py:40-42", "scripts/query_video.py:20-21", "61-75", "127",
                 "src/models/vit_text_align.py:54-65", "src/models/video_encoder.py:318-319"):
        assert cite in header, cite


def test_plugin_registry_names_the_retrieval_entry_points():
    from core.operators.plugin_hooks import get_plugin_hook
    assert get_plugin_hook("flat_ip_search").abi_symbol == "vcap_ip_search"
    assert get_plugin_hook("l2_normalize").abi_symbol == "vcap_l2_normalize"


GOOD = {
    "vcap_l2_normalize": dict(x=P, ldx=256, y=P, ldy=256, rows=4, dim=256, eps=1e-12, mode=0, stream=None),
    "vcap_ip_index_convert": dict(x=P, ldx=256, rows=4, dim=256, dtype=N.DT_BF16, dst=P, stream=None),
    "vcap_ip_search": dict(dtype=N.DT_F32, db=P, n=1000, dim=256, q=P, nq=4, k=5, scores=P, ids=P, ws=P,
                           ws_bytes=1 << 30, max_blocks=0, stream=None),
}
L2, CV, IP = "vcap_l2_normalize", "vcap_ip_index_convert", "vcap_ip_search"
LIMITS = {"dim": "vcap_ip_search: dim must be a multiple of 64 in 64..1024", "k": "vcap_ip_search: k must be in 1..128",
          "nq": "vcap_ip_search: nq must be in 1..64 with nq * dim <= 16384"}
ROWS = [
    (L2, dict(x=None), ARG, "vcap_l2_normalize: bad arguments"),
    (L2, dict(y=None), ARG, "vcap_l2_normalize: bad arguments"),
    (L2, dict(rows=-1), ARG, "vcap_l2_normalize: bad arguments"),
    (L2, dict(dim=0), ARG, "vcap_l2_normalize: bad arguments"),
    (L2, dict(ldx=255), ARG, "vcap_l2_normalize: bad arguments"),
    (L2, dict(ldy=255), ARG, "vcap_l2_normalize: bad arguments"),
    (L2, dict(mode=2), ARG, "vcap_l2_normalize: eps_mode must be 0 (max(norm, eps)) or 1 (norm + eps)"),
    (CV, dict(x=None), ARG, "vcap_ip_index_convert: bad arguments"),
    (CV, dict(dst=None), ARG, "vcap_ip_index_convert: bad arguments"),
    (CV, dict(rows=-1), ARG, "vcap_ip_index_convert: bad arguments"),
    (CV, dict(ldx=128), ARG, "vcap_ip_index_convert: bad arguments"),
    (CV, dict(dtype=N.DT_F16), ARG, "vcap_ip_index_convert: storage_dtype must be VCAP_DT_F32 or VCAP_DT_BF16"),
    (CV, dict(dim=254, ldx=256), UNSUP,
     "vcap_ip_index_convert: dim and ldx in whole 16-byte vectors; x and dst 16-byte aligned"),
    (CV, dict(x=P + 4), UNSUP, "vcap_ip_index_convert: dim and ldx in whole 16-byte vectors; x and dst 16-byte aligned"),
    (IP, dict(db=None), ARG, "vcap_ip_search: null pointer"),
    (IP, dict(q=None), ARG, "vcap_ip_search: null pointer"),
    (IP, dict(scores=None), ARG, "vcap_ip_search: null pointer"),
    (IP, dict(ids=None), ARG, "vcap_ip_search: null pointer"),
    (IP, dict(ws=None), ARG, "vcap_ip_search: null pointer"),
    (IP, dict(n=-1), ARG, "vcap_ip_search: negative size"),
    (IP, dict(nq=-1), ARG, "vcap_ip_search: negative size"),
    (IP, dict(k=-1), ARG, "vcap_ip_search: negative size"),
    (IP, dict(dim=-64), ARG, "vcap_ip_search: negative size"),
    (IP, dict(max_blocks=-1), ARG, "vcap_ip_search: negative size"),
    (IP, dict(dtype=N.DT_F16), ARG, "vcap_ip_search: storage_dtype must be VCAP_DT_F32 or VCAP_DT_BF16"),
    (IP, dict(dtype=N.DT_MXFP8), ARG, "vcap_ip_search: storage_dtype must be VCAP_DT_F32 or VCAP_DT_BF16"),
    (IP, dict(dim=0), UNSUP, LIMITS["dim"]),
    (IP, dict(dim=96), UNSUP, LIMITS["dim"]),
    (IP, dict(dim=1088, nq=1), UNSUP, LIMITS["dim"]),
    (IP, dict(k=0), UNSUP, LIMITS["k"]),
    (IP, dict(k=129), UNSUP, LIMITS["k"]),
    (IP, dict(nq=0), UNSUP, LIMITS["nq"]),
    (IP, dict(nq=65, dim=64), UNSUP, LIMITS["nq"]),
    (IP, dict(nq=17, dim=1024), UNSUP, LIMITS["nq"]),
    (IP, dict(n=1 << 31), UNSUP, "vcap_ip_search: n must be below 2^31 rows"),
    (IP, dict(db=P + 8), UNSUP, "vcap_ip_search: db and queries must be 16-byte aligned, the workspace 8-byte"),
    (IP, dict(ws_bytes=1024), WS, "vcap_ip_search: workspace too small (vcap_ip_search_workspace_bytes)"),
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


# per scan workgroup and query: k + 2 * slab rows slots of 8 bytes; min(512, ceil(n / slab rows)) workgroups;
# the queries of one pass (16 * max(1, min(4, 1024 / dim)) at most)
@pytest.mark.parametrize("args, expected", [
    ((2000, 256, 1, 5), 33536),                            # 16 * 1 * (5 + 256) * 8 = 33408, rounded up
    ((1_000_000, 256, 64, 100), 93_323_264),               # 512 * 64 * (100 + 256) * 8
    ((70_001, 1024, 16, 128), 25_165_824),                  # 512 * 16 * (128 + 256) * 8
    ((0, 64, 3, 5), 6400),                                 # one (unused) workgroup, rounded up to 256 bytes
    ((100_000, 768, 21, 10), 17_432_576),                   # 512 * 16 * (10 + 256) * 8: 21 queries at dim 768 = two passes of <= 16
])
def test_workspace_sizes_are_pinned(args, expected):
    lib = N.lib()
    assert lib.vcap_ip_search_slab_rows() == 128
    got = int(lib.vcap_ip_search_workspace_bytes(*args))
    assert got == expected and got % 256 == 0


def test_workspace_query_is_zero_outside_the_limits():
    lib = N.lib()
    for args in ((1000, 96, 1, 5), (1000, 256, 65, 5), (1000, 256, 1, 129), (-1, 256, 1, 5), (1000, 1024, 17, 5)):
        assert int(lib.vcap_ip_search_workspace_bytes(*args)) == 0
    assert lib.vcap_ip_search_workgroups(0, 0) == 1 and lib.vcap_ip_search_workgroups(129, 0) == 2
    assert lib.vcap_ip_search_workgroups(10 ** 6, 32) == 32 and lib.vcap_ip_search_workgroups(-1, 0) == ARG
