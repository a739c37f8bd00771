"""The text tower on the GPU (vcap_text_encode through HipTextEmbedder) against the float64 oracle of
tests/text_tower_cases.py on its whole case table, in both operand dtypes; determinism; chunking over the
row limit; the NaN answer to an out-of-range id on the device; text-to-video search end to end through
scripts/query_text.py in a fresh process; HipAlignModel.forward.

Bounds (derived in text_tower_cases.py): f32 out 1e-5 and hidden_out HIDDEN_ATOL against the fp64 oracle;
bf16 4 x the case's CPU rounding budget plus the f32 bound.  Every test prints its figures before it asserts.
"""
import json
import subprocess
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

import text_tower_cases as TC
from helpers import case as golden_case
from vcap import retrieval as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


@lru_cache(maxsize=None)
def _embedder(name: str, dtype: str) -> R.HipTextEmbedder:
    return R.HipTextEmbedder.from_state_dict(TC.state_dict(name), TC.PAD_ID[name], TC.TOWERS[name][1], dtype, "cuda:0")


def _encode(name, dtype, ids, hidden=True):
    emb = _embedder(name, dtype)
    got = emb.encode_text(ids, return_hidden=hidden)
    torch.cuda.synchronize()
    if hidden:
        return got[0].cpu().numpy(), got[1].cpu().numpy()
    return got.cpu().numpy()


@pytest.mark.parametrize("case", TC.CASES, ids=TC.CASE_IDS)
def test_f32_matches_the_fp64_oracle(device, case):
    want_o, want_h = TC.oracle(case)
    out, hid = _encode(case.tower, "f32", TC.ids_of(case))
    eo, eh = float(np.abs(out - want_o).max()), float(np.abs(hid - want_h).max())
    print(f"TEXT_F32 {case.id} out_err {eo:.3e} (bound {TC.F32_OUT_ATOL:.1e}) hidden_err {eh:.3e} "
          f"(bound {TC.HIDDEN_ATOL:.3e})")
    assert out.dtype == np.float32 and out.shape == want_o.shape and hid.shape == want_h.shape
    assert eo <= TC.F32_OUT_ATOL
    assert eh <= TC.HIDDEN_ATOL
    assert np.abs(np.linalg.norm(out.astype(np.float64), axis=1) - 1).max() <= 1e-6


@pytest.mark.parametrize("case", TC.CASES, ids=TC.CASE_IDS)
def test_bf16_stays_inside_four_rounding_budgets(device, case):
    want_o, want_h = TC.oracle(case)
    bo, bh = TC.bf16_budget(case)
    out, hid = _encode(case.tower, "bf16", TC.ids_of(case))
    eo, eh = float(np.abs(out - want_o).max()), float(np.abs(hid - want_h).max())
    print(f"TEXT_BF16 {case.id} out_err {eo:.3e} budget {bo:.3e} ratio {eo / bo if bo else float('nan'):.2f} "
          f"hidden_err {eh:.3e} budget {bh:.3e} ratio {eh / bh if bh else float('nan'):.2f}")
    assert eo <= 4 * bo + TC.F32_OUT_ATOL
    assert eh <= 4 * bh + TC.HIDDEN_ATOL
    assert np.abs(np.linalg.norm(out.astype(np.float64), axis=1) - 1).max() <= 1e-6


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", [c for c in TC.CASES if (c.tower, c.B, c.L) in
                                  {("e128", 3, 11), ("ref", 8, 64), ("ref", 1, 17), ("ref_0layers", 5, 33)}],
                         ids=lambda c: c.id)
def test_two_calls_give_the_same_bits_with_or_without_hidden_out(device, case, dtype):
    ids = TC.ids_of(case)
    o1, h1 = _encode(case.tower, dtype, ids)
    o2, h2 = _encode(case.tower, dtype, ids)
    o3 = _encode(case.tower, dtype, ids, hidden=False)
    assert o1.tobytes() == o2.tobytes() == o3.tobytes() and h1.tobytes() == h2.tobytes()


def test_a_batch_over_the_row_limit_goes_in_chunks(device):
    """B = 9, L = 64 is 576 rows, over vcap_gpt2_max_rows() = 512: two calls of 8 and 1 captions."""
    name = "ref"
    big = TC.Case(name, 9, 64, ("none", "trailing", "interior", "allpad", "trailing", "none", "interior",
                                "trailing", "none"))
    ids = TC.ids_of(big)
    assert ids.shape[0] * ids.shape[1] > _embedder(name, "f32").max_rows
    out = _encode(name, "f32", ids, hidden=False)
    single = np.concatenate([_encode(name, "f32", ids[i:i + 1], hidden=False) for i in range(9)])
    want, _ = TC.oracle(big)
    e_single, e_oracle = float(np.abs(out - single).max()), float(np.abs(out - want).max())
    print(f"TEXT_CHUNK vs per-caption {e_single:.3e} vs oracle {e_oracle:.3e}")
    assert e_single <= TC.F32_OUT_ATOL and e_oracle <= TC.F32_OUT_ATOL


@pytest.mark.parametrize("name", ["ref", "ref_0layers", "e128"])
@pytest.mark.parametrize("bad", ["vocab", "negative"])
def test_an_out_of_range_id_on_the_device_is_nan_for_its_caption_only(device, name, bad):
    c = TC.Case(name, 3, 11, ("trailing", "none", "none"))
    ids = TC.ids_of(c).copy()
    want, _ = TC.oracle(c)
    ids[1, 4] = TC.TOWERS[name][5] if bad == "vocab" else -1
    t = torch.from_numpy(ids).to(device)                      # a device tensor is not range-checked on the host
    out, hid = _embedder(name, "f32").encode_text(t, return_hidden=True)
    torch.cuda.synchronize()
    out, hid = out.cpu().numpy(), hid.cpu().numpy()
    assert np.isnan(out[1]).all()
    assert np.isfinite(out[[0, 2]]).all() and np.isfinite(hid[[0, 2]]).all()
    assert np.abs(out[[0, 2]] - want[[0, 2]]).max() <= TC.F32_OUT_ATOL
    with pytest.raises(ValueError, match="outside"):
        _embedder(name, "f32").encode_text(ids)               # the same ids from the host are refused


def test_host_side_refusals(device):
    emb = _embedder("e128", "f32")
    with pytest.raises(ValueError, match="at most 64"):
        emb.encode_text(np.ones((1, 65), np.int64))
    out = emb.encode_text([1, 2, 3])                          # [L] -> one caption
    assert tuple(out.shape) == (1, 64) and out.is_cuda and out.dtype == torch.float32


def test_text_to_video_search_in_a_fresh_process(device, tmp_path):
    """40 distinct captions indexed by their text embeddings; scripts.query_text in a child process finds
    caption i first with score 1 for three i - one of them shorter than the others, so the script's right
    padding with pad_id has to reproduce the indexed row."""
    name, pad = "ref", TC.PAD_ID["ref"]
    V, L = TC.TOWERS[name][5], 12
    rs = np.random.RandomState(11)
    ids = rs.randint(1, V, size=(40, L)).astype(np.int64)
    ids[17, 8:] = pad                                          # caption 17 has 8 tokens
    assert len({tuple(r) for r in ids.tolist()}) == 40
    index = R.FlatIPIndex(TC.TOWERS[name][4], "f32", device)
    index.add(_embedder(name, "f32").encode_text(ids))
    index.metadata = [{"video_id": f"vid{i}", "caption": f"caption {i}"} for i in range(40)]
    index.save(tmp_path / "index")
    ckpt = tmp_path / "align.pt"
    torch.save({"model_state": {k: torch.from_numpy(v) for k, v in TC.state_dict(name).items()}}, ckpt)
    picks = [3, 17, 39]
    cmd = [sys.executable, "-m", "scripts.query_text", "--index_dir", str(tmp_path / "index"), "--ckpt", str(ckpt),
           "--pad_id", str(pad), "--topk", "5", "--device", str(device), "--out_json", str(tmp_path / "hits.json")]
    for i in picks:
        toks = [t for t in ids[i].tolist() if t != pad]
        cmd += ["--ids", " ".join(map(str, toks))]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    hits = json.loads((tmp_path / "hits.json").read_text())
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("[1] ")]
    assert len(hits) == len(lines) == 3
    for i, h, ln in zip(picks, hits, lines):
        print(f"TEXT_QUERY caption {i}: first hit {h[0]}")
        assert h[0][0] == i and abs(h[0][1] - 1.0) <= 1e-5 and len(h) == 5
        assert all(a[1] >= b[1] for a, b in zip(h, h[1:])) and h[1][1] < 0.999
        assert ln == f"[1] score={h[0][1]:.4f} | id=vid{i} | caption=caption {i}"


def test_align_model_forward_is_the_cosine_embedding_loss(device):
    meta, g, va, ga, sd, frames = golden_case("tiny")
    name = "ref"
    c = TC.Case(name, meta["B"], 16, ("none", "trailing"))
    want_t, _ = TC.oracle(c)
    want_v = torch.nn.functional.normalize(torch.from_numpy(g["encoder_out"]).double(), dim=1)
    assert want_v.shape == want_t.shape
    want = float(torch.nn.CosineEmbeddingLoss()(want_v, torch.from_numpy(want_t), torch.ones(meta["B"], dtype=torch.float64)))
    model = R.HipAlignModel(R.HipVideoEmbedder.from_state_dict(sd, va, "fp32", device), _embedder(name, "f32"))
    video = torch.from_numpy(frames).to(device)
    loss = model(video, TC.ids_of(c))
    torch.cuda.synchronize()
    assert loss.is_cuda and loss.dim() == 0
    print(f"TEXT_ALIGN loss {float(loss):.8f} oracle {want:.8f}")
    assert abs(float(loss) - want) <= TC.F32_OUT_ATOL
    assert torch.equal(model.encode_text(TC.ids_of(c)), _embedder(name, "f32").encode_text(TC.ids_of(c)))
    assert tuple(model.encode_video(video).shape) == (meta["B"], 256)
