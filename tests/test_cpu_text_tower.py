"""The text tower without a GPU: the oracles of text_tower_cases.py against each other, the three facts of
the reference's encode_text the device path must reproduce (pads are attended, the pad row is gathered as
stored, an all-pad caption gives normalize(proj.bias)), the state-dict split, and every refusal of
vcap_text_encode / vcap_text_workspace_bytes (csrc/runtime_text.hip) through the C ABI with dummy pointers:
each row is refused before any launch, so nothing is dereferenced on the device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import text_tower_cases as TC
from vcap import _native as N
from vcap import retrieval as R

ARG, WS, UNSUP = N.E_ARG, N.E_WORKSPACE, N.E_UNSUPPORTED


@pytest.mark.parametrize("case", TC.CASES, ids=TC.CASE_IDS)
def test_numpy_restatement_equals_torch_float64(case):
    (o, h), (o2, h2) = TC.oracle(case), TC.restated(case)
    assert o.shape == (case.B, TC.TOWERS[case.tower][4]) and h.shape == (case.B, case.L, TC.TOWERS[case.tower][0])
    assert np.abs(o - o2).max() <= 1e-10 and np.abs(h - h2).max() <= 1e-10
    assert np.abs(np.linalg.norm(o, axis=1) - 1).max() <= 1e-12


def test_pads_are_attended():
    """A padded caption is not its trimmed self: the encoder gets no key-padding mask, only the pool does."""
    name, pad = "ref", TC.PAD_ID["ref"]
    ids = TC.ids_of(TC.Case(name, 1, 16, ("none",)))[:, :12].copy()
    ids[0, 7:] = pad
    padded, _ = TC.oracle_ids(name, ids)
    trimmed, _ = TC.oracle_ids(name, ids[:, :7])
    assert np.abs(padded - trimmed).max() > 1e-3


def test_pad_row_is_gathered_as_stored():
    name = "e128"
    sd = TC.state_dict(name)
    assert np.abs(sd["txt_emb.weight"][TC.PAD_ID[name]]).max() > 0.1        # a checkpoint's pad row is not zero
    ids = np.full((1, 4), TC.PAD_ID[name], np.int64)
    _, hidden = TC.np_tower({k: v for k, v in sd.items() if not k.startswith("txt_enc.")}, ids, TC.PAD_ID[name], 2)
    assert np.array_equal(hidden[0, 0], sd["txt_emb.weight"][TC.PAD_ID[name]].astype(np.float64))


@pytest.mark.parametrize("name", list(TC.TOWERS))
def test_all_pad_caption_is_normalized_bias(name):
    case = TC.Case(name, 2, 16, ("none", "allpad"))
    out, _ = TC.oracle(case)
    b = TC.state_dict(name)["txt_proj.bias"].astype(np.float64)
    assert np.abs(out[1] - b / np.linalg.norm(b)).max() <= 1e-12
    assert np.abs(out[0] - out[1]).max() > 1e-2


def test_state_dict_split():
    rs = np.random.RandomState(0)
    txt = TC.state_dict("e128")
    state = {"vit.blocks.0.attn.qkv.weight": rs.randn(6, 4).astype(np.float64), "vit.cls_token": rs.randn(1, 1, 4),
             "vid_proj.weight": rs.randn(3, 4), "vid_proj.bias": rs.randn(3), "encoder.proj.extra": rs.randn(2),
             **txt}
    for wrapped in (state, {"model_state": state}):
        got = R.text_tower_state_dict(wrapped)
        assert set(got) == set(txt) and all(k.startswith("txt_") for k in got)
        assert all(v.dtype == np.float32 and np.array_equal(v, txt[k]) for k, v in got.items())
        # remap_alignment_state_dict as it was: vit.* / vid_proj.* renamed, txt_* dropped, f32
        vid = R.remap_alignment_state_dict(wrapped)
        assert list(vid) == ["encoder.backbone.blocks.0.attn.qkv.weight", "encoder.backbone.cls_token",
                             "encoder.proj.weight", "encoder.proj.bias", "encoder.proj.extra"]
        src = ["vit.blocks.0.attn.qkv.weight", "vit.cls_token", "vid_proj.weight", "vid_proj.bias", "encoder.proj.extra"]
        for k, s in zip(vid, src):
            assert vid[k].dtype == np.float32 and np.array_equal(vid[k], state[s].astype(np.float32))
    import torch
    got = R.text_tower_state_dict({k: torch.from_numpy(v).double() for k, v in txt.items()})
    assert all(v.dtype == np.float32 and np.array_equal(v, txt[k]) for k, v in got.items())


# ---- refusals
_BUF = C.create_string_buffer(4096)
P = (C.addressof(_BUF) + 15) & ~15           # a 16-byte-aligned non-null address no refused call reads
BIG = 1 << 30


def _layers(n=2, **bad):
    arr = (N.TextLayer * n)()
    for ly in arr:
        for f, _ in N.TextLayer._fields_:
            setattr(ly, f, P)
    for f, v in bad.items():
        setattr(arr[n - 1], f, v)
    return arr


_KEEP = []


def _desc(**kw):
    f = dict(dtype=N.DT_F32, vocab=97, dim=128, n_layer=2, n_head=2, ffn=512, proj_dim=64, pad_id=5, ln_eps=1e-5,
             emb=P, proj_w=P, proj_b=P, layers=_layers())
    f.update(kw)
    _KEEP.append(f["layers"])
    return N.TextDesc(**f)


GOOD = dict(ids=P, B=2, L=16, out=P, hidden=None, ws=P, ws_bytes=BIG)

# (descriptor fields made bad, call arguments made bad, code, vcap_last_error() after "vcap_text_encode: ")
ROWS = [
    (None, {}, ARG, "text desc is null"),
    (dict(dtype=N.DT_F16), {}, ARG, "dtype must be VCAP_DT_F32 or VCAP_DT_BF16"),
    (dict(dtype=N.DT_MXFP8), {}, ARG, "dtype must be VCAP_DT_F32 or VCAP_DT_BF16"),
    (dict(dim=192), {}, UNSUP, "head_dim must be 64"),
    (dict(n_head=4), {}, UNSUP, "head_dim must be 64"),
    (dict(dim=0, n_head=0), {}, UNSUP, "head_dim must be 64"),
    (dict(dim=192, n_head=3), {}, UNSUP, "dim must be a multiple of 128"),
    (dict(dim=1152, n_head=18), {}, UNSUP, "dim > 1024 (LayerNorm rows are held in registers)"),
    (dict(ffn=192), {}, UNSUP, "ffn must be a multiple of 128 in 128..4096"),
    (dict(ffn=0), {}, UNSUP, "ffn must be a multiple of 128 in 128..4096"),
    (dict(ffn=4224), {}, UNSUP, "ffn must be a multiple of 128 in 128..4096"),
    (dict(proj_dim=96), {}, UNSUP, "proj_dim must be a multiple of 64 in 64..1024"),
    (dict(proj_dim=0), {}, UNSUP, "proj_dim must be a multiple of 64 in 64..1024"),
    (dict(proj_dim=1088), {}, UNSUP, "proj_dim must be a multiple of 64 in 64..1024"),
    (dict(pad_id=-1), {}, ARG, "pad_id must be inside the vocabulary"),
    (dict(pad_id=97), {}, ARG, "pad_id must be inside the vocabulary"),
    (dict(vocab=0, pad_id=0), {}, ARG, "pad_id must be inside the vocabulary"),
    (dict(n_layer=-1), {}, ARG, "n_layer < 0"),
    ({}, dict(B=0), ARG, "B must be at least 1"),
    ({}, dict(L=0), UNSUP, "L must be in 1..64"),
    ({}, dict(L=65), UNSUP, "L must be in 1..64"),
    ({}, dict(B=9, L=64), UNSUP, "B*L exceeds vcap_gpt2_max_rows()"),
    ({}, dict(B=513, L=1), UNSUP, "B*L exceeds vcap_gpt2_max_rows()"),
    ({}, dict(ids=None), ARG, "null pointer"),
    ({}, dict(out=None), ARG, "null pointer"),
    ({}, dict(ws=None), ARG, "null pointer"),
    (dict(emb=None), {}, ARG, "emb / proj / layers pointer is null"),
    (dict(proj_w=None), {}, ARG, "emb / proj / layers pointer is null"),
    (dict(proj_b=None), {}, ARG, "emb / proj / layers pointer is null"),
    (dict(layers=None), {}, ARG, "emb / proj / layers pointer is null"),
    (dict(layers=_layers(2, fc2_w=None)), {}, ARG, "layer 1 has a null pointer"),
    (dict(layers=_layers(2, ln1_g=None)), {}, ARG, "layer 1 has a null pointer"),
    (dict(emb=P + 4), {}, UNSUP, "emb, proj_w and the workspace must be 16-byte aligned"),
    (dict(proj_w=P + 8), {}, UNSUP, "emb, proj_w and the workspace must be 16-byte aligned"),
    ({}, dict(ws=P + 4), UNSUP, "emb, proj_w and the workspace must be 16-byte aligned"),
    ({}, dict(ws_bytes="short"), WS, "workspace too small (vcap_text_workspace_bytes)"),
]


def _call(desc_kw, args_kw):
    lib = N.lib()
    d = None if desc_kw is None else _desc(**desc_kw)
    a = dict(GOOD, **args_kw)
    if a["ws_bytes"] == "short":
        a["ws_bytes"] = int(lib.vcap_text_workspace_bytes(C.byref(d), a["B"], a["L"])) - 1
    rc = lib.vcap_text_encode(C.byref(d) if d is not None else None, a["ids"], a["B"], a["L"], a["out"], a["hidden"],
                              a["ws"], a["ws_bytes"], None)
    return rc, (lib.vcap_last_error() or b"").decode()


@pytest.mark.parametrize("desc_kw,args_kw,code,msg", ROWS,
                         ids=[f"{i}-{m[:28]}" for i, (_, _, _, m) in enumerate(ROWS)])
def test_refusals(desc_kw, args_kw, code, msg):
    rc, text = _call(desc_kw, args_kw)
    assert rc == code and text == "vcap_text_encode: " + msg, (rc, text)


def test_no_layers_needs_no_layer_array_to_pass_the_checks():
    """n_layer == 0 with layers == NULL passes every pointer check: the next refusal is the workspace's."""
    rc, text = _call(dict(n_layer=0, layers=None), dict(ws_bytes="short"))
    assert rc == WS, (rc, text)


def test_workspace_bytes():
    lib = N.lib()
    for dt, es in ((N.DT_F32, 4), (N.DT_BF16, 2)):
        d = _desc(dtype=dt)
        need = int(lib.vcap_text_workspace_bytes(C.byref(d), 2, 16))
        rows = 2 * 16
        assert need >= rows * (128 * 4 + (128 + 3 * 128 + 128 + 512) * es)     # x, xt, qkv, attn, act
        assert need <= 2 * rows * (128 * 4 + (128 + 3 * 128 + 128 + 512) * es)
        assert int(lib.vcap_text_workspace_bytes(C.byref(d), 8, 64)) > need
    d0 = _desc(n_layer=0, layers=None)
    assert int(lib.vcap_text_workspace_bytes(C.byref(d0), 1, 1)) > 0
    for bad_desc, B, L in ((dict(dim=192), 2, 16), (dict(ffn=100), 2, 16), (dict(proj_dim=32), 2, 16),
                           (dict(pad_id=200), 2, 16), (dict(dtype=N.DT_F16), 2, 16), ({}, 0, 16), ({}, 2, 0),
                           ({}, 2, 65), ({}, 9, 64)):
        assert int(lib.vcap_text_workspace_bytes(C.byref(_desc(**bad_desc)), B, L)) == 0
        assert lib.vcap_last_error().decode().startswith("vcap_text_workspace_bytes: ")
    assert int(lib.vcap_text_workspace_bytes(None, 2, 16)) == 0


def test_bindings_cover_the_header():
    text = (Path(TC.__file__).resolve().parents[1] / "include" / "vcap.h").read_text()
    lib = N.lib()
    for name in ("vcap_text_workspace_bytes", "vcap_text_encode"):
        assert name in N.SIGNATURES and name + "(" in text and hasattr(lib, name)
    assert "#define VCAP_ABI_VERSION 16" in text and N.ABI_VERSION == 16
    # the ctypes structs name the header's fields in the header's order
    for struct, ctype in (("vcap_text_layer", N.TextLayer), ("vcap_text_desc", N.TextDesc)):
        body = re.sub(r"/\*.*?\*/", "", text.split("typedef struct " + struct + " {")[1].split("} " + struct)[0],
                      flags=re.S)
        assert re.findall(r"(\w+)\s*[,;]", body) == [f for f, _ in ctype._fields_]


def test_host_ids_are_range_checked_and_long_captions_raise():
    emb = R.HipTextEmbedder.__new__(R.HipTextEmbedder)     # _ids needs no device state but these two
    emb.vocab, emb.device = 97, "cpu"
    with pytest.raises(ValueError, match="outside"):
        emb._ids([[1, 2, 97]])
    with pytest.raises(ValueError, match="outside"):
        emb._ids(np.array([-1, 2]))
    with pytest.raises(ValueError, match="at most 64"):
        emb._ids(np.zeros((1, 65), np.int64))
    with pytest.raises(ValueError, match="integers"):
        emb._ids(np.zeros((1, 4), np.float32))
    assert tuple(emb._ids([1, 2, 3]).shape) == (1, 3)


def test_from_state_dict_refuses_a_head_width_other_than_64():
    with pytest.raises(ValueError, match="dim / nhead must be 64"):
        R.HipTextEmbedder.from_state_dict(TC.state_dict("e128"), TC.PAD_ID["e128"], nhead=8, device="cpu")
    with pytest.raises(ValueError, match="pad_id"):
        R.HipTextEmbedder.from_state_dict(TC.state_dict("e128"), 97, nhead=2, device="cpu")
