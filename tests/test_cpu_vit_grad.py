"""CPU side of the ViT encoder's backward: the fp64 oracle of tests/vit_grad_cases.py against central finite
differences, the bf16 emulation with its roundings switched off against the oracle, the refusals of
vcap_vit_encode_backward / vcap_vit_attention_backward that return before any device call (through the C ABI, as
test_cpu_abi_refusals.py calls it), scripts.train_full's parser and up-front refusals, and the vit.* <->
encoder.backbone.* name mapping."""
import ctypes as C

import numpy as np
import pytest
import torch

import vit_grad_cases as VG
from oracle import vcap_oracle as O
from vcap import _native as N

ARG, WS, UNSUP = N.E_ARG, N.E_WORKSPACE, N.E_UNSUPPORTED


# ---- the oracle
def test_oracle_gradients_agree_with_central_differences():
    name = "G1"
    c = VG.CASES[name]
    sd, video, G = VG.weights(name), VG.frames(name).double(), VG.grad_out(name).double()
    g64 = VG.grads_of(name, "fp64")

    def scalar(p):
        # oracle.encoder's own lines without its closing .float(), whose float32 rounding of enc_out
        # (~1e-7 |out|) divided by 2 h would drown the difference quotient
        feat = O.vit_forward_features(p, c.arch, video.reshape(c.B * c.T, *video.shape[2:]))
        pooled = O.cls_temporal_pool(feat, c.B, c.T)
        out = torch.nn.functional.linear(pooled, p["encoder.proj.weight"], p["encoder.proj.bias"])
        return float((G * out).sum())

    p0 = {n: torch.from_numpy(np.ascontiguousarray(v)).double() for n, v in sd.items()}
    assert abs(scalar(p0) - float((G * O.encoder(p0, c.arch, video).double()).sum())) <= 1e-4
    rng = np.random.default_rng(0)
    h = 1e-5
    for k, g in g64.items():
        flat = g.reshape(-1)
        for idx in rng.choice(flat.numel(), size=min(3, flat.numel()), replace=False):
            p = {n: torch.from_numpy(np.ascontiguousarray(v)).double().clone() for n, v in sd.items()}
            p[k].reshape(-1)[idx] += h
            up = scalar(p)
            p[k].reshape(-1)[idx] -= 2 * h
            fd = (up - scalar(p)) / (2 * h)
            # fp64: truncation ~ h^2 f''' and rounding ~ 1e-16 |scalar| / h, both far below 1e-6 of the tensor's scale
            assert abs(fd - float(flat[idx])) <= 1e-6 * float(g.abs().max()) + 1e-9, (k, int(idx), fd, float(flat[idx]))


@pytest.mark.parametrize("name", ["G1", "G2", "G5"])
def test_the_emulation_with_identity_rounding_reproduces_the_oracle(name):
    g64, re = VG.grads_of(name, "fp64"), VG.grads_of(name, "restated")
    assert g64.keys() == re.keys()
    for k in g64:
        assert VG.err(re[k], g64[k]) <= 1e-11, (k, VG.err(re[k], g64[k]))


def test_attention_formulas_are_autograd_of_softmax_attention():
    g = torch.Generator().manual_seed(1)
    q, k, v, dO = (torch.randn(2, 3, 33, 64, generator=g, dtype=torch.float64) for _ in range(4))
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = torch.softmax(qa @ ka.transpose(-1, -2) / 8.0, -1) @ va
    want = torch.autograd.grad((out * dO).sum(), (qa, ka, va))
    o, dq, dk, dv = VG.attention_formulas(q, k, v, dO)
    assert torch.allclose(o, out.detach(), atol=1e-13)
    for a, b in zip((dq, dk, dv), want):
        assert torch.allclose(a, b, atol=1e-12)


def test_every_bound_is_positive_or_an_exact_tensor():
    """The bf16 emulation must differ from the oracle wherever the device meets a rounding; only tensors that
    meet none may have a zero bound: encoder.proj.bias and the final norm's bias, whose gradients are functions
    of grad_out and encoder.proj.weight alone."""
    for prec in VG.PRECISIONS:
        tol = VG.tolerances("G1", prec)
        zero = sorted(k for k, v in tol.items() if v == 0.0)
        assert zero == ([] if prec == "f32" else ["encoder.backbone.norm.bias", "encoder.proj.bias"]), (prec, zero)


# ---- refusals before any device call
_BUF = C.create_string_buffer(8192)
P = (C.addressof(_BUF) + 255) & ~255          # a 256-byte aligned non-null address no refused call reads
_VLAYERS = (N.VitLayer * 2)()
_GLAYERS = (N.VitGradLayer * 2)()
_PLAYERS = (N.VitParamGradsLayer * 2)()
for _l in list(_GLAYERS) + list(_PLAYERS):
    for _f, _ in _l._fields_:
        setattr(_l, _f, P)
BIG = 1 << 40


def _vit(**kw):
    f = dict(dtype=N.DT_F32, dim=128, depth=2, heads=2, patch=16, image=224, mlp=512, video_dim=256, kpad=768,
             ln_eps=1e-6, patch_w=P, patch_b=P, cls=P, pos=P, norm_g=P, norm_b=P, proj_w=P, proj_b=P, layers=_VLAYERS)
    f.update(kw)
    return N.VitDesc(**f)


def _gdesc(**kw):
    f = dict(dtype=N.DT_F32, dim=128, mlp=512, depth=2, layers=_GLAYERS)
    f.update(kw)
    return N.VitGradDesc(**f)


def _grads(**kw):
    f = dict(proj_w=P, proj_b=P, norm_g=P, norm_b=P, patch_w=P, patch_b=P, cls=P, pos=P, layers=_PLAYERS)
    f.update(kw)
    return N.VitParamGrads(**f)


def _call(desc=None, gdesc=None, frames=P, B=1, T=1, n_tail=1, grad_out=P, enc_out=P, grads=None, ws=P, ws_bytes=BIG):
    desc = _vit() if desc is None else desc
    gdesc = _gdesc() if gdesc is None else gdesc
    grads = _grads() if grads is None else grads
    rc = N.lib().vcap_vit_encode_backward(C.byref(desc), C.byref(gdesc), frames, B, T, n_tail, grad_out, enc_out,
                                          C.byref(grads), ws, ws_bytes, None)
    return rc, (N.lib().vcap_last_error() or b"").decode()


REFUSALS = [
    ("n_tail 0", dict(n_tail=0), ARG, "n_tail outside 1 .. depth"),
    ("n_tail past depth", dict(n_tail=3), ARG, "n_tail outside 1 .. depth"),
    ("B 0", dict(B=0), ARG, "B and T must be positive"),
    ("null frames", dict(frames=None), ARG, "null pointer"),
    ("null grad_out", dict(grad_out=None), ARG, "null pointer"),
    ("null enc_out", dict(enc_out=None), ARG, "null pointer"),
    ("null workspace", dict(ws=None), ARG, "null pointer"),
    ("null head gradient", dict(grads=_grads(norm_g=None)), ARG, "a head gradient pointer is null"),
    ("null patch gradient at full depth", dict(n_tail=2, grads=_grads(pos=None)), ARG, "n_tail == depth needs"),
    ("fp16 operands", dict(desc=_vit(dtype=N.DT_F16), gdesc=_gdesc(dtype=N.DT_F16)), UNSUP, "operand dtype must be"),
    ("mxfp8 operands", dict(desc=_vit(dtype=N.DT_MXFP8, dim=256, heads=4, mlp=1024, kpad=768),
                            gdesc=_gdesc(dtype=N.DT_MXFP8, dim=256, mlp=1024)), UNSUP, "operand dtype must be"),
    ("width 64", dict(desc=_vit(dim=64, heads=1, mlp=256), gdesc=_gdesc(dim=64, mlp=256)), UNSUP,
     "multiples of 128"),
    ("mlp 192", dict(desc=_vit(mlp=192), gdesc=_gdesc(mlp=192)), UNSUP, "multiples of 128"),
    ("grad desc dtype differs", dict(gdesc=_gdesc(dtype=N.DT_BF16)), ARG, "differ from the vit desc"),
    ("grad desc depth differs", dict(gdesc=_gdesc(depth=3)), ARG, "differ from the vit desc"),
    ("more than 65535 (frame, head) pairs", dict(B=40000), UNSUP, "B * T * heads > 65535"),
    ("more than 2^22 rows", dict(B=150, T=150), UNSUP, "B * T * tokens > 2^22"),
    ("short workspace", dict(ws_bytes=4096), WS, "workspace too small"),
    ("misaligned workspace", dict(ws=P + 8), UNSUP, "256-byte aligned"),
]


@pytest.mark.parametrize("what,kw,code,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_encode_backward_refusals_return_before_any_device_call(what, kw, code, text):
    rc, msg = _call(**kw)
    assert rc == code, (rc, msg)
    assert text in msg, msg


def test_the_workspace_query_is_zero_outside_the_limits():
    q = N.lib().vcap_vit_backward_workspace_bytes
    assert q(C.byref(_vit()), 1, 1, 1) > 0
    assert q(C.byref(_vit()), 1, 1, 2) > q(C.byref(_vit()), 1, 1, 1)
    for d, B, T, n in ((_vit(), 1, 1, 0), (_vit(), 1, 1, 3), (_vit(), 0, 1, 1), (_vit(dtype=N.DT_F16), 1, 1, 1),
                       (_vit(dim=64, heads=1, mlp=256), 1, 1, 1), (_vit(), 40000, 1, 1), (_vit(), 150, 150, 1)):
        assert q(C.byref(d), B, T, n) == 0


ATTN_REFUSALS = [
    ("null qkv", dict(qkv=None), ARG), ("null dout", dict(dout=None), ARG), ("null dqkv", dict(dqkv=None), ARG),
    ("null workspace", dict(ws=None), ARG), ("no frames", dict(frames=0), ARG), ("no tokens", dict(tokens=0), ARG),
    ("289 tokens", dict(tokens=289), UNSUP), ("fp16", dict(dtype=N.DT_F16), UNSUP), ("mxfp8", dict(dtype=N.DT_MXFP8), UNSUP),
    ("misaligned qkv", dict(qkv=P + 4), UNSUP), ("65536 (frame, head) pairs", dict(frames=16384, heads=4), UNSUP),
]


@pytest.mark.parametrize("what,kw,code", ATTN_REFUSALS, ids=[r[0] for r in ATTN_REFUSALS])
def test_attention_backward_refusals_return_before_any_device_call(what, kw, code):
    f = dict(dtype=N.DT_F32, qkv=P, dout=P, dqkv=P, frames=1, tokens=4, heads=1, ws=P)
    f.update(kw)
    rc = N.lib().vcap_vit_attention_backward(f["dtype"], f["qkv"], f["dout"], f["dqkv"], f["frames"], f["tokens"],
                                             f["heads"], f["ws"], None)
    assert rc == code, (rc, N.lib().vcap_last_error())


# ---- the CLI's parser and up-front refusals; the name mapping
def test_train_full_parser_and_refusals():
    from scripts.train_full import build_argparser, check_args, frozen_argv
    ap = build_argparser()
    a = ap.parse_args(["--model", "vit"])
    check_args(a)
    assert a.unfreeze_vit_last == 0 and a.freeze_vit is False and a.precision == "bf16"
    check_args(ap.parse_args(["--model", "vit", "--unfreeze_vit_last", "2", "--precision", "fp32"]))
    check_args(ap.parse_args(["--model", "vit", "--freeze_vit", "--precision", "fp16"]))   # frozen: train_align's business
    with pytest.raises(SystemExit, match="simple"):
        check_args(ap.parse_args(["--model", "simple"]))
    with pytest.raises(SystemExit, match="fp16"):
        check_args(ap.parse_args(["--model", "vit", "--precision", "fp16"]))
    with pytest.raises(SystemExit, match="fp8"):
        check_args(ap.parse_args(["--model", "vit", "--precision", "fp8"]))
    with pytest.raises(SystemExit, match="unfreeze_vit_last"):
        check_args(ap.parse_args(["--model", "vit", "--unfreeze_vit_last", "-1"]))
    with pytest.raises(SystemExit, match="max_len"):
        check_args(ap.parse_args(["--model", "vit", "--max_len", "65"]))
    for flag in ("ann_train", "ann_val", "batch_size", "num_frame", "max_len", "lr", "epochs", "max_steps", "val_every",
                 "run_dir", "ckpt_dir", "ckpt_name", "freeze_vit", "vit_name", "image_size", "seed"):
        assert hasattr(a, flag), flag
    assert frozen_argv(["--freeze_vit", "--unfreeze_vit_last", "3", "--lr", "1e-3", "--unfreeze_vit_last=2"]) == [
        "--freeze_vit", "--lr", "1e-3"]


def test_train_full_with_freeze_vit_delegates_to_train_align(monkeypatch):
    from scripts import train_align, train_full
    seen = []
    monkeypatch.setattr(train_align, "main", lambda argv=None: seen.append(list(argv)) or 0)
    assert train_full.main(["--model", "vit", "--freeze_vit", "--unfreeze_vit_last", "1", "--epochs", "3"]) == 0
    assert seen == [["--model", "vit", "--freeze_vit", "--epochs", "3"]]


def test_the_vit_name_mapping_round_trips():
    from vcap.retrieval import remap_alignment_state_dict
    from vcap.train_align import align_param_name, encoder_param_name
    sd = VG.weights("G1")
    aligned = {align_param_name(k): v for k, v in sd.items()}
    assert all(k.startswith(("vit.", "vid_proj.")) for k in aligned)
    assert {"vit.cls_token", "vit.blocks.1.attn.qkv.weight", "vit.norm.bias", "vid_proj.weight"} <= set(aligned)
    assert {encoder_param_name(k) for k in aligned} == set(sd)
    back = remap_alignment_state_dict(aligned)
    assert set(back) == set(sd) and all(np.array_equal(back[k], sd[k]) for k in sd)
    assert VG.param_names(VG.CASES["G1"].arch, 2) and set(VG.param_names(VG.CASES["G1"].arch, 2)) == set(sd)
    with pytest.raises(KeyError):
        align_param_name("txt_proj.weight")
    with pytest.raises(KeyError):
        encoder_param_name("txt_proj.weight")
