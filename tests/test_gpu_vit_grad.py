"""The ViT encoder's backward on the GPU (vcap_vit_encode_backward through HipViTEncoder.encode_backward, and
vcap_vit_attention_backward alone) against the fp64 autograd oracle of tests/vit_grad_cases.py, in both operand
dtypes.

Bounds (derived in vit_grad_cases.py, CPU quantities of the case and tensor): f32 <= 10 x the error of torch
float32 autograd, bf16 <= 3 x the error of the fp64 emulation that rounds where the device rounds.  A tensor
whose oracle is identically zero must be exact +0.  A tensor whose bf16 emulation error is exactly 0 meets no
bf16 rounding at all (encoder.proj.bias and the final norm's bias: functions of grad_out and encoder.proj.weight
alone): there the bound 3 x 0 is asked in the only form f32 arithmetic can meet - the bf16 call must give the
f32 call's bits, which are held to the f32 bound.  Where float32 autograd itself is exact (a one-term sum:
encoder.proj.bias of a one-video call, dV of a one-token attention) the bound 10 x 0 is asked as it stands: the
device must equal the oracle.  Every test prints its figures before it asserts.
"""
import ctypes as C
from functools import lru_cache

import pytest
import torch

import vit_grad_cases as VG
from vcap import _native as N
from vcap.model import HipViTEncoder

pytestmark = pytest.mark.gpu
DTYPES = list(VG.PRECISIONS)
_PREC = {"f32": "fp32", "bf16": "bf16"}
_DT = {"f32": (N.DT_F32, torch.float32), "bf16": (N.DT_BF16, torch.bfloat16)}


def _new_encoder(name: str, dtype: str, sd=None) -> HipViTEncoder:
    c = VG.CASES[name]
    sd = VG.weights(name) if sd is None else sd
    enc = HipViTEncoder(sd, c.arch, _PREC[dtype], "cuda:0", video_dim=VG.VIDEO_DIM)
    enc.enable_grad(sd, c.depth)
    return enc


@lru_cache(maxsize=None)
def _encoder(name: str, dtype: str) -> HipViTEncoder:
    return _new_encoder(name, dtype)


def _host(grads):
    return {k: v.cpu() for k, v in grads.items()}


def _backward(name, dtype, video, G, n_tail, chunk=None, enc=None):
    enc = _encoder(name, dtype) if enc is None else enc
    out, grads = enc.encode_backward(video.to("cuda:0"), G.to("cuda:0"), n_tail, chunk=chunk)
    torch.cuda.synchronize()
    return out.cpu(), _host(grads)


@lru_cache(maxsize=None)
def _case_backward(name, dtype, n_tail):
    return _backward(name, dtype, VG.frames(name), VG.grad_out(name), n_tail)


def _bits(t: torch.Tensor) -> bytes:
    return t.contiguous().numpy().tobytes()


def _same_bits(a, b) -> bool:
    return a.keys() == b.keys() and all(_bits(a[k]) == _bits(b[k]) for k in a)


def _check_against_oracle(tag, grads, g64s, tol, f32_grads=None):
    worst, failed = 0.0, []
    for k, g in grads.items():
        g64 = g64s[k]
        assert g.dtype == torch.float32 and g.shape == g64.shape, k
        if VG.is_zero_tensor(g64):
            ok = bool(VG.is_plus_zero(g).all())
            print(f"{tag} {k} oracle zero: exact +0 {ok}")
        elif tol[k] == 0.0 and f32_grads is None:
            ok = VG.err(g, g64) == 0.0   # float32 autograd is exact here (a one-term sum): so must the device be
            print(f"{tag} {k} float32 autograd is exact: equal to the oracle {ok}")
        elif tol[k] == 0.0:
            ok = _bits(g) == _bits(f32_grads[k])
            print(f"{tag} {k} no bf16 rounding point: bits of the f32 call {ok}")
        else:
            e = VG.err(g, g64)
            ok = e <= tol[k]
            worst = max(worst, e / tol[k])
            print(f"{tag} {k} err {e:.3e} bound {tol[k]:.3e} ratio {e / tol[k]:.3f}")
        if not ok:
            failed.append(k)
    print(f"{tag} worst err / bound {worst:.3f}")
    assert not failed, failed


# ---- 1. the oracle: every case x dtype x n_tail, every returned tensor
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,n_tail", VG.RUNS, ids=[f"{n}-tail{k}" for n, k in VG.RUNS])
def test_gradients_match_the_fp64_oracle(device, name, n_tail, dtype):
    _, grads = _case_backward(name, dtype, n_tail)
    assert sorted(grads) == sorted(VG.param_names(VG.CASES[name].arch, n_tail))
    f32 = _case_backward(name, "f32", n_tail)[1] if dtype == "bf16" else None
    _check_against_oracle(f"VIT_GRAD {dtype} {name} n_tail={n_tail}", grads, VG.grads_of(name, "fp64"),
                          VG.tolerances(name, dtype), f32)


# ---- 2. the attention backward alone, at token counts the forward's windows do not reach
def _attention_backward(dtype, qkv, dout, tokens, heads, nframes):
    dt, tdt = _DT[dtype]
    lib = N.lib()
    q = qkv.to("cuda:0").to(tdt).contiguous()
    do = dout.to("cuda:0").contiguous()
    dqkv = torch.full((nframes * tokens, 3 * 64 * heads), float("nan"), dtype=torch.float32, device="cuda:0")
    ws = torch.empty(int(lib.vcap_vit_attention_backward_workspace_bytes(dt, nframes, tokens, heads)),
                     dtype=torch.uint8, device="cuda:0")
    N.check(lib.vcap_vit_attention_backward(dt, q.data_ptr(), do.data_ptr(), dqkv.data_ptr(), nframes, tokens, heads,
                                            ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
            "vcap_vit_attention_backward")
    torch.cuda.synchronize()
    return dqkv.cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nframes", VG.ATTN_FRAMES)
@pytest.mark.parametrize("heads", VG.ATTN_HEADS)
@pytest.mark.parametrize("tokens", VG.ATTN_TOKENS)
def test_attention_backward_alone(device, tokens, heads, nframes, dtype):
    qkv, dout = VG.attn_inputs(tokens, heads, nframes, dtype)
    g64, bound = VG.attn_bounds(tokens, heads, nframes, dtype)
    got = _attention_backward(dtype, qkv, dout, tokens, heads, nframes)
    failed = []
    for k, g, t64 in zip(("dq", "dk", "dv"), VG.split3(got, heads), VG.split3(g64, heads)):
        if VG.is_zero_tensor(t64):   # one token: P = 1, dS = 0
            ok = bool(VG.is_plus_zero(g).all())
            print(f"VIT_ATTN_BWD {dtype} N={tokens} H={heads} F={nframes} {k} oracle zero: exact +0 {ok}")
        elif bound[k] == 0.0:   # one token: dV = dO, which the CPU reference forms exactly - so must the device
            ok = VG.err(g, t64) == 0.0
            print(f"VIT_ATTN_BWD {dtype} N={tokens} H={heads} F={nframes} {k} reference exact: equal to the oracle {ok}")
        else:
            e = VG.err(g, t64)
            ok = e <= bound[k]
            print(f"VIT_ATTN_BWD {dtype} N={tokens} H={heads} F={nframes} {k} err {e:.3e} bound {bound[k]:.3e} "
                  f"ratio {e / bound[k]:.3f}")
        if not ok:
            failed.append(k)
    assert not failed, failed


# ---- 3. the forward's bits, no state
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,n_tail", [("G1", 2), ("G3", 1), ("G3", 3), ("G4", 1), ("G5", 2)])
def test_enc_out_has_encodes_bits_and_the_backward_leaves_no_state(device, name, n_tail, dtype):
    enc, video = _encoder(name, dtype), VG.frames(name).to("cuda:0")
    before = enc.encode(video)[0].cpu()
    out, _ = _backward(name, dtype, VG.frames(name), VG.grad_out(name), n_tail)
    after = enc.encode(video)[0].cpu()
    assert _bits(before) == _bits(out) == _bits(after)


# ---- 4. determinism
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["G1", "G3", "G5"])
def test_two_calls_and_a_cu_masked_stream_give_the_same_bits(device, name, dtype):
    n_tail = VG.CASES[name].depth
    video, G = VG.frames(name), VG.grad_out(name)
    o1, g1 = _backward(name, dtype, video, G, n_tail)
    o2, g2 = _backward(name, dtype, video, G, n_tail)
    assert _bits(o1) == _bits(o2) and _same_bits(g1, g2)
    h = C.c_void_p()
    N.check(N.lib().vcap_stream_create_cu_reserved(32, C.byref(h)), "masked stream")
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.ExternalStream(h.value, device=device)):
            o3, g3 = _backward(name, dtype, video, G, n_tail)
    finally:
        torch.cuda.synchronize()
        N.check(N.lib().vcap_stream_destroy(h), "stream destroy")
    assert _bits(o1) == _bits(o3) and _same_bits(g1, g3)


# ---- 5. linearity and exact zeros
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["G1", "G3", "G5"])
def test_doubling_grad_out_doubles_every_gradient_exactly(device, name, dtype):
    n_tail = VG.CASES[name].depth
    _, g1 = _case_backward(name, dtype, n_tail)
    _, g2 = _backward(name, dtype, VG.frames(name), 2 * VG.grad_out(name), n_tail)
    for k in g1:
        assert _bits(2 * g1[k]) == _bits(g2[k]), k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["G1", "G3", "G4"])
def test_a_zero_grad_out_gives_plus_zero_everywhere(device, name, dtype):
    n_tail = VG.CASES[name].depth
    _, g = _backward(name, dtype, VG.frames(name), torch.zeros_like(VG.grad_out(name)), n_tail)
    bad = [k for k, v in g.items() if not bool(VG.is_plus_zero(v).all())]
    assert not bad, bad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["G1", "G3", "G5"])
def test_appending_a_video_with_a_zero_grad_out_row_changes_no_bit(device, name, dtype):
    c = VG.CASES[name]
    video, G = VG.frames(name), VG.grad_out(name)
    extra = torch.randn(1, c.T, 3, c.image, c.image, generator=torch.Generator().manual_seed(5))
    _, g1 = _case_backward(name, dtype, c.depth)
    _, g2 = _backward(name, dtype, torch.cat([video, extra]), torch.cat([G, torch.zeros(1, VG.VIDEO_DIM)]), c.depth,
                      chunk=c.B + 1)
    bad = [k for k in g1 if _bits(g1[k]) != _bits(g2[k])]
    assert not bad, bad


# ---- 6. the tail
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 2])
def test_a_shorter_tail_returns_the_same_bits_and_no_frozen_parameter(device, k, dtype):
    _, full = _case_backward("G3", dtype, 3)
    _, part = _case_backward("G3", dtype, k)
    assert sorted(part) == sorted(VG.param_names(VG.CASES["G3"].arch, k))
    frozen = [n for n in part if any(f".blocks.{i}." in n for i in range(3 - k))] + [
        n for n in part if "patch_embed" in n or n.endswith("cls_token") or n.endswith("pos_embed")]
    assert not frozen, frozen
    bad = [n for n in part if _bits(part[n]) != _bits(full[n])]
    assert not bad, bad


# ---- 7. chunking
@pytest.mark.parametrize("dtype", DTYPES)
def test_three_clips_in_chunks_of_two_and_one(device, dtype):
    name = "G5"   # B = 3
    c = VG.CASES[name]
    video, G = VG.frames(name), VG.grad_out(name)
    o, g = _backward(name, dtype, video, G, c.depth, chunk=2)
    oa, ga = _backward(name, dtype, video[:2], G[:2], c.depth)
    ob, gb = _backward(name, dtype, video[2:], G[2:], c.depth)
    assert _bits(o) == _bits(torch.cat([oa, ob]))
    bad = [k for k in g if _bits(g[k]) != _bits(ga[k] + gb[k])]
    assert not bad, bad
    f32 = _backward(name, "f32", video, G, c.depth, chunk=2)[1] if dtype == "bf16" else None
    _check_against_oracle(f"VIT_GRAD_CHUNKS {dtype} {name}", g, VG.grads_of(name, "fp64"), VG.tolerances(name, dtype),
                          f32)


# ---- 8. load_state_dict refreshes in place
@pytest.mark.parametrize("dtype", DTYPES)
def test_load_state_dict_keeps_the_pointers_and_matches_a_fresh_encoder(device, dtype):
    name = "G1"
    sd = VG.weights(name)
    enc = _new_encoder(name, dtype)
    ptrs = {k: v.data_ptr() for k, v in enc._device_params().items()}
    gptrs = {k: v.data_ptr() for k, v in enc._grad_keep.items()}
    g = torch.Generator().manual_seed(3)
    new = {k: (torch.from_numpy(v) + 0.01 * torch.randn(v.shape, generator=g)).numpy() for k, v in sd.items()}
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()})
    assert ptrs == {k: v.data_ptr() for k, v in enc._device_params().items()}
    assert gptrs == {k: v.data_ptr() for k, v in enc._grad_keep.items()}
    fresh = _new_encoder(name, dtype, new)
    video = VG.frames(name).to("cuda:0")
    assert _bits(enc.encode(video)[0].cpu()) == _bits(fresh.encode(video)[0].cpu())
    G = VG.grad_out(name)
    _, g1 = _backward(name, dtype, VG.frames(name), G, 2, enc=enc)
    _, g2 = _backward(name, dtype, VG.frames(name), G, 2, enc=fresh)
    assert _same_bits(g1, g2)


# ---- 9. refusals: documented codes, outputs untouched
def _raw_call(enc, video, G, n_tail, *, desc=None, grad_desc=None, ws_bytes=None, grad_out_ptr=None):
    c = enc.arch
    B, T = video.shape[:2]
    names = enc.param_names(min(max(n_tail, 1), c.depth))
    g = {k: torch.full(enc._param_shape(k), 7.0, dtype=torch.float32, device="cuda:0") for k in names}
    pw = torch.full((c.dim, enc.kpad), 7.0, dtype=torch.float32, device="cuda:0")
    nt = min(max(n_tail, 1), c.depth)
    layers = (N.VitParamGradsLayer * nt)()
    p = "encoder.backbone."
    for j, i in enumerate(range(c.depth - nt, c.depth)):
        for key, field in enc._BLOCK_FIELDS:
            setattr(layers[j], field, g[f"{p}blocks.{i}.{key}"].data_ptr())
    pg = N.VitParamGrads(proj_w=g["encoder.proj.weight"].data_ptr(), proj_b=g["encoder.proj.bias"].data_ptr(),
                         norm_g=g[p + "norm.weight"].data_ptr(), norm_b=g[p + "norm.bias"].data_ptr(),
                         patch_w=pw.data_ptr(), patch_b=N.ptr(g.get(p + "patch_embed.proj.bias")),
                         cls=N.ptr(g.get(p + "cls_token")), pos=N.ptr(g.get(p + "pos_embed")), layers=layers)
    out = torch.full((B, enc.video_dim), 7.0, dtype=torch.float32, device="cuda:0")
    full = enc.backward_workspace_bytes(B, T, nt)
    ws = torch.empty(max(full, 1), dtype=torch.uint8, device="cuda:0")
    rc = N.lib().vcap_vit_encode_backward(C.byref(enc.desc if desc is None else desc),
                                          C.byref(enc.grad_desc if grad_desc is None else grad_desc),
                                          video.data_ptr(), B, T, n_tail,
                                          G.data_ptr() if grad_out_ptr is None else grad_out_ptr, out.data_ptr(),
                                          C.byref(pg), ws.data_ptr(), full if ws_bytes is None else ws_bytes,
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    untouched = all(bool((t == 7.0).all()) for t in list(g.values()) + [pw, out])
    return rc, untouched


def _copy_desc(src, cls, **kw):
    d = cls()
    C.memmove(C.byref(d), C.byref(src), C.sizeof(cls))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("what,code", [("n_tail_zero", N.E_ARG), ("n_tail_past_depth", N.E_ARG),
                                       ("null_grad_out", N.E_ARG), ("short_workspace", N.E_WORKSPACE),
                                       ("f16", N.E_UNSUPPORTED), ("mxfp8", N.E_UNSUPPORTED),
                                       ("grad_desc_dtype", N.E_ARG)])
def test_refusals_give_the_documented_codes_and_write_nothing(device, what, code):
    enc = _encoder("G1", "bf16")
    video, G = VG.frames("G1").to("cuda:0"), VG.grad_out("G1").to("cuda:0")
    kw, n_tail = {}, 2
    if what == "n_tail_zero":
        n_tail = 0
    elif what == "n_tail_past_depth":
        n_tail = 3
    elif what == "null_grad_out":
        kw["grad_out_ptr"] = 0
    elif what == "short_workspace":
        kw["ws_bytes"] = enc.backward_workspace_bytes(2, 3, 2) - 1
    elif what == "f16":
        kw["desc"] = _copy_desc(enc.desc, N.VitDesc, dtype=N.DT_F16)
    elif what == "mxfp8":
        kw["desc"] = _copy_desc(enc.desc, N.VitDesc, dtype=N.DT_MXFP8, dim=256, heads=4, mlp=1024)
    elif what == "grad_desc_dtype":
        kw["grad_desc"] = _copy_desc(enc.grad_desc, N.VitGradDesc, dtype=N.DT_F32)
    rc, untouched = _raw_call(enc, video, G, n_tail, **kw)
    print(f"VIT_GRAD_REFUSAL {what}: rc {rc}, outputs untouched {untouched}")
    assert rc == code and untouched


def test_attention_backward_refusals(device):
    lib = N.lib()
    buf = torch.full((64,), 7.0, dtype=torch.float32, device="cuda:0")
    p = buf.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    assert lib.vcap_vit_attention_backward(N.DT_F32, p, p, p, 1, 289, 1, p, s) == N.E_UNSUPPORTED
    assert lib.vcap_vit_attention_backward(N.DT_F16, p, p, p, 1, 4, 1, p, s) == N.E_UNSUPPORTED
    assert lib.vcap_vit_attention_backward(N.DT_F32, 0, p, p, 1, 4, 1, p, s) == N.E_ARG
    assert lib.vcap_vit_attention_backward(N.DT_F32, p, p, p, 0, 4, 1, p, s) == N.E_ARG
    assert lib.vcap_vit_attention_backward_workspace_bytes(N.DT_F32, 1, 289, 1) == 0
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())


# ---- 10. end to end: the autograd Function, the trainer, the checkpoint, the CLI
def _align_setup(dtype):
    import text_tower_cases as TC
    from vcap import retrieval as R
    from vcap.train_align import align_param_name
    from vcap.weights import synthetic_vit
    name, c = "e128", VG.CASES["G1"]
    P = TC.TOWERS[name][4]
    vit = synthetic_vit(5, c.arch, video_dim=P)
    sd = {**TC.state_dict(name), **{align_param_name(k): v for k, v in vit.items()}}
    enc = HipViTEncoder(R.remap_alignment_state_dict(sd), c.arch, _PREC[dtype], "cuda:0", video_dim=P)
    emb = R.HipTextEmbedder.from_state_dict(sd, TC.PAD_ID[name], TC.TOWERS[name][1], dtype, "cuda:0")
    ids = TC.ids_of(TC.Case(name, c.B, 12, ("none", "trailing")))
    return sd, enc, emb, ids, VG.frames("G1").to("cuda:0")


@pytest.mark.parametrize("dtype", DTYPES)
def test_encode_video_and_encode_text_reach_every_parameter_under_the_cosine_loss(device, dtype):
    from vcap.train_align import AlignTrainer
    sd, enc, emb, ids, video = _align_setup(dtype)
    tr = AlignTrainer(emb, sd, video_encoder=enc)
    assert tr.vit_n_tail == 2 and set(tr.vit_names) == set(enc.param_names(2))
    loss = tr.loss(video, ids)
    loss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad for k, p in zip(tr.vit_names + tr.names, tr.vit_params + tr.params)}
    missing = [k for k, g in got.items() if g is None or not bool(torch.isfinite(g).all()) or not bool(g.any())]
    print(f"VIT_TRAIN_LOSS {dtype} loss {float(loss):.8f}, {len(got)} parameters, unreached {missing}")
    assert not missing, missing


@pytest.mark.parametrize("dtype", DTYPES)
def test_twenty_steps_lower_the_loss_and_the_checkpoint_reloads(device, dtype, tmp_path):
    import text_tower_cases as TC
    from vcap import retrieval as R
    from vcap.train_align import AlignTrainer
    sd, enc, emb, ids, video = _align_setup(dtype)
    tr = AlignTrainer(emb, sd, lr=5e-4, video_encoder=enc, unfreeze_vit_last=0)
    before = tr.evaluate(video, ids)
    losses = [tr.step(video, ids) for _ in range(20)]
    after = tr.evaluate(video, ids)
    print(f"VIT_TRAIN {dtype} loss before {before:.6f} after 20 steps {after:.6f} (first step {losses[0]:.6f})")
    assert losses[0] == before and after < before and tr.steps == 20
    state = tr.state_dict()
    assert set(state) == set(sd) and all(v.device.type == "cpu" for v in state.values())
    moved = [k for k in state if k.startswith("vit.") and not torch.equal(state[k], torch.from_numpy(sd[k]))]
    assert len(moved) == len([k for k in sd if k.startswith("vit.")]), "every vit.* tensor trains with every block unfrozen"
    path = tmp_path / "align.pt"
    torch.save({"model_state": state}, path)
    loaded = torch.load(path, map_location="cpu", weights_only=True)
    c = VG.CASES["G1"]
    model = R.HipAlignModel(
        R.HipVideoEmbedder.from_state_dict(loaded, c.arch, _PREC[dtype], "cuda:0", video_dim=enc.video_dim),
        R.HipTextEmbedder.from_state_dict(loaded, TC.PAD_ID["e128"], TC.TOWERS["e128"][1], dtype, "cuda:0"))
    assert _bits(model.video_embedder.encoder.encode(video)[0].cpu()) == _bits(enc.encode(video)[0].cpu())
    again = float(model(video, ids))
    print(f"VIT_TRAIN {dtype} reloaded loss {again:.8f}")
    assert abs(again - after) <= 1e-6   # the model normalises with the device kernel, the trainer with F.normalize


def _clip_dir(root, name, seed, n=4, h=64, w=64):
    from PIL import Image
    import numpy as np
    d = root / name
    d.mkdir()
    g = np.random.default_rng(seed)
    for i in range(n):
        Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(d / f"frame_{i:04d}.jpg", quality=90)
    return d


def test_train_full_cli_runs_two_steps_on_a_two_clip_directory(device, tmp_path):
    import json
    from scripts import train_full
    anns = [{"video_id": f"v{i}", "frames_dir": str(_clip_dir(tmp_path, f"clip{i}", i)),
             "caption_ids": [[3 + i, 7, 9, 11 + i]]} for i in range(2)]
    ann = tmp_path / "annotations.json"
    ann.write_text(json.dumps(anns), "utf-8")
    rc = train_full.main(["--model", "vit", "--vit_name", "vit_tiny_test", "--max_steps", "2", "--epochs", "1",
                          "--num_frame", "2", "--batch_size", "1", "--ann_train", str(ann), "--ann_val", str(ann),
                          "--vocab_size", "64", "--pad_id", "0", "--txt_dim", "128", "--txt_layers", "1",
                          "--txt_nhead", "2", "--proj_dim", "64", "--precision", "bf16", "--weights_seed", "2",
                          "--device", "cuda:0", "--run_dir", str(tmp_path / "run"), "--ckpt_dir", str(tmp_path / "ckpt")])
    assert rc == 0
    assert len((tmp_path / "run" / "events.csv").read_text().splitlines()) == 2
    ck = torch.load(tmp_path / "ckpt" / "msvd_vitalign_best.pt", map_location="cpu", weights_only=True)
    keys = set(ck["model_state"])
    assert {"vit.cls_token", "vit.blocks.1.mlp.fc2.weight", "vid_proj.weight", "txt_proj.bias"} <= keys
