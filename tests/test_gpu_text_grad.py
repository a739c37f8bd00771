"""The text tower's backward on the GPU (vcap_text_encode_backward through HipTextEmbedder.encode_text_backward,
vcap.train_align.EncodeText and AlignTrainer) against the fp64 autograd oracle of tests/text_grad_cases.py, in
both operand dtypes.

Bounds (derived in text_grad_cases.py, CPU quantities of the case and tensor): f32 <= 10 x the error of torch
float32 autograd, bf16 <= 3 x the error of the fp64 emulation that rounds where the device rounds.  A tensor
whose oracle is identically zero must be exact +0.  A tensor whose bf16 emulation error is exactly 0 meets no
bf16 rounding at all (a tower of 0 layers; txt_proj.bias of an all-pad call): there the bound 3 x 0 is asked
in the only form f32 arithmetic can meet - the bf16 call must give the f32 call's bits, which are held to the
f32 bound.  Every test prints its figures before it asserts.
"""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import text_grad_cases as GC
import text_tower_cases as TC
from vcap import _native as N
from vcap import retrieval as R

pytestmark = pytest.mark.gpu
DTYPES = ["f32", "bf16"]


@lru_cache(maxsize=None)
def _embedder(name: str, dtype: str) -> R.HipTextEmbedder:
    emb = R.HipTextEmbedder.from_state_dict(TC.state_dict(name), TC.PAD_ID[name], TC.TOWERS[name][1], dtype, "cuda:0")
    return emb.enable_grad()


def _host(grads):
    """device grads -> {name: cpu tensor}; the embedding gradient stays (ids, rows)"""
    return {k: (tuple(t.cpu() for t in v) if isinstance(v, tuple) else v.cpu()) for k, v in grads.items()}


def _backward(name, dtype, ids, G):
    out, grads = _embedder(name, dtype).encode_text_backward(ids, G)
    torch.cuda.synchronize()
    return out.cpu(), _host(grads)


@lru_cache(maxsize=None)
def _case_backward(case, dtype):
    return _backward(case.tower, dtype, GC.ids_of(case), GC.grad_out(case))


def _dense(name, grads):
    """every gradient as a dense tensor under its state-dict name"""
    ids, rows = grads["txt_emb.weight"]
    return {**grads, "txt_emb.weight": GC.dense_embedding_grad(ids, rows, TC.TOWERS[name][5])}


def _bits(t: torch.Tensor) -> bytes:
    return t.contiguous().numpy().tobytes()


def _same_bits(a, b) -> bool:
    if a.keys() != b.keys():
        return False
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, tuple):
            if not all(_bits(p) == _bits(q) for p, q in zip(x, y)):
                return False
        elif _bits(x) != _bits(y):
            return False
    return True


def _check_against_oracle(tag, tower, dense, g64s, tol, f32_dense=None):
    worst = 0.0
    failed = []
    for k, g64 in g64s.items():
        g = dense[k]
        assert g.dtype == torch.float32 and g.shape == g64.shape, k
        if GC.is_zero_tensor(g64):
            ok = bool(GC.is_plus_zero(g).all())
            print(f"{tag} {k} oracle zero: exact +0 {ok}")
        elif tol[k] == 0.0:
            assert f32_dense is not None, "an f32 reference error cannot be 0"
            ok = _bits(g) == _bits(f32_dense[k])
            print(f"{tag} {k} no bf16 rounding point: bits of the f32 call {ok}")
        else:
            e = GC.err(g, g64)
            ok = e <= tol[k]
            worst = max(worst, e / tol[k])
            print(f"{tag} {k} err {e:.3e} bound {tol[k]:.3e} ratio {e / tol[k]:.3f}")
        if not ok:
            failed.append(k)
    print(f"{tag} worst err / bound {worst:.3f}")
    assert not failed, failed


# ---- 1. the oracle, every tensor, every case
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", GC.CASES, ids=GC.case_id)
def test_gradients_match_the_fp64_oracle(device, case, dtype):
    _, grads = _case_backward(case, dtype)
    f32 = _dense(case.tower, _case_backward(case, "f32")[1]) if dtype == "bf16" else None
    _check_against_oracle(f"TEXT_GRAD {dtype} {GC.case_id(case)}", case.tower, _dense(case.tower, grads),
                          GC.oracle_grads(case), GC.tolerances(case, dtype), f32)


# ---- 2. the forward's bits, no state
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [GC.find("e128", 3, 11), GC.find("ref", 8, 64), GC.find("ref_0layers", 5, 33),
                                  GC.find("ref", 2, 16)], ids=GC.case_id)
def test_out_has_encode_texts_bits_and_the_backward_leaves_no_state(device, case, dtype):
    emb, ids = _embedder(case.tower, dtype), GC.ids_of(case)
    before = emb.encode_text(ids).cpu()
    out, _ = _backward(case.tower, dtype, ids, GC.grad_out(case))
    after = emb.encode_text(ids).cpu()
    assert _bits(before) == _bits(out) == _bits(after)


# ---- 3. determinism
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [GC.find("e128", 5, 33), GC.find("ref", 8, 64), GC.find("ref", 3, 11)], ids=GC.case_id)
def test_two_calls_and_a_cu_masked_stream_give_the_same_bits(device, case, dtype):
    ids, G = GC.ids_of(case), GC.grad_out(case)
    o1, g1 = _backward(case.tower, dtype, ids, G)
    o2, g2 = _backward(case.tower, dtype, ids, G)
    assert _bits(o1) == _bits(o2) and _same_bits(g1, g2)
    h = C.c_void_p()
    N.check(N.lib().vcap_stream_create_cu_reserved(32, C.byref(h)), "masked stream")
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.ExternalStream(h.value, device=device)):
            o3, g3 = _backward(case.tower, dtype, ids, G)
    finally:
        torch.cuda.synchronize()
        N.check(N.lib().vcap_stream_destroy(h), "stream destroy")
    assert _bits(o1) == _bits(o3) and _same_bits(g1, g3)


# ---- 4. power-of-two scaling is exact
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [GC.find("e128", 3, 11), GC.find("ref", 5, 33)], ids=GC.case_id)
def test_doubling_grad_out_doubles_every_gradient_exactly(device, case, dtype):
    ids, G = GC.ids_of(case), GC.grad_out(case)
    _, g1 = _backward(case.tower, dtype, ids, G)
    _, g2 = _backward(case.tower, dtype, ids, 2 * G)
    d1, d2 = _dense(case.tower, g1), _dense(case.tower, g2)
    for k in d1:
        assert _bits(2 * d1[k]) == _bits(d2[k]), k
    assert torch.equal(g1["txt_emb.weight"][0], g2["txt_emb.weight"][0])


# ---- 5. the row-sparse embedding gradient
def _raw_embedding(name, dtype, ids, G):
    """(emb_ids [M], emb_rows [M, E], count) as the ABI leaves them: one chunk, nothing trimmed"""
    emb = _embedder(name, dtype)
    t = emb._ids(ids)
    n, L = t.shape
    M = n * L
    out = torch.empty(n, emb.proj_dim, dtype=torch.float32, device=emb.device)
    _, (eids, rows, count) = emb._backward_chunk(t, G.to(emb.device).contiguous(), out)
    torch.cuda.synchronize()
    return eids.cpu(), rows.cpu(), count


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [GC.find("e128", 5, 33), GC.find("ref", 8, 64), GC.find("e128", 2, 16),
                                  GC.find("ref", 1, 4)] + GC.CRAFTED, ids=GC.case_id)
def test_embedding_rows_are_sorted_distinct_and_padded_with_minus_one(device, case, dtype):
    name, ids = case.tower, GC.ids_of(case)
    pad = TC.PAD_ID[name]
    all_ids, all_rows, count = _raw_embedding(name, dtype, ids, GC.grad_out(case))
    want = np.unique(ids[ids != pad])
    print(f"TEXT_GRAD_EMB {dtype} {GC.case_id(case)} count {int(count)} host count {want.size} of M {ids.size}")
    assert int(count) == want.size
    assert all_ids.shape == (ids.size,) and all_rows.shape == (ids.size, TC.TOWERS[name][0])
    assert np.array_equal(all_ids[:want.size].numpy(), want)          # ascending, distinct, no pad id
    assert bool((all_ids[want.size:] == -1).all())
    assert bool(GC.is_plus_zero(all_rows[want.size:]).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", GC.CRAFTED, ids=GC.case_id)
def test_one_row_summing_33_positions_is_within_bound(device, case, dtype):
    _, grads = _case_backward(case, dtype)
    ids, rows = grads["txt_emb.weight"]
    assert ids.tolist() == [TC.PAD_ID[case.tower] + 2] and rows.shape[0] == 1
    f32 = _dense(case.tower, _case_backward(case, "f32")[1]) if dtype == "bf16" else None
    _check_against_oracle(f"TEXT_GRAD_REPEAT {dtype} {GC.case_id(case)}", case.tower, _dense(case.tower, grads),
                          GC.oracle_grads(case), GC.tolerances(case, dtype), f32)


# ---- 6. exact zeros
def _encoder_and_proj_w(dense):
    return {k: v for k, v in dense.items() if k != "txt_proj.bias"}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tower", GC.TOWERS)
def test_an_all_pad_call_gives_plus_zero_everywhere_but_proj_bias(device, tower, dtype):
    case = GC.find(tower, 1, 4)
    _, grads = _case_backward(case, dtype)
    ids, rows = grads["txt_emb.weight"]
    assert ids.numel() == 0 and rows.shape[0] == 0
    dense = _dense(tower, grads)
    for k, v in _encoder_and_proj_w(dense).items():
        assert bool(GC.is_plus_zero(v).all()), k
    g64 = GC.oracle_grads(case)["txt_proj.bias"]
    e, tol = GC.err(dense["txt_proj.bias"], g64), GC.tolerances(case, "f32")["txt_proj.bias"]
    print(f"TEXT_GRAD_ZERO {dtype} {tower} proj_b err {e:.3e} f32 bound {tol:.3e}")
    assert e <= tol          # no bf16 rounding point: both dtypes meet the f32 bound


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tower", GC.TOWERS)
def test_zero_grad_out_for_the_only_live_caption_gives_the_same_zeros(device, tower, dtype):
    case = GC.find(tower, 2, 16)                      # caption 0 has no pad, caption 1 only pads
    G = GC.grad_out(case).clone()
    G[0] = 0.0
    _, grads = _backward(tower, dtype, GC.ids_of(case), G)
    ids, rows = grads["txt_emb.weight"]
    assert ids.numel() == 16 or ids.numel() == np.unique(GC.ids_of(case)[0]).size
    assert bool(GC.is_plus_zero(rows).all())
    dense = _dense(tower, grads)
    for k, v in _encoder_and_proj_w(dense).items():
        assert bool(GC.is_plus_zero(v).all()), k
    g64 = GC.grads_from(tower, GC.ids_of(case), G, "fp64")["txt_proj.bias"]
    tol = GC.F32_FACTOR * GC.err(GC.grads_from(tower, GC.ids_of(case), G, "f32")["txt_proj.bias"], g64)
    e = GC.err(dense["txt_proj.bias"], g64)
    print(f"TEXT_GRAD_ZERO_G {dtype} {tower} proj_b err {e:.3e} f32 bound {tol:.3e}")
    assert e <= tol


# ---- 7. chunking in Python
@pytest.mark.parametrize("dtype", DTYPES)
def test_twenty_captions_of_33_go_in_two_calls_summed_in_order(device, dtype):
    name = "ref"
    big = TC.Case(name, 20, 33, tuple(["none", "trailing", "interior", "allpad", "trailing"] * 4))
    ids, emb = TC.ids_of(big), _embedder(name, dtype)
    G = torch.randn(20, TC.TOWERS[name][4], generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    per = emb.max_rows // 33
    assert per == 15                                              # 15 + 5 captions
    out, grads = _backward(name, dtype, ids, G)
    oa, ga = _backward(name, dtype, ids[:per], G[:per])
    ob, gb = _backward(name, dtype, ids[per:], G[per:])
    assert _bits(out) == _bits(torch.cat([oa, ob]))
    da, db, dd = _dense(name, ga), _dense(name, gb), _dense(name, grads)
    for k in dd:
        assert _bits(dd[k]) == _bits(da[k] + db[k]), k
    assert np.array_equal(grads["txt_emb.weight"][0].numpy(), np.unique(ids[ids != TC.PAD_ID[name]]))
    g64s = GC.grads_from(name, ids, G, "fp64")
    _check_against_oracle(f"TEXT_GRAD_CHUNK {dtype}", name, dd, g64s, GC.tolerances_from(name, ids, G, dtype, g64s))


# ---- 8. refusals
def _raw_call(emb, desc, gdesc, n, L, ws_bytes=None, null_grad=False):
    dev, E, F, P = emb.device, emb.dim, emb.ffn, emb.proj_dim
    M = n * L
    lib = N.lib()
    sentinel = 123.0
    bufs = []

    def buf(*shape, dtype=torch.float32):
        t = torch.full(shape, sentinel if dtype == torch.float32 else 77, dtype=dtype, device=dev)
        bufs.append(t)
        return t

    glayers = (N.TextParamGradsLayer * max(emb.n_layer, 1))()
    shapes = {"in_w": (3 * E, E), "in_b": (3 * E,), "out_w": (E, E), "out_b": (E,), "ln1_g": (E,), "ln1_b": (E,),
              "fc1_w": (F, E), "fc1_b": (F,), "fc2_w": (E, F), "fc2_b": (E,), "ln2_g": (E,), "ln2_b": (E,)}
    for i in range(emb.n_layer):
        for f, shp in shapes.items():
            setattr(glayers[i], f, buf(*shp).data_ptr())
    grads = N.TextParamGrads(proj_w=None if null_grad else buf(P, E).data_ptr(), proj_b=buf(P).data_ptr(),
                             emb_ids=buf(M, dtype=torch.int32).data_ptr(), emb_rows=buf(M, E).data_ptr(),
                             emb_count=buf(1, dtype=torch.int32).data_ptr(), layers=glayers)
    ids = torch.ones(n, L, dtype=torch.int32, device=dev)
    G = torch.ones(n, P, dtype=torch.float32, device=dev)
    out = buf(n, P)
    need = int(lib.vcap_text_encode_backward_workspace_bytes(C.byref(desc), C.byref(gdesc), n, L))
    ws = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=dev)
    rc = lib.vcap_text_encode_backward(C.byref(desc), C.byref(gdesc), ids.data_ptr(), n, L, G.data_ptr(), C.byref(grads),
                                       out.data_ptr(), ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                                       R._stream(dev))
    torch.cuda.synchronize()
    untouched = all(bool((t == (sentinel if t.dtype == torch.float32 else 77)).all()) for t in bufs)
    return rc, need, untouched


def test_refusals_return_the_documented_codes_and_write_nothing(device):
    emb = _embedder("e128", "f32")
    gd = emb.grad_desc
    rc, need, untouched = _raw_call(emb, emb.desc, gd, 2, 8)
    assert rc == 0 and need > 0 and not untouched                                   # the call itself works
    for field, value in (("dtype", N.DT_BF16), ("dim", 256), ("ffn", 1024), ("n_layer", 1)):
        bad = N.TextGradDesc(dtype=gd.dtype, dim=gd.dim, ffn=gd.ffn, n_layer=gd.n_layer, layers=gd.layers)
        setattr(bad, field, value)
        rc, need, untouched = _raw_call(emb, emb.desc, bad, 2, 8)
        assert (rc, need, untouched) == (N.E_ARG, 0, True), field
    assert _raw_call(emb, emb.desc, gd, 1, 65) == (N.E_UNSUPPORTED, 0, True)
    assert _raw_call(emb, emb.desc, gd, 27, 19) == (N.E_UNSUPPORTED, 0, True)      # B * L = 513
    rc, need, untouched = _raw_call(emb, emb.desc, gd, 2, 8, ws_bytes=1024)
    assert (rc, untouched) == (N.E_WORKSPACE, True) and need > 1024
    rc, need, untouched = _raw_call(emb, emb.desc, gd, 2, 8, null_grad=True)
    assert (rc, untouched) == (N.E_ARG, True)
    with pytest.raises(ValueError, match="at most 64"):
        emb.encode_text_backward(np.ones((1, 65), np.int64), torch.zeros(1, 64))
    with pytest.raises(ValueError, match="grad_out"):
        emb.encode_text_backward(np.ones((2, 8), np.int64), torch.zeros(1, 64))


# ---- 9. an id outside the vocabulary, delivered on the device
@pytest.mark.parametrize("name", ["ref", "ref_0layers", "e128"])
@pytest.mark.parametrize("bad", ["vocab", "negative", "huge"])
def test_an_out_of_range_id_on_the_device_gives_nan_gradients_and_no_fault(device, name, bad):
    c = GC.find(name, 3, 11)
    ids = GC.ids_of(c).copy()
    V = TC.TOWERS[name][5]
    ids[1, 4] = {"vocab": V, "negative": -1, "huge": 2 ** 31 - 1}[bad]
    t = torch.from_numpy(ids).to(device).to(torch.int32)          # a device tensor is not range-checked on the host
    out, grads = _embedder(name, "f32").encode_text_backward(t, GC.grad_out(c))
    torch.cuda.synchronize()
    grads = _host(grads)
    assert bool(torch.isnan(out[1]).all()) and bool(torch.isfinite(out[[0, 2]]).all())
    eids, rows = grads["txt_emb.weight"]
    assert bool(((eids >= 0) & (eids < V)).all())                 # the bad id is never listed
    for k, v in grads.items():
        if k != "txt_emb.weight":
            assert bool(torch.isnan(v).all()), k
    # the tower still answers afterwards
    again, _ = _backward(name, "f32", GC.ids_of(c), GC.grad_out(c))
    assert bool(torch.isfinite(again).all())


# ---- 10. load_state_dict in place
@pytest.mark.parametrize("dtype", DTYPES)
def test_load_state_dict_rewrites_every_device_weight_in_place(device, dtype):
    name = "e128"
    sd = TC.state_dict(name)
    emb = R.HipTextEmbedder.from_state_dict(sd, TC.PAD_ID[name], 2, dtype, "cuda:0").enable_grad()
    rs = np.random.RandomState(3)
    sd2 = {k: (v + 0.05 * rs.randn(*v.shape)).astype(np.float32) for k, v in sd.items()}
    ptrs = bytes(emb.desc), bytes(emb.layers), bytes(emb.grad_desc), bytes(emb._glayers)
    case = GC.find(name, 3, 11)
    ids, G = GC.ids_of(case), GC.grad_out(case)
    emb.load_state_dict({k: torch.from_numpy(v) for k, v in sd2.items()})
    fresh = R.HipTextEmbedder.from_state_dict(sd2, TC.PAD_ID[name], 2, dtype, "cuda:0").enable_grad()
    assert ptrs == (bytes(emb.desc), bytes(emb.layers), bytes(emb.grad_desc), bytes(emb._glayers))
    assert _bits(emb.encode_text(ids).cpu()) == _bits(fresh.encode_text(ids).cpu())
    o1, g1 = emb.encode_text_backward(ids, G)
    o2, g2 = fresh.encode_text_backward(ids, G)
    torch.cuda.synchronize()
    assert _bits(o1.cpu()) == _bits(o2.cpu()) and _same_bits(_host(g1), _host(g2))
    emb.load_state_dict(sd)                                        # numpy values, back to the first weights
    assert _bits(emb.encode_text(ids).cpu()) == _bits(_embedder(name, dtype).encode_text(ids).cpu())


# ---- 11. the autograd Function under the training loss
def _align_batch(name, B, L, vid_dim=96):
    g = torch.Generator().manual_seed(77)
    E, H, Fd, nl, P, V = TC.TOWERS[name]
    ids = TC.ids_of(TC.Case(name, B, L, tuple(["none", "trailing", "interior"] * (B // 3))))
    feat = torch.randn(B, vid_dim, generator=g)
    vid_w = torch.randn(P, vid_dim, generator=g) / np.sqrt(vid_dim)
    vid_b = 0.1 * torch.randn(P, generator=g)
    return ids, feat, vid_w, vid_b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["e128", "ref"])
def test_encode_text_function_reaches_every_parameter_under_the_cosine_loss(device, name, dtype):
    from vcap.train_align import AlignTrainer
    ids, feat, vid_w, vid_b = _align_batch(name, 6, 12)
    sd = {**TC.state_dict(name), "vid_proj.weight": vid_w.numpy(), "vid_proj.bias": vid_b.numpy()}
    emb = R.HipTextEmbedder.from_state_dict(sd, TC.PAD_ID[name], TC.TOWERS[name][1], dtype, "cuda:0")
    tr = AlignTrainer(emb, sd)
    loss = tr.loss(feat.to(device), ids)
    loss.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.cpu() for k, p in zip(tr.names, tr.params)}
    got.update({"vid_proj.weight": tr.vid_proj.weight.grad.cpu(), "vid_proj.bias": tr.vid_proj.bias.grad.cpu()})
    assert all(g is not None for g in got.values())
    l64, g64s = GC.align_loss_grads(name, ids, feat, vid_w, vid_b, "fp64")
    _, ref = GC.align_loss_grads(name, ids, feat, vid_w, vid_b, "f32" if dtype == "f32" else "bf16")
    factor = GC.F32_FACTOR if dtype == "f32" else GC.BF16_FACTOR
    tol = {k: factor * e for k, e in GC.errors(ref, g64s).items()}
    print(f"TEXT_GRAD_LOSS {dtype} {name} loss {float(loss):.8f} fp64 {l64:.8f}")
    assert got.keys() == g64s.keys()
    _check_against_oracle(f"TEXT_GRAD_LOSS {dtype} {name}", name, got, g64s, tol)


# ---- 12. the trainer
@pytest.mark.parametrize("dtype", DTYPES)
def test_twenty_steps_lower_the_loss_and_the_state_dict_round_trips(device, dtype):
    from vcap.train_align import AlignTrainer
    name = "e128"
    ids, feat, vid_w, vid_b = _align_batch(name, 6, 12)
    feat = feat.to(device)
    sd = {**TC.state_dict(name), "vid_proj.weight": vid_w.numpy(), "vid_proj.bias": vid_b.numpy()}
    emb = R.HipTextEmbedder.from_state_dict(sd, TC.PAD_ID[name], 2, dtype, "cuda:0")
    tr = AlignTrainer(emb, sd, lr=5e-4)
    before = tr.evaluate(feat, ids)
    losses = [tr.step(feat, ids) for _ in range(20)]
    after = tr.evaluate(feat, ids)
    print(f"TEXT_TRAIN {dtype} loss before {before:.6f} after 20 steps {after:.6f} (first step {losses[0]:.6f})")
    assert losses[0] == before and after < before and tr.steps == 20
    state = tr.state_dict()
    assert set(state) == set(sd) and all(v.device.type == "cpu" for v in state.values())
    fresh = R.HipTextEmbedder.from_state_dict(state, TC.PAD_ID[name], 2, dtype, "cuda:0")
    v = tr.encode_video(feat).detach()
    t = fresh.encode_text(ids)
    again = float(torch.nn.functional.cosine_embedding_loss(v, t, torch.ones(6, device=device)))
    assert again == after
