"""vcap_gpt2_score_backward_tail on the GPU: the gradient of the teacher-forced objective with respect to
every parameter of the last n_tail GPT-2 blocks (csrc/gpt2_weight_grad.hip, csrc/runtime_gpt2_grad.hip),
HipGPT2Decoder.score_backward_tail / load_tail and the training surface of vcap/train.py, against the fp64
autograd oracle of tests/tail_grad_cases.py.

Tolerances are per parameter tensor and come from CPU runs alone (tail_grad_cases.tolerance):
  fp32  err <= 10 * err(torch CPU float32 autograd of the same case and tensor)
  bf16  err <= 3 * err(the bf16-emulated CPU run of the same case and tensor)
with err(g) = max |g - g64| / max |g64| over the tensor.  The accuracy test prints every tensor's measured
error, bound and ratio before it asserts.  Cases and shapes: tail_grad_cases' docstring."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

import score_cases as SC
import score_grad_cases as G
import tail_grad_cases as TG
from vcap import _native as N
from vcap.model import GenConfig, HipGPT2Decoder

pytestmark = pytest.mark.gpu
PRECS = ["fp32", "bf16"]
V = TG.V
SENTINEL = 777.0


@lru_cache(maxsize=None)
def decoder(E, prec):
    d = HipGPT2Decoder(SC.state_dict(E, V), SC.arch(E, V), prec, "cuda", screen=False)
    d.enable_grad(SC.state_dict(E, V))
    return d


def last_error() -> str:
    return (N.lib().vcap_last_error() or b"").decode()


def _dev_inputs(dec, x, km, tg, w):
    dev = dec.device
    return (x.to(dev, torch.float32).contiguous(), None if km is None else km.to(dev, torch.uint8).contiguous(),
            tg.to(dev, torch.int32).contiguous(), None if w is None else w.to(dev, torch.float32).contiguous())


def abi_backward(dec, x, km, tg, w):
    """One raw vcap_gpt2_score_backward call -> (grad, logprobs, loss[2])."""
    x, km, tg, w = _dev_inputs(dec, x, km, tg, w)
    B, S, _ = x.shape
    grad, lp, loss = torch.empty_like(x), torch.empty(B, S, device=x.device), torch.empty(2, device=x.device)
    ws = torch.empty(int(N.lib().vcap_gpt2_score_backward_workspace_bytes(C.byref(dec.desc), C.byref(dec.grad_desc),
                                                                          B, S)), dtype=torch.uint8, device=x.device)
    rc = N.lib().vcap_gpt2_score_backward(C.byref(dec.desc), C.byref(dec.grad_desc), x.data_ptr(), B, S, N.ptr(km),
                                          tg.data_ptr(), N.ptr(w), grad.data_ptr(), lp.data_ptr(), loss.data_ptr(),
                                          ws.data_ptr(), ws.numel(), torch.cuda.current_stream(x.device).cuda_stream)
    torch.cuda.synchronize(x.device)
    assert rc == 0, last_error()
    return grad, lp, loss


def abi_tail(dec, x, km, tg, w, n_tail, ws_bytes=None, n_field=None, null=None, pass_struct=True):
    """One raw vcap_gpt2_score_backward_tail call -> (rc, grad, logprobs, loss[2], {name: gradient}); every
    output pre-filled with a sentinel so that a refused call is seen to have written nothing.  n_field: the
    struct's n_tail when it differs from the allocated layers; null: (entry, field) passed as NULL."""
    x, km, tg, w = _dev_inputs(dec, x, km, tg, w)
    dev = x.device
    B, S, _ = x.shape
    names = dec.tail_names(n_tail)
    grad = torch.full_like(x, SENTINEL)
    lp, loss = torch.full((B, S), SENTINEL, device=dev), torch.full((2,), SENTINEL, device=dev)
    pgs = [torch.full(dec._tail_shape(k), SENTINEL, device=dev) for k in names]
    layers = (N.GPT2ParamGradsLayer * n_tail)()
    for i in range(n_tail):
        for j, (field, _) in enumerate(N.GPT2ParamGradsLayer._fields_):
            setattr(layers[i], field, None if null == (i, field) else pgs[i * 12 + j].data_ptr())
    pg = N.GPT2ParamGrads(n_tail=n_tail if n_field is None else n_field, layers=layers)
    need = int(N.lib().vcap_gpt2_score_backward_tail_workspace_bytes(C.byref(dec.desc), C.byref(dec.grad_desc), B, S,
                                                                     n_tail))
    ws = torch.empty(max(need if ws_bytes is None else ws_bytes, 1), dtype=torch.uint8, device=dev)
    rc = N.lib().vcap_gpt2_score_backward_tail(C.byref(dec.desc), C.byref(dec.grad_desc), x.data_ptr(), B, S, N.ptr(km),
                                               tg.data_ptr(), N.ptr(w), grad.data_ptr(),
                                               C.byref(pg) if pass_struct else None, lp.data_ptr(), loss.data_ptr(),
                                               ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                                               torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return rc, grad, lp, loss, dict(zip(names, pgs))


def run_tail(c, prec, n_tail, wmode="rand", w=None):
    x, km, tg, w0 = TG.inputs(c, wmode)
    rc, grad, lp, loss, pg = abi_tail(decoder(c.E, prec), x, km, tg, w0 if w is None else w, n_tail)
    assert rc == 0, last_error()
    return grad, lp, loss, pg


def same_bits(a, b) -> bool:
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a) and set(a) == set(b)


# ------------------------------------------------------------------------------- 0. the product alone
# Operands are integers in [-8, 8]: every product and every partial sum of <= 512 of them is an integer below
# 2^24, exact in bf16 operands and f32 accumulation in ANY summation order - so the bound is equality with
# the fp64 product.  Both buffers carry 40 rows of NaN past M: rows the reduction must never read.
DW_SHAPES = [(128, 128), (128, 384), (512, 128), (256, 1024)]                       # (K, N): 2 to 8 x 1 to 8 tiles
DW_ROWS = [1, 31, 32, 33, 63, 64, 65, 129, 512]
DW_DTYPES = {"fp32": (N.DT_F32, torch.float32), "bf16": (N.DT_BF16, torch.bfloat16)}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("K,Nc", DW_SHAPES)
def test_product_kernel_is_exact_on_integers_and_never_reads_past_m(K, Nc, prec):
    dt, tdt = DW_DTYPES[prec]
    g = torch.Generator().manual_seed(K + 7 * Nc)
    for M in DW_ROWS:
        X = torch.randint(-8, 9, (M + 40, K), generator=g).double()
        Y = torch.randint(-8, 9, (M + 40, Nc), generator=g).double()
        Y[M // 2] = 0.0                                       # a literal zero row contributes nothing
        want = X[:M].t() @ Y[:M]
        X[M:], Y[M:] = float("nan"), float("nan")
        Xd, Yd = X.to("cuda", tdt).contiguous(), Y.to("cuda", tdt).contiguous()
        out = torch.full((K, Nc), SENTINEL, device="cuda")
        rc = N.lib().vcap_gpt2_weight_grad(dt, Xd.data_ptr(), Yd.data_ptr(), out.data_ptr(), M, K, Nc,
                                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0, last_error()
        assert torch.equal(out.cpu().double(), want), (M, K, Nc, float((out.cpu().double() - want).abs().max()))


def test_product_kernel_refusals_write_nothing():
    X, Y = torch.zeros(64, 128, device="cuda"), torch.zeros(64, 128, device="cuda")
    out = torch.full((128, 128), SENTINEL, device="cuda")
    call = N.lib().vcap_gpt2_weight_grad
    s = torch.cuda.current_stream().cuda_stream
    assert call(N.DT_F16, X.data_ptr(), Y.data_ptr(), out.data_ptr(), 64, 128, 128, s) == N.E_ARG
    assert call(N.DT_F32, None, Y.data_ptr(), out.data_ptr(), 64, 128, 128, s) == N.E_ARG
    assert call(N.DT_F32, X.data_ptr(), Y.data_ptr(), out.data_ptr(), 0, 128, 128, s) == N.E_ARG
    assert call(N.DT_F32, X.data_ptr(), Y.data_ptr(), out.data_ptr(), 513, 128, 128, s) == N.E_UNSUPPORTED
    assert call(N.DT_F32, X.data_ptr(), Y.data_ptr(), out.data_ptr(), 64, 96, 128, s) == N.E_UNSUPPORTED
    assert call(N.DT_F32, X.data_ptr(), Y.data_ptr(), out.data_ptr(), 64, 128, 64, s) == N.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("n_tail", TG.N_TAILS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", TG.CASES, ids=lambda c: c.name)
def test_weight_gradients_match_fp64_autograd(c, prec, n_tail):
    _, _, _, pg = run_tail(c, prec, n_tail)
    g64, tol = TG.oracle(c), TG.tolerance(c, "rand", prec)
    names = TG.tail_names(2, n_tail)
    assert list(pg) == names and len(names) == 12 * n_tail
    factor = TG.F32_FACTOR if prec == "fp32" else TG.BF16_FACTOR
    bad = []
    for k in names:
        ok, e = TG.check(k, pg[k].cpu(), g64[k], tol[k])
        ref = tol[k] / factor
        print(f"tail_grad {c.name} {prec} n_tail={n_tail} {k[len(TG.P):]}: err {e:.3e} tol {tol[k]:.3e} "
              f"cpu_ref_err {ref:.3e} ratio {e / ref if ref else 0.0:.3f}")
        assert tuple(pg[k].shape) == tuple(g64[k].shape), k
        if not ok:
            bad.append((k, e, tol[k]))
    assert not bad, bad


# -------------------------------------------------------------------------------------- 2. the contracts
EXACT = [TG.MASKS[1], TG.MASKS[2], TG.ROWS[7]]   # right, interior, 129 rows


@pytest.mark.parametrize("n_tail", TG.N_TAILS)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", EXACT, ids=lambda c: c.name)
def test_embedding_gradient_and_forward_outputs_are_score_backwards_bits(c, prec, n_tail):
    grad, lp, loss, _ = run_tail(c, prec, n_tail)
    g0, lp0, loss0 = abi_backward(decoder(c.E, prec), *TG.inputs(c))
    assert torch.equal(grad.view(torch.int32), g0.view(torch.int32))
    assert torch.equal(lp.view(torch.int32), lp0.view(torch.int32))
    assert torch.equal(loss.view(torch.int32), loss0.view(torch.int32))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", [TG.MASKS[2], TG.ROWS[7]], ids=lambda c: c.name)
def test_two_calls_and_a_cu_masked_stream_give_the_same_bits(device, c, prec):
    g1, _, _, p1 = run_tail(c, prec, 2)
    g2, _, _, p2 = run_tail(c, prec, 2)
    assert torch.equal(g1, g2) and same_bits(p1, p2)
    h = C.c_void_p()
    N.check(N.lib().vcap_stream_create_cu_reserved(32, C.byref(h)), "masked stream")
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.ExternalStream(h.value, device=device)):
            g3, _, _, p3 = run_tail(c, prec, 2)
    finally:
        torch.cuda.synchronize()
        N.check(N.lib().vcap_stream_destroy(h), "stream destroy")
    assert torch.equal(g1, g3) and same_bits(p1, p3)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c", EXACT, ids=lambda c: c.name)
def test_doubling_grad_logprob_doubles_every_bit(c, prec):
    w = G.weights_w(c, "rand")
    _, _, _, p1 = run_tail(c, prec, 2)
    _, _, _, p2 = run_tail(c, prec, 2, w=2.0 * w)
    assert same_bits({k: 2.0 * v for k, v in p1.items()}, p2)
    assert all(bool((v != 0).any()) for v in p1.values())


@pytest.mark.parametrize("n_tail", TG.N_TAILS)
@pytest.mark.parametrize("prec", PRECS)
def test_all_targets_ignored_gives_plus_zero_everywhere(prec, n_tail):
    grad, lp, loss, pg = run_tail(TG.IGNORED, prec, n_tail, "null")
    assert bool(G.is_plus_zero(grad).all()) and loss.tolist() == [0.0, 0.0]
    for k, v in pg.items():
        assert bool(G.is_plus_zero(v).all()), k


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c,extra", [(TG.MASKS[1], 2), (TG.ROWS[1], 3), (TG.ROWS[3], 1)],
                         ids=["39_to_65_rows", "31_to_124_rows", "33_to_44_rows"])
def test_appending_uncounted_sequences_changes_no_bit(c, extra, prec):
    dec = decoder(c.E, prec)
    x, km, tg, w = TG.inputs(c)
    _, _, _, _, p1 = abi_tail(dec, x, km, tg, w, 2)
    g = torch.Generator().manual_seed(99)
    x2 = torch.cat([x, 0.3 * torch.randn(extra, c.S, c.E, generator=g)], dim=0)
    km2 = None if km is None else torch.cat([km, torch.ones(extra, c.S, dtype=km.dtype)], dim=0)
    tg2 = torch.cat([tg, torch.full((extra, c.S), SC.IGNORE, dtype=tg.dtype)], dim=0)
    w2 = torch.cat([w, torch.randn(extra, c.S, generator=g)], dim=0)
    rc, _, _, _, p2 = abi_tail(dec, x2, km2, tg2, w2, 2)
    assert rc == 0, last_error()
    assert same_bits(p1, p2)


@pytest.mark.parametrize("prec", PRECS)
def test_python_chunking_adds_the_chunks_in_order(prec):
    c = SC.Case("chunk_9x64", 128, V, 9, 64, "interior")   # 576 rows: two chunks (8 + 1 sequences)
    dec = decoder(c.E, prec)
    x, km, tg, w = TG.inputs(c)
    res, grad, pg = dec.score_backward_tail(x, km, tg, w, 2)
    res0, grad0 = dec.score_backward(x, km, tg, w)
    assert torch.equal(grad, grad0) and torch.equal(res.logprobs, res0.logprobs)
    assert torch.equal(res.nll_sum, res0.nll_sum) and torch.equal(res.count, res0.count)
    _, ga, _, _, pa = abi_tail(dec, x[:8], km[:8], tg[:8], w[:8], 2)
    _, gb, _, _, pb = abi_tail(dec, x[8:], km[8:], tg[8:], w[8:], 2)
    assert torch.equal(grad[:8], ga) and torch.equal(grad[8:], gb)
    assert list(pg) == dec.tail_names(2)
    assert same_bits(pg, {k: pa[k] + pb[k] for k in pa})
    # one chunk: the single call's bits
    c1 = TG.MASKS[2]
    x, km, tg, w = TG.inputs(c1)
    _, _, pg1 = dec.score_backward_tail(x, km, tg, w, 1)
    _, _, _, _, p1 = abi_tail(dec, x, km, tg, w, 1)
    assert same_bits(pg1, p1)


# ------------------------------------------------------------------------------------------ 3. refusals
def _untouched(grad, lp, loss, pg) -> bool:
    return all(bool((t == SENTINEL).all()) for t in (grad, lp, loss, *pg.values()))


def test_refused_calls_return_the_codes_and_write_nothing():
    dec = decoder(128, "fp32")
    c = TG.MASKS[0]
    x, km, tg, w = TG.inputs(c)
    for n_field in (0, 3, -1):
        rc, *outs = abi_tail(dec, x, km, tg, w, 2, n_field=n_field)
        assert rc == N.E_ARG and "n_tail outside 1 .. n_layer" in last_error()
        assert _untouched(*outs)
    rc, *outs = abi_tail(dec, x, km, tg, w, 2, pass_struct=False)
    assert rc == N.E_ARG and "param_grads is null" in last_error() and _untouched(*outs)
    for null in ((0, "attn_w"), (1, "ln2_b")):
        rc, *outs = abi_tail(dec, x, km, tg, w, 2, null=null)
        assert rc == N.E_ARG and "a gradient pointer is null" in last_error() and _untouched(*outs)
    need = int(N.lib().vcap_gpt2_score_backward_tail_workspace_bytes(C.byref(dec.desc), C.byref(dec.grad_desc), c.B,
                                                                     c.S, 2))
    base = int(N.lib().vcap_gpt2_score_backward_workspace_bytes(C.byref(dec.desc), C.byref(dec.grad_desc), c.B, c.S))
    assert need > base
    for short in (need - 1, base):     # the activation-only call's workspace is not enough
        rc, *outs = abi_tail(dec, x, km, tg, w, 2, ws_bytes=short)
        assert rc == N.E_WORKSPACE and "workspace too small" in last_error() and _untouched(*outs)
    tg513 = torch.zeros(1, 513, dtype=torch.long)
    rc, *outs = abi_tail(dec, torch.zeros(1, 513, 128), None, tg513, None, 2, ws_bytes=need)
    assert rc == N.E_UNSUPPORTED and "vcap_gpt2_max_rows" in last_error() and _untouched(*outs)
    with pytest.raises(N.VcapError):
        dec.score_backward_tail(x, km, tg, w, 3)
    with pytest.raises(N.VcapError):
        dec.score_backward_tail(x, km, tg, w, 0)


# ------------------------------------------------------------------------------------------ 4. load_tail
def _pointers(dec):
    out = [getattr(dec.desc, f) for f in ("wte", "lm_head", "wpe", "lnf_g", "lnf_b", "lm_head_screen")]
    out.append(C.addressof(dec.layers))
    for ly in dec.layers:
        out += [getattr(ly, f) for f, _ in N.GPT2Layer._fields_]
    out += [dec.grad_desc.wte_t, C.addressof(dec._grad_layers)]
    for ly in dec._grad_layers:
        out += [getattr(ly, f) for f, _ in N.GPT2GradLayer._fields_]
    return out


def _updated_state(sd, names, seed=11):
    """sd with every named tensor moved by a seeded 5 % (of its max magnitude) perturbation."""
    rng = np.random.default_rng(seed)
    out = dict(sd)
    for k in names:
        a = sd[k].astype(np.float32)
        out[k] = (a + 0.05 * float(np.abs(a).max() + 0.1) * rng.standard_normal(a.shape)).astype(np.float32)
    return out


@pytest.mark.parametrize("prec", PRECS)
def test_load_tail_equals_a_fresh_decoder_and_keeps_every_pointer(prec):
    c = TG.MASKS[2]
    sd, ar = SC.state_dict(c.E, V), SC.arch(c.E, V)
    dec = HipGPT2Decoder(sd, ar, prec, "cuda", screen=False)
    dec.enable_grad(sd)
    x, km, tg, w = TG.inputs(c)
    cfg = GenConfig(12, 0, 3, 1.1, ar.eos_token_id, ar.eos_token_id, True)
    prefix = x[:, :4].cuda().contiguous()
    # the scoring call first: it grows the decoder's workspace to its final size, and a decode graph is keyed
    # by the workspace it was captured with
    logits_before = dec.score(x, km, tg, want_logits=True).logits.clone()
    ids_before = dec.generate_ids(prefix, [ar.bos_token_id], cfg).clone()   # captures the decode graph
    ptrs, cached = _pointers(dec), int(N.lib().vcap_graph_cache_size())

    names = dec.tail_names(2)
    sd2 = _updated_state(sd, names)
    dec.load_tail({k: torch.from_numpy(sd2[k]) for k in names})
    assert _pointers(dec) == ptrs
    fresh = HipGPT2Decoder(sd2, ar, prec, "cuda", screen=False)
    fresh.enable_grad(sd2)

    got, want = dec.score(x, km, tg, want_logits=True), fresh.score(x, km, tg, want_logits=True)
    assert not torch.equal(got.logits, logits_before)
    assert torch.equal(got.logits.view(torch.int32), want.logits.view(torch.int32))
    assert torch.equal(got.logprobs, want.logprobs)
    ids_after = dec.generate_ids(prefix, [ar.bos_token_id], cfg).clone()    # replayed from the cache
    assert int(N.lib().vcap_graph_cache_size()) == cached
    ids_fresh = fresh.generate_ids(prefix, [ar.bos_token_id], cfg)
    assert torch.equal(ids_after, ids_fresh)
    assert ids_before.shape == ids_after.shape
    # the grad desc's copies were rewritten too: the backward of both decoders agrees bit for bit
    _, g1, p1 = dec.score_backward_tail(x, km, tg, w, 2)
    _, g2, p2 = fresh.score_backward_tail(x, km, tg, w, 2)
    assert torch.equal(g1, g2) and same_bits(p1, p2)
    # a partial state (one layer's tensors) is accepted; other keys are ignored
    dec.load_tail({names[0]: torch.from_numpy(sd[names[0]]), "decoder.mapper.0.bias": torch.zeros(3)})
    assert _pointers(dec) == ptrs


# ------------------------------------------------------------------------------------ 5. autograd wiring
WIRE = SC.Case("wiring", 128, V, 3, 12)   # 3 clips, prefix 4 + captions of 9 ids (8 inputs)
VIDEO_DIM = 256


def wiring_batch():
    """test_gpu_score_grad.py's wiring batch: (video_emb [3, 256] f32, caption_ids [3, 9], pad_id) with
    bos = eos = pad = V - 1, the last caption right-padded by two."""
    g = torch.Generator().manual_seed(2024)
    emb = torch.randn(WIRE.B, VIDEO_DIM, generator=g, dtype=torch.float32)
    pad = WIRE.V - 1
    ids = torch.randint(0, WIRE.V - 1, (WIRE.B, 9), generator=g)
    ids[:, 0] = pad
    ids[:, -1] = pad
    ids[2, -3:] = pad
    return emb, ids, pad


def linear_from(sd, dtype):
    w = torch.from_numpy(sd["decoder.mapper.0.weight"].copy())
    lin = torch.nn.Linear(w.shape[1], w.shape[0]).to(dtype)
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(torch.from_numpy(sd["decoder.mapper.0.bias"].copy()))
    return lin


def replica_inputs(lin64, emb, ids, pad, prec="fp32"):
    """The fp64 replica's (inputs_embeds with the Linear's graph, key mask, shifted targets).  The token rows
    are the ones the decoder feeds itself: its own table's, bf16-rounded for a bf16 decoder."""
    wte = SC.sd64(WIRE.E, WIRE.V, rounded=prec == "bf16")[SC.DS.WTE]
    inp, labels = ids[:, :-1], ids[:, 1:]
    prefix = lin64(emb.double()).reshape(WIRE.B, SC.PREFIX_LEN, WIRE.E)
    x = torch.cat([prefix, wte[inp]], dim=1)
    km = torch.cat([torch.ones(WIRE.B, SC.PREFIX_LEN, dtype=torch.uint8), (inp != pad).to(torch.uint8)], dim=1)
    return x, km, SC.shift_labels(labels)


def replica_loss(lin64, emb, ids, pad, sd=None):
    x, km, tg = replica_inputs(lin64, emb, ids, pad)
    logits = SC.masked_forward(SC.sd64(WIRE.E, WIRE.V) if sd is None else sd, SC.arch(WIRE.E, WIRE.V), x, km)
    return G._objective(logits, tg, None) / int((tg >= 0).sum())


def new_text_decoder(prec):
    from vcap.caption import HipTextDecoder
    sd = SC.state_dict(WIRE.E, WIRE.V)
    dec = HipTextDecoder(sd, SC.arch(WIRE.E, WIRE.V), prec, "cuda")
    dec.hip.enable_grad(sd)
    return dec


@lru_cache(maxsize=None)
def text_decoder(prec):
    """Shared by the tests that leave the decoder's weights as they are."""
    return new_text_decoder(prec)


@pytest.mark.parametrize("prec", PRECS)
def test_loss_backward_fills_the_mapper_and_every_tail_gradient(prec):
    from vcap import train as T
    dec = text_decoder(prec)
    sd = SC.state_dict(WIRE.E, WIRE.V)
    emb, ids, pad = wiring_batch()
    lin = linear_from(sd, torch.float32).cuda()
    tail = T.tail_parameters(dec.hip, sd, 2)
    assert list(tail) == dec.hip.tail_names(2) and len(tail) == 24
    loss = T.compute_loss(dec, emb, ids, pad, lin, tail)
    assert loss.requires_grad
    loss.backward()
    # the fp64 replica on the same inputs, and the per-tensor bounds of these very inputs from the CPU runs
    lin64 = linear_from(sd, torch.float64)
    x, km, tg = replica_inputs(lin64, emb, ids, pad, prec)
    w = torch.full(tg.shape, -1.0 / int((tg >= 0).sum()))
    xd = x.detach()
    kind, factor = ("f32", TG.F32_FACTOR) if prec == "fp32" else ("bf16", TG.BF16_FACTOR)
    g64 = TG.param_grads_of(WIRE, "", "fp64", xd, km, tg, w)
    ref = TG.param_grads_of(WIRE, "", kind, xd, km, tg, w)
    bad = []
    for k, p in tail.items():
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape), k
        tol = factor * TG.err(ref[k], g64[k])
        e = TG.err(p.grad.cpu(), g64[k])
        print(f"tail_grad wiring {prec} {k[len(TG.P):]}: err {e:.3e} tol {tol:.3e}")
        assert 0.0 < tol < 1.0
        if not e <= tol:
            bad.append((k, e, tol))
    assert not bad, bad
    # the mapper, as test_gpu_score_grad.py bounds it: the embedding-gradient bound of these inputs
    gx64 = G.grad_of(WIRE, "", "fp64", xd, km, tg, w)
    tol = factor * G.err(G.grad_of(WIRE, "", kind, xd, km, tg, w), gx64) * VIDEO_DIM
    obj = G._objective(SC.masked_forward(SC.sd64(WIRE.E, WIRE.V), SC.arch(WIRE.E, WIRE.V), x, km), tg, w)
    obj.backward()
    e, eb = G.err(lin.weight.grad.cpu(), lin64.weight.grad), G.err(lin.bias.grad.cpu(), lin64.bias.grad)
    print(f"tail_grad wiring {prec} mapper: weight.grad err {e:.3e} bias.grad err {eb:.3e} tol {tol:.3e}")
    assert e <= tol and eb <= tol


@pytest.mark.parametrize("prec", PRECS)
def test_trainer_with_an_unfrozen_tail_lowers_the_loss_and_round_trips(prec):
    from vcap import train as T
    dec = new_text_decoder(prec)            # its weights are trained here: not shared
    sd = SC.state_dict(WIRE.E, WIRE.V)
    ar = SC.arch(WIRE.E, WIRE.V)
    emb, ids, pad = wiring_batch()
    tr = T.MapperTrainer(dec, sd, pad_id=pad, dropout=0.0, unfreeze_gpt2_last=2, lr_gpt2=1e-5)
    assert [g["lr"] for g in tr.optimizer.param_groups] == [3e-4, 1e-5]
    assert all(g["weight_decay"] == 0.01 for g in tr.optimizer.param_groups)
    assert len(tr.optimizer.param_groups[1]["params"]) == 24
    first = tr.evaluate(emb, ids)
    for _ in range(20):
        tr.step(emb, ids)
    last = tr.evaluate(emb, ids)
    # the CPU fp64 replica of the same two-group AdamW loop
    lin64 = linear_from(sd, torch.float64)
    sd64 = TG.leaves_of(SC.sd64(WIRE.E, WIRE.V), dec.hip.tail_names(2))
    opt = torch.optim.AdamW([{"params": list(lin64.parameters()), "lr": 3e-4},
                             {"params": [sd64[k] for k in dec.hip.tail_names(2)], "lr": 1e-5}], weight_decay=0.01)
    first64 = float(replica_loss(lin64, emb, ids, pad, sd64))
    for _ in range(20):
        opt.zero_grad()
        replica_loss(lin64, emb, ids, pad, sd64).backward()
        opt.step()
    last64 = float(replica_loss(lin64, emb, ids, pad, sd64))
    print(f"tail_grad trainer {prec}: device {first:.4f} -> {last:.4f}, fp64 replica {first64:.4f} -> {last64:.4f}")
    assert first64 - last64 > 0
    assert first - last >= 0.5 * (first64 - last64)
    # state_dict() carries the trained tail; loading it into a decoder built from the original weights gives
    # the trained decoder's bits
    state = tr.state_dict()
    assert set(state) == {T.MAPPER_W, T.MAPPER_B, *dec.hip.tail_names(2)}
    moved = [k for k in dec.hip.tail_names(2) if not torch.equal(state[k], torch.from_numpy(sd[k]))]
    assert len(moved) == 24
    other = HipGPT2Decoder(sd, ar, prec, "cuda", screen=False)
    other.load_tail(state)
    c = TG.MASKS[2]
    x, km, tg, _ = TG.inputs(c)
    a, b = dec.hip.score(x, km, tg, want_logits=True), other.score(x, km, tg, want_logits=True)
    assert torch.equal(a.logits.view(torch.int32), b.logits.view(torch.int32))


@pytest.mark.parametrize("prec", PRECS)
def test_trainer_without_a_tail_is_the_mapper_trainer_bit_for_bit(prec):
    from vcap import train as T
    dec = text_decoder(prec)
    sd = SC.state_dict(WIRE.E, WIRE.V)
    emb, ids, pad = wiring_batch()
    plain = T.MapperTrainer(dec, sd, pad_id=pad, dropout=0.0)
    zero = T.MapperTrainer(dec, sd, pad_id=pad, dropout=0.0, unfreeze_gpt2_last=0)
    assert not zero.tail and len(zero.optimizer.param_groups) == 1
    a = [plain.step(emb, ids) for _ in range(3)]
    b = [zero.step(emb, ids) for _ in range(3)]
    assert a == b
    assert set(zero.state_dict()) == {T.MAPPER_W, T.MAPPER_B}
