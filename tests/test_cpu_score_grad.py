"""The CPU side of the scoring call's backward (vcap_gpt2_score_backward): the fp64 autograd oracle of
tests/score_grad_cases.py against HF's own autograd, the exact-zero properties in the oracle, the CPU-derived
tolerances of the GPU tests, and the argument refusals of the two new entry points through the C ABI (no
GPU: every row is refused before the first launch)."""
import ctypes as C

import pytest
import torch

import score_cases as SC
import score_grad_cases as G
from vcap import _native as N


# ------------------------------------------------------------------------------- 1. the oracle against HF
@pytest.mark.parametrize("mask", ["interior", "right"])
def test_oracle_gradient_equals_hf_autograd(mask):
    transformers = pytest.importorskip("transformers")
    c = SC.Case(f"hf_{mask}", 128, 1009, 3, 13, mask)
    ar = SC.arch(c.E, c.V)
    cfg = transformers.GPT2Config(vocab_size=c.V, n_positions=ar.n_positions, n_embd=c.E, n_layer=ar.n_layer,
                                  n_head=ar.n_head, activation_function="gelu_new", resid_pdrop=0.0, embd_pdrop=0.0,
                                  attn_pdrop=0.0, layer_norm_epsilon=ar.ln_eps)
    cfg._attn_implementation = "eager"
    model = transformers.GPT2LMHeadModel(cfg).double().eval()
    pre = "decoder.model."
    state = {k[len(pre):]: v for k, v in SC.sd64(c.E, c.V).items() if k.startswith(pre)}
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all(k.endswith(("attn.bias", "attn.masked_bias")) for k in missing), (missing, unexpected)
    x, km = SC.embeds(c).double().requires_grad_(True), SC.key_mask(c)
    tg = SC.targets(c).clone()
    tg[:, -1] = SC.IGNORE                      # HF's shift scores nothing at the last position
    labels = torch.cat([torch.full((c.B, 1), SC.IGNORE), tg[:, :-1]], dim=1)
    out = model(inputs_embeds=x, attention_mask=km.long(), labels=labels)
    count = int((tg >= 0).sum())
    w = torch.full(tg.shape, -1.0 / count, dtype=torch.float64)
    # HF's loss casts the logits to float32 before its cross-entropy (transformers loss_utils: "upcast to
    # float"), so the gradient of out.loss is float32-limited whatever the model's dtype (2.3e-8 here).  The
    # fp64 comparison therefore takes HF's own graph up to out.logits and the same shifted cross-entropy in
    # fp64 on top; out.loss itself is checked to float32 accuracy.
    loss_hf = G._objective(out.logits, tg, w)
    assert abs(float(out.loss) - float(loss_hf)) <= 1e-6 * abs(float(loss_hf))
    (g_hf,) = torch.autograd.grad(loss_hf, x)
    g = G.grad_of(c, "", "fp64", x.detach(), km, tg, w)
    e = G.err(g, g_hf)
    print(f"oracle vs HF autograd ({mask}): err {e:.3e}")
    assert e <= 1e-10


# --------------------------------------------------------------------------------- 2. exact zeros, fp64
@pytest.mark.parametrize("c", G.CASES + G.IGNORED, ids=lambda c: c.name)
def test_oracle_has_the_exact_zeros(c):
    g = G.oracle_grad(c, "rand")
    z = G.zero_positions(c)
    assert bool((g[z] == 0).all())
    if c.targets == "ignored":
        assert bool(z.all())


def test_zero_positions_cover_the_three_classes():
    z = G.zero_positions(G.MASKS[2])            # interior: hidden keys with an ignored target
    tg, km = G.targets(G.MASKS[2]), SC.key_mask(G.MASKS[2])
    assert bool(((km == 0) & (tg < 0) & z).any())
    c = G.SHAPES[3]                             # edges: position S - 2 ignored, S - 1 counted for the last sequence
    last = G.last_counted(G.targets(c), c.V)
    assert last.tolist()[-1] == c.S - 1


# ---------------------------------------------------------------------------------------- 3. tolerances
@pytest.mark.parametrize("c,wmode", [(c, "rand") for c in G.CASES] + [(c, "null") for c in G.MASKS],
                         ids=lambda v: v if isinstance(v, str) else v.name)
def test_cpu_tolerances_are_finite_and_nonzero(c, wmode):
    t32, t16 = G.tolerance(c, wmode, "fp32"), G.tolerance(c, wmode, "bf16")
    print(f"score_grad tolerance {c.name} w={wmode}: fp32 {t32:.3e} (cpu f32 err {t32 / G.F32_FACTOR:.3e}), "
          f"bf16 {t16:.3e} (emulation err {t16 / G.BF16_FACTOR:.3e})")
    assert 0.0 < t32 < 1e-3
    assert t32 < t16 < 0.2


# ------------------------------------------------------------------------------------------ 4. refusals
ARG, WS, UNSUP = N.E_ARG, N.E_WORKSPACE, N.E_UNSUPPORTED
_BUF = C.create_string_buffer(4096)
P = C.addressof(_BUF)                      # a non-null address no refused call reads
_GLAYERS = (N.GPT2Layer * 2)()
_GRADLAYERS = (N.GPT2GradLayer * 2)()
for _ly in _GRADLAYERS:
    for _name, _ in N.GPT2GradLayer._fields_:
        setattr(_ly, _name, P)
BIG = 1 << 40


def _gpt2(**kw):
    f = dict(dtype=N.DT_F32, n_embd=128, n_layer=2, n_head=2, vocab=1009, n_positions=64, prefix_len=4, ln_eps=1e-5,
             wte=P, lm_head=P, wpe=P, lnf_g=P, lnf_b=P, layers=_GLAYERS, lm_head_screen=None, screen_bound=0.0)
    f.update(kw)
    return N.GPT2Desc(**f)


def _grad(**kw):
    f = dict(dtype=N.DT_F32, n_embd=128, n_layer=2, vocab_pad=1024, wte_t=P, layers=_GRADLAYERS)
    f.update(kw)
    return N.GPT2GradDesc(**f)


GOOD = dict(d=_gpt2, g=_grad, embeds=P, B=2, S=9, mask=None, targets=P, w=None, grad=P, logprob=None, loss=None, ws=P,
            ws_bytes=BIG, stream=None)

# (the argument made bad, code, vcap_last_error() text): one row per distinct refusal
ROWS = [
    (dict(d=None), ARG, "gpt2 desc is null"),
    (dict(desc=dict(dtype=N.DT_MXFP8)), ARG, "gpt2 dtype"),
    (dict(desc=dict(n_embd=192), gdesc=dict(n_embd=192)), UNSUP, "gpt2 head_dim must be 64"),
    (dict(desc=dict(n_embd=1152, n_head=18), gdesc=dict(n_embd=1152)), UNSUP,
     "n_embd > 1024 (LayerNorm rows are held in registers)"),
    (dict(desc=dict(wte=None)), ARG, "gpt2 wte / lm_head / wpe / ln_f pointer is null"),
    (dict(g=None), ARG, "gpt2 grad desc is null"),
    (dict(gdesc=dict(layers=None)), ARG, "gpt2 grad desc is null"),
    (dict(gdesc=dict(dtype=N.DT_BF16)), ARG, "gpt2 grad desc: dtype / n_embd / n_layer differ from the decoder's"),
    (dict(gdesc=dict(n_layer=3)), ARG, "gpt2 grad desc: dtype / n_embd / n_layer differ from the decoder's"),
    (dict(gdesc=dict(vocab_pad=1009)), ARG, "gpt2 grad desc: vocab_pad is not the vocabulary rounded up to 128"),
    (dict(gdesc=dict(wte_t=None)), ARG, "gpt2 grad desc: a weight pointer is null"),
    (dict(embeds=None), ARG, "vcap_gpt2_score_backward: bad arguments"),
    (dict(B=0), ARG, "vcap_gpt2_score_backward: bad arguments"),
    (dict(S=0), ARG, "vcap_gpt2_score_backward: bad arguments"),
    (dict(ws=None), ARG, "vcap_gpt2_score_backward: bad arguments"),
    (dict(targets=None), ARG, "vcap_gpt2_score_backward: targets and grad_embeds are required"),
    (dict(grad=None), ARG, "vcap_gpt2_score_backward: targets and grad_embeds are required"),
    (dict(B=57), UNSUP, "B*S exceeds vcap_gpt2_max_rows()"),                  # 57 * 9 = 513 rows
    (dict(B=1, S=65), UNSUP, "S exceeds n_positions"),
    (dict(ws_bytes=4096), WS,
     "vcap_gpt2_score_backward: workspace too small (vcap_gpt2_score_backward_workspace_bytes)"),
]


def _call(bad):
    a = dict(GOOD)
    desc, gdesc = bad.pop("desc", {}), bad.pop("gdesc", {})
    a.update(bad)
    d = a["d"](**desc) if a["d"] is not None else None
    g = a["g"](**gdesc) if a["g"] is not None else None
    rc = N.lib().vcap_gpt2_score_backward(None if d is None else C.byref(d), None if g is None else C.byref(g),
                                          a["embeds"], a["B"], a["S"], a["mask"], a["targets"], a["w"], a["grad"],
                                          a["logprob"], a["loss"], a["ws"], a["ws_bytes"], a["stream"])
    return rc, (N.lib().vcap_last_error() or b"").decode()


@pytest.mark.parametrize("bad,code,msg", ROWS, ids=[f"{i}_{list(r[0])[0]}" for i, r in enumerate(ROWS)])
def test_score_backward_refusals(bad, code, msg):
    rc, text = _call(dict(bad))
    assert (rc, text) == (code, msg)


def test_workspace_query_is_zero_outside_the_limits():
    q = N.lib().vcap_gpt2_score_backward_workspace_bytes
    d, g = _gpt2(), _grad()
    inside = int(q(C.byref(d), C.byref(g), 2, 9))
    assert inside > int(N.lib().vcap_gpt2_score_workspace_bytes(C.byref(d), 2, 9)) > 0
    assert int(q(C.byref(d), C.byref(g), 56, 9)) > inside          # 504 rows
    assert int(q(C.byref(d), C.byref(g), 57, 9)) == 0              # 513 rows
    assert int(q(C.byref(d), C.byref(g), 1, 65)) == 0              # S > n_positions
    assert int(q(C.byref(d), C.byref(g), 0, 9)) == 0
    assert int(q(C.byref(d), None, 2, 9)) == 0
    assert int(q(None, C.byref(g), 2, 9)) == 0
    bad = _grad(vocab_pad=1152)
    assert int(q(C.byref(d), C.byref(bad), 2, 9)) == 0
    wide = _gpt2(n_embd=1152, n_head=18)
    assert int(q(C.byref(wide), C.byref(_grad(n_embd=1152)), 2, 9)) == 0
