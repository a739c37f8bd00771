"""The CPU side of GPT-2 tail fine-tuning (vcap_gpt2_score_backward_tail): the fp64 weight-gradient oracle of
tests/tail_grad_cases.py against central finite differences, the bf16 emulation with its roundings switched
off against the plain forward, the CPU-derived per-tensor tolerances of the GPU tests, the training script's
flags, the Python surface and the binding, and the tail call's own argument refusals through the C ABI (no
GPU: every row is refused before the first launch)."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import score_cases as SC
import score_grad_cases as G
import tail_grad_cases as TG
from vcap import _native as N

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------- 1. the oracle against finite differences
def test_oracle_equals_central_differences_on_every_tensor():
    c = TG.MASKS[2]                       # 13 positions, interior mask
    ar = SC.arch(c.E, c.V)
    x, km, tg, w = TG.inputs(c)
    g64 = TG.oracle(c)
    base = SC.sd64(c.E, c.V)
    gen = torch.Generator().manual_seed(5)
    names = TG.tail_names(ar.n_layer, ar.n_layer)
    assert len(names) == 24 and len(set(n.split(".", 5)[5] for n in names)) == 12
    worst = 0.0
    with torch.no_grad():
        for name in names:
            flat = g64[name].reshape(-1)
            # the entry of largest gradient and two seeded ones
            picks = [int(flat.abs().argmax())] + torch.randint(0, flat.numel(), (2,), generator=gen).tolist()
            for i in picks:
                h = 1e-5 * max(1.0, abs(float(base[name].reshape(-1)[i])))
                vals = []
                for sgn in (1.0, -1.0):
                    sd = dict(base)
                    t = base[name].clone()
                    t.reshape(-1)[i] += sgn * h
                    sd[name] = t
                    vals.append(float(G._objective(SC.masked_forward(sd, ar, x.double(), km), tg, w)))
                fd = (vals[0] - vals[1]) / (2 * h)
                e = abs(fd - float(flat[i])) / float(flat.abs().max())
                worst = max(worst, e)
                assert e <= 1e-6, (name, i, fd, float(flat[i]))
    print(f"tail_grad oracle vs central differences: worst error {worst:.3e} of the tensor's max |g|")


def test_hooked_forward_without_rounding_equals_masked_forward(monkeypatch):
    c = TG.MASKS[1]
    monkeypatch.setattr(G.DS, "bf16_rne", lambda t: t)
    got = TG.param_grads_of(c, "rand", "bf16", sd=SC.sd64(c.E, c.V))    # the unrounded weights as leaves
    want = TG.oracle(c)
    for k in want:
        assert TG.err(got[k], want[k]) <= 1e-12, k


# ---------------------------------------------------------------------------------------- 2. tolerances
@pytest.mark.parametrize("c", TG.CASES, ids=lambda c: c.name)
def test_every_tensor_tolerance_is_usable(c):
    t32, t16 = TG.tolerance(c, "rand", "fp32"), TG.tolerance(c, "rand", "bf16")
    assert set(t32) == set(t16) == set(TG.tail_names(2, 2))
    lo32, hi32 = min(t32.values()), max(t32.values())
    lo16, hi16 = min(t16.values()), max(t16.values())
    print(f"tail_grad tolerance {c.name}: fp32 {lo32:.3e} .. {hi32:.3e}, bf16 {lo16:.3e} .. {hi16:.3e}")
    for k in t32:
        assert bool((TG.oracle(c)[k] != 0).any()), k
        assert 0.0 < t32[k] < 1.0, (k, t32[k])
        assert 0.0 < t16[k] < 1.0, (k, t16[k])


def test_ignored_case_has_an_all_zero_oracle():
    g = TG.oracle(TG.IGNORED, "null")
    assert all(bool((v == 0).all()) for v in g.values())
    assert all(t == 0.0 for t in TG.tolerance(TG.IGNORED, "null", "fp32").values())


def test_cases_cover_the_row_steps_and_widths():
    assert sorted(c.B * c.S for c in TG.ROWS) == [1, 31, 32, 33, 63, 64, 65, 129, 512]
    assert [c.E for c in TG.WIDTHS] == [128, 256, 384, 768, 1024]
    assert [c.mask for c in TG.MASKS] == ["none", "right", "interior"]


# -------------------------------------------------------------------------------------------- 3. script
def test_script_accepts_the_tail_flags_and_still_refuses_bos():
    from scripts import train_caption_mapper as S
    a = S.build_argparser().parse_args(["--unfreeze_gpt2_last", "2", "--lr_gpt2", "1e-5"])
    assert a.unfreeze_gpt2_last == 2 and a.lr_gpt2 == 1e-5
    assert S.build_argparser().parse_args([]).lr_gpt2 == 1e-5
    with pytest.raises(SystemExit) as ei:       # the tail flag is not what stops this call
        S.main(["--unfreeze_gpt2_last", "2", "--lr_gpt2", "1e-5", "--cond_mode", "bos"])
    assert "cond_mode bos" in str(ei.value) and "unfreeze" not in str(ei.value)
    with pytest.raises(SystemExit) as ei:
        S.main(["--cond_mode", "bos"])
    assert "cond_mode bos" in str(ei.value)


# ------------------------------------------------------------------------------------------- 4. surface
def test_train_module_exposes_the_tail_surface():
    import inspect

    from vcap import train as T
    from vcap.model import HipGPT2Decoder
    assert issubclass(T.ScoreLogProbsTail, torch.autograd.Function)
    sig = inspect.signature(T.MapperTrainer.__init__).parameters
    assert sig["unfreeze_gpt2_last"].default == 0 and sig["lr_gpt2"].default == 1e-5
    assert "tail" in inspect.signature(T.compute_loss).parameters
    assert "tail" in inspect.signature(T.lm_loss).parameters
    assert callable(T.tail_parameters) and callable(T.MapperTrainer.load_tail)
    for name in ("score_backward_tail", "load_tail", "tail_names"):
        assert callable(getattr(HipGPT2Decoder, name))
    assert list(inspect.signature(HipGPT2Decoder.score_backward_tail).parameters)[1:6] == [
        "embeds", "key_mask", "targets", "grad_logprob", "n_tail"]
    assert HipGPT2Decoder.TAIL_PARAMS == TG.PARAMS


def _header_arg_count(name: str) -> int:
    text = (ROOT / "include" / "vcap.h").read_text()
    m = re.search(r"\b" + name + r"\(([^;]*?)\);", text, re.S)
    assert m, f"{name} is not declared in include/vcap.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", ["vcap_gpt2_score_backward_tail_workspace_bytes", "vcap_gpt2_score_backward_tail",
                                  "vcap_gpt2_weight_grad"])
def test_binding_declares_the_header_signature(name):
    assert name in N.SIGNATURES
    assert len(N.SIGNATURES[name][1]) == _header_arg_count(name)
    assert hasattr(N.lib(), name)


def test_param_grads_struct_matches_the_header():
    text = (ROOT / "include" / "vcap.h").read_text()
    m = re.search(r"typedef struct vcap_gpt2_param_grads_layer \{(.*?)\} vcap_gpt2_param_grads_layer;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"\*(\w+)", body)
    assert fields == [f for f, _ in N.GPT2ParamGradsLayer._fields_]
    assert C.sizeof(N.GPT2ParamGradsLayer) == 12 * C.sizeof(C.c_void_p)
    assert N.ABI_VERSION == 16 and N.lib().vcap_abi_version() == 16


# ------------------------------------------------------------------------------------------ 5. refusals
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


def _grad():
    return N.GPT2GradDesc(dtype=N.DT_F32, n_embd=128, n_layer=2, vocab_pad=1024, wte_t=P, layers=_GRADLAYERS)


def _pg(n_tail=2, null_field=None, layers=True):
    ls = (N.GPT2ParamGradsLayer * 2)()
    for i, ly in enumerate(ls):
        for name, _ in N.GPT2ParamGradsLayer._fields_:
            setattr(ly, name, None if (null_field == (i, name)) else P)
    return N.GPT2ParamGrads(n_tail=n_tail, layers=ls if layers else None), ls


def _tail_call(pg, B=2, S=9, ws_bytes=BIG, grad=P, targets=P):
    d, g = _gpt2(), _grad()
    rc = N.lib().vcap_gpt2_score_backward_tail(C.byref(d), C.byref(g), P, B, S, None, targets, None, grad,
                                               None if pg is None else C.byref(pg), None, None, P, ws_bytes, None)
    return rc, (N.lib().vcap_last_error() or b"").decode()


def test_tail_refusals_before_any_launch():
    assert _tail_call(None) == (ARG, "vcap_gpt2_score_backward_tail: param_grads is null")
    pg, _k = _pg(layers=False)
    assert _tail_call(pg) == (ARG, "vcap_gpt2_score_backward_tail: param_grads is null")
    for n in (0, -1, 3):
        pg, _k = _pg(n_tail=n)
        assert _tail_call(pg) == (ARG, "vcap_gpt2_score_backward_tail: n_tail outside 1 .. n_layer")
    for field in ((0, "ln1_g"), (1, "mproj_b"), (1, "fc_w")):
        pg, _k = _pg(null_field=field)
        assert _tail_call(pg) == (ARG, "vcap_gpt2_score_backward_tail: a gradient pointer is null")
    pg, _k = _pg(n_tail=1, null_field=(1, "fc_w"))      # entry 1 is not read with n_tail = 1
    assert _tail_call(pg, ws_bytes=4096)[0] == WS
    pg, _k = _pg()
    assert _tail_call(pg, grad=None) == (ARG, "vcap_gpt2_score_backward_tail: targets and grad_embeds are required")
    assert _tail_call(pg, targets=None)[0] == ARG
    assert _tail_call(pg, B=57) == (UNSUP, "B*S exceeds vcap_gpt2_max_rows()")
    assert _tail_call(pg, B=1, S=65) == (UNSUP, "S exceeds n_positions")
    assert _tail_call(pg, ws_bytes=4096) == (
        WS, "vcap_gpt2_score_backward_tail: workspace too small (vcap_gpt2_score_backward_tail_workspace_bytes)")


def test_product_refusals_before_any_launch():
    call = N.lib().vcap_gpt2_weight_grad
    A = (P + 15) & ~15                         # 16-byte aligned, inside the buffer

    def rc_msg(*a):
        return call(*a), (N.lib().vcap_last_error() or b"").decode()

    assert rc_msg(N.DT_F16, A, A, A, 64, 128, 128, None) == (ARG, "vcap_gpt2_weight_grad: dtype")
    assert rc_msg(N.DT_BF16, None, A, A, 64, 128, 128, None) == (ARG, "vcap_gpt2_weight_grad: null or unaligned pointer")
    assert rc_msg(N.DT_BF16, A, A + 8, A, 64, 128, 128, None)[0] == ARG
    assert rc_msg(N.DT_F32, A, A, A, 0, 128, 128, None) == (ARG, "vcap_gpt2_weight_grad: bad sizes")
    assert rc_msg(N.DT_F32, A, A, A, 513, 128, 128, None) == (UNSUP, "M exceeds vcap_gpt2_max_rows()")
    assert rc_msg(N.DT_F32, A, A, A, 64, 96, 128, None)[0] == UNSUP
    assert rc_msg(N.DT_F32, A, A, A, 64, 128, 192, None)[0] == UNSUP


def test_tail_workspace_query():
    q = N.lib().vcap_gpt2_score_backward_tail_workspace_bytes
    base = N.lib().vcap_gpt2_score_backward_workspace_bytes
    d, g = _gpt2(), _grad()
    b0 = int(base(C.byref(d), C.byref(g), 2, 9))
    one, two = int(q(C.byref(d), C.byref(g), 2, 9, 1)), int(q(C.byref(d), C.byref(g), 2, 9, 2))
    assert b0 < one < two
    # two operand snapshots per unfrozen layer: M * 5E elements (f32 here), each piece rounded up to 256 bytes
    assert two - one >= 18 * 5 * 128 * 4
    for n in (0, 3, -1):
        assert int(q(C.byref(d), C.byref(g), 2, 9, n)) == 0
    assert int(q(C.byref(d), C.byref(g), 57, 9, 1)) == 0
    assert int(q(C.byref(d), C.byref(g), 1, 65, 1)) == 0
    assert int(q(None, C.byref(g), 2, 9, 1)) == 0
    assert int(q(C.byref(d), None, 2, 9, 1)) == 0
