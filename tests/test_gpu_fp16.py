"""The fp16 ViT precision: the reference's own autocast dtype (torch.autocast(float16) around its ViT,
src/models/video_encoder.py:261-264; GPT-2 stays fp32) on the HIP path.

Kernels against torch at the smallest shapes that take every path (partial tiles, prologue / steady
state / tail of the K loop, both GEMM kernels, both attention kernels, both fused kernels), then the
encoder, the pipeline, the tokens and the surface on the golden cases.  Tolerances come from the
fp16 format (11 significand bits: one rounding is 2^-11 relative) and from the CPU oracle run under
fp16 autocast, never from what the kernels give."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import case
from vcap import _native as N
from vcap import fidelity, search
from vcap.model import GenConfig, HipGPT2Decoder, HipPrefix, HipViTEncoder

pytestmark = pytest.mark.gpu

# Teacher-forced raw-logit error of fp16 ViT + fp32 decoder against the reference's fp32 logits: 2 x the
# error of the reference itself under fp16 autocast (CPU oracle on the golden inputs: 0.0009 b16_b8,
# 0.0008 l14_medium) - two correct fp16 implementations differ from each other by about as much as each
# differs from fp32.
FP16_E2E_TOL = 0.002
# max |encoder_out - golden| of the CPU oracle under torch.autocast("cpu", dtype=float16), measured once
# on the golden inputs (the two large cases; the two small ones are computed in the test)
E_REF_MEASURED = {"b16_b8": 1.6e-3, "l14_medium": 1.2e-3}

_M = {}


def _s():
    return torch.cuda.current_stream().cuda_stream


def _rand(shape, seed, scale=1.0, device="cuda"):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=gen) * scale).to(device)


def _ulps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance in fp16 units in the last place between two fp16 tensors (sign-magnitude bit patterns
    mapped to a monotonic integer line; +0 and -0 coincide)."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


def _hf(ga, L=24, beams=1, max_blocks=0):
    c = GenConfig(L, 8, 3, 1.1, ga.eos_token_id, ga.eos_token_id, True, num_beams=beams)
    c.max_blocks = max_blocks
    return c


def _models(device, name, decoder=True):
    """fp16 ViT + prefix (+ fp32 decoder, built when first asked for) of a golden case; one case resident
    at a time."""
    meta, g, va, ga, sd, frames = case(name)
    if name not in _M:
        _M.clear()
        torch.cuda.empty_cache()
        _M[name] = [HipViTEncoder(sd, va, "fp16", device), HipPrefix(sd, ga.n_embd, device=device), None]
    if decoder and _M[name][2] is None:
        _M[name][2] = HipGPT2Decoder(sd, ga, "fp32", device)
    return (meta, g, va, ga, sd, torch.from_numpy(frames).to(device)) + tuple(_M[name])


# ------------------------------------------------------------------------------------- LayerNorm

def _layernorm_f16(x, g, b, eps=1e-6):
    rows, D = x.shape
    y = torch.empty(rows, D, dtype=torch.float16, device=x.device)
    N.check(N.lib().vcap_layernorm(N.DT_F16, x.data_ptr(), D, y.data_ptr(), D, N.ptr(g), N.ptr(b), rows, D, eps, _s()),
            "layernorm")
    return y


@pytest.mark.parametrize("rows,D", [(5, 128), (3, 768)])
def test_layernorm_f16(device, rows, D):
    """f32 rows -> fp16 (D = 128: the scalar kernel; 768: the vector one) against F.layer_norm(x).half():
    within 1 fp16 ulp wherever finite, inf exactly where torch's .half() overflows (no clamp), and
    subnormal results rounded, not flushed."""
    x = _rand((rows, D), 11, 2.0) + 0.5
    g, b = _rand((D,), 12, 0.1) + 1, _rand((D,), 13, 0.1)
    y, ref = _layernorm_f16(x, g, b), F.layer_norm(x, (D,), g, b, 1e-6).half()
    assert torch.isfinite(ref).all() and int(_ulps(y, ref).max()) <= 1
    # outputs beyond 65504
    big = torch.full((D,), 4.0e4, device=device)
    zero = torch.zeros(D, device=device)
    y, ref = _layernorm_f16(x, big, zero), F.layer_norm(x, (D,), big, zero, 1e-6).half()
    assert torch.isinf(ref).any() and not torch.isinf(ref).all()
    assert torch.equal(torch.isinf(y), torch.isinf(ref)) and torch.equal(y[torch.isinf(ref)], ref[torch.isinf(ref)])
    fin = torch.isfinite(ref)
    assert int(_ulps(y[fin], ref[fin]).max()) <= 1
    # outputs around 1e-6: fp16 subnormals (below 6.1e-5)
    small = torch.full((D,), 1.0e-6, device=device)
    y, ref = _layernorm_f16(x, small, zero), F.layer_norm(x, (D,), small, zero, 1e-6).half()
    assert float(ref.float().abs().max()) < 6.1e-5 and int((ref != 0).sum()) > D // 2
    assert int((y != 0).sum()) > D // 2, "subnormal results were flushed to zero"
    assert int(_ulps(y, ref).max()) <= 1


# ------------------------------------------------------------------------------------------ GEMM

GM, GN, GK = 300, 272, 256    # partial row and column tiles of both kernels; 4 K-tiles: prologue, steady state, tail


def _gemm(in_dt, out_dt, A, W, out, bias, act=0, res=None):
    (m, k), n = A.shape, W.shape[0]
    N.check(N.lib().vcap_gemm(in_dt, out_dt, A.data_ptr(), k, W.data_ptr(), k, out.data_ptr(), n, m, n, k,
                              N.ptr(bias), act, N.ptr(res), n if res is not None else 0, 1 if res is not None else 0,
                              0, 0, 0, 0, _s()), "vcap_gemm")
    return out


@pytest.mark.parametrize("policy", [1, 2])
def test_gemm_f16(device, policy):
    """vcap_gemm with F16 operands under the 128x128 (policy 1) and the 256x256 kernel (policy 2).

    F16 out against torch on the same fp16 operands, |d| <= 2^-10 |ref| + 1e-7: one fp16 rounding of an
    f32-accumulated value is 2^-11 relative.  The torch product is taken in fp64: torch's own fp32 matmul
    is up to 1.3e-6 away from the exact product at this K (its summation error, 13 x the absolute term of
    the bound, which outputs near zero - cancelling sums - then miss through the reference's error alone);
    the exact product asks no less of the kernel.  The GELU epilogue rounds twice (its input, as autocast's
    Linear does, and its output).  The first of the two passes through the GELU, whose relative condition
    number k(x) = |x gelu'(x) / gelu(x)| is 1 at 0, up to 1.3 for x > 0 and grows without bound for x < 0
    (5 at x = -2.3), so 2^-10 |ref| holds only where k is close to 1: that check runs on operands scaled to
    |pre-activation| < 0.5 (k <= 1.2; on CPU the same roundings reach 0.96 of the bound), and a second GELU
    check at ViT-like magnitudes (|x| up to 2.5) uses the bound the two roundings really give,
    (k(x) + 1) 2^-11 |ref| + 1e-7.
    F32 out: accumulator + bias is rounded to fp16 BEFORE the f32 residual is added (with a zero residual
    every output is an fp16 value), and the in-place add is one f32 add of that value."""
    A = _rand((GM, GK), 51).half()
    b = _rand((GN,), 53, 0.1)
    W = _rand((GN, GK), 52, 0.03).half()
    pre = A.double() @ W.double().t() + b.double()
    try:
        N.check(N.lib().vcap_set_gemm_policy(policy), "policy")
        out = _gemm(N.DT_F16, N.DT_F16, A, W, torch.empty(GM, GN, dtype=torch.float16, device=device), b)
        d, bound = (out.double() - pre).abs(), 2.0 ** -10 * pre.abs() + 1e-7
        print(f"policy {policy} bias: max |d| / bound {float((d / bound).max()):.3f}")
        assert bool((d <= bound).all())
        # GELU, small pre-activations: the bound of two roundings
        Ws, bs = _rand((GN, GK), 52, 0.005).half(), _rand((GN,), 53, 0.05)
        ref = F.gelu(A.double() @ Ws.double().t() + bs.double(), approximate="tanh")
        out = _gemm(N.DT_F16, N.DT_F16, A, Ws, torch.empty(GM, GN, dtype=torch.float16, device=device), bs, act=1)
        d, bound = (out.double() - ref).abs(), 2.0 ** -10 * ref.abs() + 1e-7
        print(f"policy {policy} gelu (|x| < 0.5): max |d| / bound {float((d / bound).max()):.3f}")
        assert bool((d <= bound).all())
        # GELU, ViT-like pre-activations: the condition-number bound
        x64 = pre.clone().requires_grad_(True)
        g64 = F.gelu(x64, approximate="tanh")
        g64.sum().backward()
        kappa = (x64 * x64.grad / g64).abs().detach()
        out = _gemm(N.DT_F16, N.DT_F16, A, W, torch.empty(GM, GN, dtype=torch.float16, device=device), b, act=1)
        d = (out.double() - g64.detach()).abs()
        bound = (kappa + 1) * 2.0 ** -11 * g64.detach().abs() + 1e-7
        print(f"policy {policy} gelu (|x| < {float(x64.abs().max()):.1f}): max |d| / bound {float((d / bound).max()):.3f}")
        assert bool((d <= bound).all())
        # F32 out: rounded before the residual add
        z = _gemm(N.DT_F16, N.DT_F32, A, W, torch.zeros(GM, GN, device=device), b, res=None)
        assert torch.equal(z.half().float(), z)
        x = torch.zeros(GM, GN, device=device)
        _gemm(N.DT_F16, N.DT_F32, A, W, x, b, res=x)
        assert torch.equal(x.half().float(), x) and torch.equal(x, z)
        x = _rand((GM, GN), 54)
        x0 = x.clone()
        _gemm(N.DT_F16, N.DT_F32, A, W, x, b, res=x)
        assert torch.equal(x, x0 + z)       # the residual add is one f32 add of the rounded value
    finally:
        N.check(N.lib().vcap_set_gemm_policy(0), "policy")


@pytest.mark.parametrize("n", [GN, 288])
def test_gemm_f16_policies_bit_identical(device, n):
    """The 128- and 256-tile kernels give the same bits: F16 out (bias, GELU) and F32 out with an in-place
    residual (the CU-mask-dependent split between them cannot change an fp16 encode).  N = 272 takes the
    256-tile kernel's 8-byte-store epilogue; N = 288 (a multiple of 32, still a partial column tile) its
    16-byte-store one, the branch QKV and fc1 take in the encoder."""
    A, W, b = _rand((GM, GK), 61).half(), _rand((n, GK), 62, 0.03).half(), _rand((n,), 63, 0.1)
    outs = []
    try:
        for pol in (1, 2):
            N.check(N.lib().vcap_set_gemm_policy(pol), "policy")
            o0 = _gemm(N.DT_F16, N.DT_F16, A, W, torch.empty(GM, n, dtype=torch.float16, device=device), b)
            o1 = _gemm(N.DT_F16, N.DT_F16, A, W, torch.empty(GM, n, dtype=torch.float16, device=device), b, act=1)
            x = _rand((GM, n), 64)
            _gemm(N.DT_F16, N.DT_F32, A, W, x, b, res=x)
            o2 = _gemm(N.DT_F16, N.DT_F32, A, W, torch.empty(GM, n, device=device), b, act=1)   # GELU, f32 out
            assert torch.equal(o2.half().float(), o2)
            outs.append((o0, o1, x, o2))
    finally:
        N.check(N.lib().vcap_set_gemm_policy(0), "policy")
    for i, (a, c) in enumerate(zip(*outs)):
        assert torch.equal(a, c), (i, int((a != c).sum()))


def _splitk(dt, A, W, C, bias, G, Gs):
    m, k = A.shape
    n = W.shape[0]
    ws = torch.empty(8 * m * n, device=C.device)
    import ctypes
    splits = ctypes.c_int(0)
    N.check(N.lib().vcap_gemm_splitk(dt, A.data_ptr(), k, W.data_ptr(), k, C.data_ptr(), n, m, n, k, bias.data_ptr(),
                                     G, Gs, ws.data_ptr(), ws.numel() * 4, ctypes.byref(splits), _s()), "gemm_splitk")
    torch.cuda.synchronize()
    return splits.value


def test_gemm_f16_cls_rows_split_k(device):
    """The in-place residual GEMM of the class-token-only last block: rows remapped to m * tokens (G = 1,
    Gs = tokens), F16 operands, unsplit through vcap_gemm and with the deterministic split-K
    vcap_vit_encode uses (vcap_gemm_splitk; K = 1024 = 16 K-tiles: 4 splits).  In both, accumulator + bias
    is rounded to fp16 and THEN added to the f32 rows - on the split path after the split sum: onto zero
    rows every output is an fp16 value within 2^-10 |ref| + 1e-7 of the exact product, the split and the
    unsplit sums differ by at most one fp16 ulp (a rounding the summation order flips), onto non-zero rows
    the result is that value plus the row in one f32 add, and the other rows stay untouched."""
    BT, NT, D, K = 6, 5, 256, 1024
    A, W, b = _rand((BT, K), 71).half(), _rand((D, K), 72, 0.02).half(), _rand((D,), 73, 0.1)
    ref = A.double() @ W.double().t() + b.double()
    keep = torch.ones(BT * NT, dtype=torch.bool, device=device)
    keep[::NT] = False
    z0 = torch.zeros(BT * NT, D, device=device)
    N.check(N.lib().vcap_gemm(N.DT_F16, N.DT_F32, A.data_ptr(), K, W.data_ptr(), K, z0.data_ptr(), D, BT, D, K,
                              b.data_ptr(), 0, z0.data_ptr(), D, 1, 1, NT, 0, 0, _s()), "cls gemm")
    z1 = torch.zeros(BT * NT, D, device=device)
    splits = _splitk(N.DT_F16, A, W, z1, b, 1, NT)
    assert splits == 4, splits
    for z in (z0, z1):
        assert torch.equal(z.half().float(), z) and not bool(z[keep].any())
        d = (z[::NT].double() - ref).abs()
        assert bool((d <= 2.0 ** -10 * ref.abs() + 1e-7).all())
    assert int(_ulps(z0[::NT].half(), z1[::NT].half()).max()) <= 1
    x = _rand((BT * NT, D), 74)
    x0 = x.clone()
    assert _splitk(N.DT_F16, A, W, x, b, 1, NT) == 4
    assert torch.equal(x, x0 + z1)
    # bf16 operands take the same path without the rounding: the sum itself is added
    Ab, Wb = A.float().bfloat16(), W.float().bfloat16()
    zb = torch.zeros(BT * NT, D, device=device)
    assert _splitk(N.DT_BF16, Ab, Wb, zb, b, 1, NT) == 4
    refb = Ab.double() @ Wb.double().t() + b.double()
    assert float((zb[::NT].double() - refb).abs().max()) < 1e-5
    assert not torch.equal(zb.half().float(), zb)
    # refusals
    lib = N.lib()
    ws = torch.empty(8 * BT * D, device=device)
    args = (A.data_ptr(), K, W.data_ptr(), K, x.data_ptr(), D, BT, D, K, b.data_ptr(), 1, NT, ws.data_ptr())
    assert lib.vcap_gemm_splitk(N.DT_F32, *args, ws.numel() * 4, None, _s()) == N.E_ARG
    assert lib.vcap_gemm_splitk(N.DT_F16, *args, ws.numel() * 4 - 4, None, _s()) == N.E_WORKSPACE


# ------------------------------------------------------------------------------------- attention

def _sdpa(qkv, BT, NT, H):
    q, k, v = qkv.float().reshape(BT, NT, 3, H, 64).permute(2, 0, 3, 1, 4).unbind(0)
    return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(BT * NT, H * 64), float(v.abs().max())


@pytest.mark.parametrize("BT,NT,H", [(3, 197, 2), (2, 257, 1), (3, 50, 2), (1, 100, 1), (1, 170, 2), (1, 240, 1)])
def test_vit_attention_f16(device, BT, NT, H):
    """197 / 257 tokens: the LDS-DMA + transpose-read kernel; 50, 100, 170, 240: the generic kernel at each
    of its key paddings (64, 128, 192, 256).  Against fp32 SDPA on
    the same fp16 q / k / v, atol 2^-10 max|v|: one fp16 rounding of P <= 1 (2^-11 relative per weight of a
    convex combination of V rows) and one of the output."""
    D = H * 64
    qkv = _rand((BT * NT, 3 * D), 15, 1.5).half()
    out = torch.empty(BT * NT, D, dtype=torch.float16, device=device)
    N.check(N.lib().vcap_vit_attention(N.DT_F16, qkv.data_ptr(), out.data_ptr(), BT, NT, H, _s()), "attention")
    ref, vmax = _sdpa(qkv, BT, NT, H)
    err = float((out.float() - ref).abs().max())
    print(f"attention f16 ({BT},{NT},{H}): max err {err:.2e}, bound {2.0 ** -10 * vmax:.2e}")
    assert err <= 2.0 ** -10 * vmax


# --------------------------------------------------------------------------- fused QKV + attention

def _qa_case(device, BT, NT, H, seed, tdt=torch.float16):
    D = H * 64
    g = torch.Generator(device=device).manual_seed(seed)
    xn = torch.randn(BT * NT, D, generator=g, device=device).to(tdt)
    w = (0.05 * torch.randn(3 * D, D, generator=g, device=device)).to(tdt)
    b = 0.05 * torch.randn(3 * D, generator=g, device=device)
    return xn, w, b


def _qa_fused(dt, xn, w, b, BT, NT, H, cls_only):
    out = torch.full((BT * NT, H * 64), float("nan"), device=xn.device, dtype=xn.dtype)
    N.check(N.lib().vcap_vit_qkv_attention_dt(dt, xn.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), BT, NT,
                                              H, cls_only, _s()), "qkv_attention_dt")
    return out


@pytest.mark.parametrize("BT,NT,H", [(8, 208, 12), (3, 193, 12), (2, 197, 1), (8, 257, 16), (2, 260, 4)])
def test_fused_qkv_attention_f16_bit_identical(device, BT, NT, H):
    """vcap_vit_qkv_attention_dt(F16) against vcap_gemm(F16 -> F16) + vcap_vit_attention(F16): every row,
    and the class-token-only form, which writes nothing past its compact rows."""
    D = H * 64
    xn, w, b = _qa_case(device, BT, NT, H, BT * 1000 + NT + H)
    qkv = torch.empty(BT * NT, 3 * D, device=device, dtype=torch.float16)
    ref = torch.empty(BT * NT, D, device=device, dtype=torch.float16)
    lib = N.lib()
    N.check(lib.vcap_gemm(N.DT_F16, N.DT_F16, xn.data_ptr(), D, w.data_ptr(), D, qkv.data_ptr(), 3 * D, BT * NT,
                          3 * D, D, b.data_ptr(), 0, None, 0, 0, 0, 0, 0, 0, _s()), "qkv gemm")
    N.check(lib.vcap_vit_attention(N.DT_F16, qkv.data_ptr(), ref.data_ptr(), BT, NT, H, _s()), "attention")
    out = _qa_fused(N.DT_F16, xn, w, b, BT, NT, H, 0)
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), float((out.float() - ref.float()).abs().max())
    cls = _qa_fused(N.DT_F16, xn, w, b, BT, NT, H, 1)
    want = ref.view(BT, NT, D)[:, 0].contiguous()
    assert torch.equal(cls[:BT].view(torch.int16), want.view(torch.int16))
    assert torch.isnan(cls[BT:].float()).all()


def test_vit_attention_f16_cls_only(device):
    """The class-token-only form at (3, 197, 2) (the C ABI exposes it through the fused entry point): its
    compact rows against fp32 SDPA on the same fp16 q / k / v - those of vcap_gemm(F16 -> F16), which the
    fused kernel's on-chip q / k / v equal bit for bit (test above) - with atol 2^-10 max|v|."""
    BT, NT, H = 3, 197, 2
    D = H * 64
    xn, w, b = _qa_case(device, BT, NT, H, 5)
    cls = _qa_fused(N.DT_F16, xn, w, b, BT, NT, H, 1)[:BT]
    qkv = torch.empty(BT * NT, 3 * D, device=device, dtype=torch.float16)
    N.check(N.lib().vcap_gemm(N.DT_F16, N.DT_F16, xn.data_ptr(), D, w.data_ptr(), D, qkv.data_ptr(), 3 * D, BT * NT,
                              3 * D, D, b.data_ptr(), 0, None, 0, 0, 0, 0, 0, 0, _s()), "qkv gemm")
    ref, vmax = _sdpa(qkv, BT, NT, H)
    err = float((cls.float() - ref.view(BT, NT, -1)[:, 0]).abs().max())
    print(f"attention f16 cls_only ({BT},{NT},{H}): max err {err:.2e}, bound {2.0 ** -10 * vmax:.2e}")
    assert err <= 2.0 ** -10 * vmax


def test_fused_qkv_attention_dt_bf16_is_the_old_entry(device):
    BT, NT, H = 3, 197, 12
    xn, w, b = _qa_case(device, BT, NT, H, 9, torch.bfloat16)
    new = _qa_fused(N.DT_BF16, xn, w, b, BT, NT, H, 0)
    old = torch.full_like(new, float("nan"))
    N.check(N.lib().vcap_vit_qkv_attention(xn.data_ptr(), w.data_ptr(), b.data_ptr(), old.data_ptr(), BT, NT, H, 0,
                                           _s()), "qkv_attention")
    assert torch.equal(new.view(torch.int16), old.view(torch.int16))


def test_fused_qkv_attention_dt_refusals(device):
    xn, w, b = _qa_case(device, 2, 197, 12, 1)
    lib = N.lib()
    for nt in (192, 209, 256, 273):
        assert lib.vcap_vit_qkv_attention_dt(N.DT_F16, xn.data_ptr(), w.data_ptr(), b.data_ptr(), xn.data_ptr(), 2, nt,
                                             12, 0, _s()) == N.E_UNSUPPORTED
    for dt in (N.DT_F32, N.DT_MXFP8, 7):
        assert lib.vcap_vit_qkv_attention_dt(dt, xn.data_ptr(), w.data_ptr(), b.data_ptr(), xn.data_ptr(), 2, 197, 12,
                                             0, _s()) == N.E_ARG


def test_decoder_side_entry_points_refuse_f16(device):
    """The decoder has no fp16 mode: its entry points keep their error codes for VCAP_DT_F16 and never
    read it as a 4-byte element type."""
    lib = N.lib()
    t = torch.zeros(64, 64, device=device)
    assert lib.vcap_rows_packed_bytes(N.DT_F16, 64, 64) == 0
    assert lib.vcap_rows_pack(N.DT_F16, t.data_ptr(), 64, 64, 64, t.data_ptr(), _s()) == N.E_ARG
    assert lib.vcap_decode_attention(N.DT_F16, t.data_ptr(), t.data_ptr(), t.data_ptr(), None, 1, t.data_ptr(), 1, 1,
                                     1, 0, _s()) == N.E_ARG
    assert lib.vcap_mx_quantize(N.DT_F16, t.data_ptr(), 256, 1, 256, t.data_ptr(), t.data_ptr(), _s()) == N.E_ARG
    assert lib.vcap_gemm_mx(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), N.DT_F16, t.data_ptr(), 16, None,
                            1, 16, 256, None, 0, None, _s()) == N.E_ARG
    sd_ga = case("tiny")
    with pytest.raises(ValueError):
        HipGPT2Decoder(sd_ga[4], sd_ga[3], "fp16", device)


# --------------------------------------------------------------------------------------- encoder

@pytest.mark.parametrize("name", ["tiny", "b16_b2", "b16_b8", "l14_medium"])
def test_encoder_fp16_against_the_autocast_reference(device, name):
    """HipViTEncoder(..., "fp16") on the golden frames.  e_hip = max |encoder_out - golden (fp32)|;
    e_ref = the same error of the CPU oracle under torch.autocast(float16), which rounds exactly where the
    reference's autocast does.  e_hip <= 2 e_ref: two correct fp16 implementations differ from each other
    (summation order, rounding flips) by about as much as each differs from fp32.  e_hip <= 0.5 x the bf16
    encoder's error (8 significand bits against 11: the CPU ratio is 6-8x) - fails if fp16 aliases bf16.
    encoder.proj runs inside the autocast block, so every output is an fp16 value."""
    meta, g, va, ga, sd, video, enc, pre, _ = _models(device, name, decoder=False)
    if name in E_REF_MEASURED:
        e_ref = E_REF_MEASURED[name]     # measured on CPU (module constant), too slow to recompute here
    else:
        from oracle import vcap_oracle as O
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.float16):
            ref16 = O.encoder(sd, va, video.cpu())
        e_ref = float(np.abs(ref16.float().numpy() - g["encoder_out"]).max())
    out, _ = enc.encode(video, pre)
    e_hip = float(np.abs(out.cpu().numpy() - g["encoder_out"]).max())
    enc_bf = HipViTEncoder(sd, va, "bf16", device)
    out_bf, _ = enc_bf.encode(video)
    e_bf = float(np.abs(out_bf.cpu().numpy() - g["encoder_out"]).max())
    del enc_bf
    print(f"{name}: e_hip {e_hip:.3e}  e_ref(autocast fp16) {e_ref:.3e}  e_bf16 {e_bf:.3e}")
    assert e_hip <= 2 * e_ref, (e_hip, e_ref)
    assert e_hip <= 0.5 * e_bf, (e_hip, e_bf)
    assert torch.equal(out.half().float(), out)
    if va.tokens in (197, 257):
        assert enc.fuses_qkv_attention() and enc.fuses_qkv_attention(va.depth - 1)


# -------------------------------------------------------------------------------------- pipeline

def test_fp16_pipeline_bit_identical_to_serial(device):
    """The overlapped schedule (CU-masked encode stream, two decode lanes confined to 96 CUs, groups of 2
    batches encoded and decoded together) with the fp16 ViT and the fp32 decoder: prefixes and ids are
    those of a serial encode + decode (M-independent split-K, mask-independent GEMM plans)."""
    from vcap.pipeline import CaptionPipeline
    meta, g, va, ga, sd, video, enc, pre, dec = _models(device, "b16_b8")
    _, pre_serial = enc.encode(video, pre)
    ids_serial = dec.generate_ids(pre_serial, [ga.bos_token_id], _hf(ga)).clone()
    pipe = CaptionPipeline(enc, pre, dec, _hf(ga, max_blocks=96), video.shape[0], [ga.bos_token_id], device,
                           reserve_cus=32, dec_lanes=2, dec_group=2, enc_group=2, confine_decode=96)
    try:
        slots = [pipe.submit(video) for _ in range(5)]
        pipe.synchronize()
        for slot in slots[-2:]:
            assert torch.equal(pipe.result(slot), ids_serial)
            assert torch.equal(pipe.prefix_bufs[slot], pre_serial)
    finally:
        pipe.close()


# ---------------------------------------------------------------------------------------- tokens

def _golden_step(g, s):
    return g[f"hf_greedy_logits_s{s}_top_i"].astype(np.int64), g[f"hf_greedy_logits_s{s}_top_v"]


def _processed_top2_gap(ti, tv, hist, V, eos):
    """Processed (rep 1.1, ngram 3, min_new 8) top-2 gap of the golden raw logits, on the golden top-64."""
    row = torch.full((ti.shape[0], V), -1e30, dtype=torch.float64)
    row.scatter_(1, torch.from_numpy(ti), torch.from_numpy(tv.astype(np.float64)))
    sc = search._processors(row, torch.from_numpy(hist.astype(np.int64)), 1.1, 3, 8, eos)
    top = torch.topk(sc, 2, dim=-1).values
    return (top[:, 0] - top[:, 1]).numpy()


@pytest.mark.parametrize("name,min_certain", [("b16_b8", 4), ("l14_medium", 1)])
def test_fp16_vit_fp32_decoder_tokens(device, name, min_certain):
    """The reference's precision split on the golden clips.  Teacher-forced along the golden greedy ids,
    every raw logit the golden records (top-64 of all 24 steps) within FP16_E2E_TOL; free-running, a
    caption may leave the golden only at a step whose golden processed top-2 gap is <= 2 x tol, so the
    captions whose every gap exceeds that (b16_b8: 1, 2, 4, 6; l14_medium: 0) are identical."""
    meta, g, va, ga, sd, video, enc, pre, dec = _models(device, name)
    ref = g["hf_greedy_ids"]
    B, L, eos = ref.shape[0], ref.shape[1], ga.eos_token_id
    assert meta["hf_greedy_logit_steps"] == 24 == L
    prompt = meta.get("prompt_ids", [ga.bos_token_id])
    _, prefix = enc.encode(video, pre)
    tf = fidelity.teacher_forced_logits(dec, prefix, prompt, torch.from_numpy(ref.astype(np.int64)), L)
    errs = []
    for s in range(L):
        ti, tv = _golden_step(g, s)
        got = torch.gather(tf[s].double(), 1, torch.from_numpy(ti).to(device)).cpu().numpy()
        errs.append(float(np.abs(got - tv).max()))
    print(f"{name} fp16 ViT + fp32 decoder teacher-forced: max |dlogit| per step {np.round(errs, 5).tolist()}")
    got = dec.generate_ids(prefix, prompt, _hf(ga)).cpu().numpy()
    gaps = np.stack([_processed_top2_gap(*_golden_step(g, s), ref[:, :s], ga.vocab, eos) for s in range(L)], 1)
    certain = [b for b in range(B) if gaps[b].min() > 2 * FP16_E2E_TOL]
    same = [b for b in range(B) if np.array_equal(got[b, :L], ref[b])]
    print(f"{name}: captions identical to the golden {len(same)} of {B} {same}; certain {certain}; "
          f"smallest gap per caption {np.round(gaps.min(1), 4).tolist()}")
    assert max(errs) <= FP16_E2E_TOL, errs
    assert len(certain) >= min_certain, certain
    for b in range(B):
        first_div = next((s for s in range(L) if got[b, s] != ref[b, s]), L)
        guard = next((s for s in range(L) if gaps[b, s] <= 2 * FP16_E2E_TOL), L)
        assert first_div >= guard, (b, first_div, guard, gaps[b, :first_div + 1])
    assert set(certain) <= set(same)


def test_l14_medium_beam4_fp16_priced_against_reference(device):
    """configs[3] with the reference's precision split (fp16 ViT-L/14, fp32 device beam-4 search, max_new
    40): the search's best hypothesis scores within 2 x FP16_E2E_TOL of the reference's under fp32."""
    meta, g, va, ga, sd, video, enc, pre, dec = _models(device, "l14_medium")
    cfg = _hf(ga, 40, 4)
    _, pt = enc.encode(video, pre)
    ids = dec.generate_ids(pt, meta["prompt_ids"], cfg).cpu().tolist()
    p32 = torch.from_numpy(g["inputs_embeds"][:, :4].copy()).to(device)
    rep = fidelity.beam_divergence(dec, p32, meta["prompt_ids"], ids, g["beam4_ids"].tolist(), cfg,
                                   tol=2 * FP16_E2E_TOL)
    print(f"l14_medium beam 4, fp16 ViT + fp32 decoder: {rep}")
    assert rep["within_tol"], rep


# --------------------------------------------------------------------------------------- surface

def test_engine_runs_in_fp16(device):
    from core.config import InferenceConfig
    from core.engine import InferenceEngine
    meta, g, va, ga, sd, frames = case("tiny")
    _M.clear()
    cfg = InferenceConfig(vit_name=meta["vit"], gpt2_name=meta["gpt2"], num_frames=meta["T"], precision="fp16",
                          device=str(device), weights_seed=meta["weights_seed"])
    eng = InferenceEngine(cfg)
    assert eng.model.hip_encoder.precision == "fp16" and eng.model.hip_encoder.dt == N.DT_F16
    assert eng.model.decoder_precision == "fp32" and eng.model.decoder.hip.precision == "fp32"
    video = torch.from_numpy(frames).to(device)
    out = eng._generate_once(video, "", num_beams=1, max_new_tokens=24, temperature=1.0, top_p=1.0,
                             no_repeat_ngram_size=3, repetition_penalty=1.1)
    assert isinstance(out, str) and out.strip()
    emb, _ = eng.model.hip_encoder.encode(video)
    assert float(np.abs(emb.cpu().numpy() - g["encoder_out"]).max()) < 5e-3    # an fp16 encode, not garbage


def test_operators_take_fp16(device):
    """core.operators with torch.float16 inputs (and force_fp16 on f32 inputs): the F16 kernels, fp16
    results, within 1 ulp of torch (f32 accumulation, one rounding; the ulp covers the summation order)."""
    from core.operators.hip_linear_mapper import HipLinearCompat
    from core.operators.hip_vit_pool import vit_fused_pool_temporal
    lin = HipLinearCompat(256, 136).to(device).eval()
    with torch.no_grad():
        lin.weight.copy_(_rand((136, 256), 81, 0.05))
        lin.bias.copy_(_rand((136,), 82, 0.1))
    x = _rand((3, 7, 256), 83).half()
    ref = F.linear(x.float(), lin.weight.detach().half().float(), lin.bias.detach()).half()
    with torch.no_grad():
        y = lin(x)
    assert y.dtype == torch.float16 and lin.last_backend == "hip" and tuple(y.shape) == (3, 7, 136)
    assert int(_ulps(y, ref).max()) <= 1
    forced = HipLinearCompat(256, 136, force_fp16=True).to(device).eval()
    forced.load_state_dict(lin.state_dict())
    with torch.no_grad():
        y2 = forced(x.float())
    assert y2.dtype == torch.float16 and torch.equal(y2, y)
    B, T, tok, Cc = 2, 3, 50, 192
    feat = _rand((B * T, tok, Cc), 84).half()
    for pool in ("cls", "gap"):
        got = vit_fused_pool_temporal(feat, B, T, pool)
        fb = feat.float().reshape(B, T, tok, Cc)
        want = (fb[:, :, 0].mean(1) if pool == "cls" else fb[:, :, 1:].mean(dim=(1, 2))).half()
        assert got.dtype == torch.float16 and int(_ulps(got, want).max()) <= 1
        assert torch.equal(vit_fused_pool_temporal(feat.float(), B, T, pool, force_fp16=True), got)
