"""MXFP8 kernel sweep through the C ABI: every kernel instance, tile edge and epilogue of the fp8 ViT path
against an exact or fp64 oracle (tests/mx_cases.py derives every bound; tests/test_cpu_mx_cases.py pins the
oracle and the conditions on the CPU; DESIGN.md "MXFP8 shapes" lists which case reaches which instance).
pytest -s prints the instance / template each case reached - as mx_cases.template_of / attention_instance restate
the dispatchers (csrc/gemm256.hip launch256, csrc/vit_attention.hip attn_bf16_dispatch), not as observed from the
launch: a change of a dispatcher has to be carried into those two functions.

  1 vcap_mx_quantize, f32 and bf16 input, rows 1..513 (the partial 4-row workgroup, one to three 256-row scale
    groups), K 256 / 512 / 1280, ldx = K and K + 8: bytes and scales bit-identical to the oracle on the
    constructed blocks (ties, power-of-two maxima, zero and -0.0, scale byte 0, f32 subnormals, FLT_MAX) and on
    spread random rows; nothing written past rows * K bytes of q or past vcap_mx_scale_bytes.  Non-finite input
    as include/vcap.h states it.
  2 vcap_layernorm_mx, D 256..1024 (nv = 1..4), rows 1 / 5 / 257, ldx = D and 3 D, with and without affine, a
    constant row and a large-mean row: the oracle's bytes and scales except inside the window an f32 LayerNorm
    cannot decide, at most 0.1 % of a case.
  3 vcap_gemm_mx: the five epilogue templates of vcap_gemm256_kernel, M 1..300, N 16..384, K 256..1280, ldc = N
    and N + 16, on rotating-live-block and dense operands, against float64 dequant(A) . dequant(W)^T.  Template 4
    (GELU -> MXFP8) runs on rotating and on "unit" operands instead of dense ones: unspread normal A, W x 0.05,
    as tests/test_gpu_mx.py's GELU test - pre-activations spread over 2^+-24 leave the GELU either the identity
    or zero, with nothing for the re-quantisation to get wrong.
  4 vcap_vit_attention_mx at heads = 4, frames = 2: all five template instances on random q / k / v against the
    fp64 attention (the one-hot patterns: tests/test_gpu_attention_edges.py, precision "mxfp8").  The KE = 14
    and KE = 18 instances cannot be reached from an encode (no square grid gives 209..224 or 273..288 tokens):
    this section and the edge patterns are their only runs.
  5 one transformer block stage by stage on the GPU's own intermediates: each stage against its oracle applied
    to the GPU's actual input to that stage, the scale buffer reused as the encode reuses xn_s."""
import numpy as np
import pytest
import torch

import attention_edge_cases as A
import encoder_shapes as ES
import mx_cases as MX
from oracle import vcap_oracle as O
from vcap import _native as N
from vcap import weights

pytestmark = pytest.mark.gpu
SENT, FSENT = 0xA5, -776.0                       # byte sentinel; float sentinel (exact in bf16)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _scale_bytes(rows, K):
    return int(N.lib().vcap_mx_scale_bytes(rows, K))


def _quantize(dev, x, bf16=False, ldx=None, fill=SENT):
    """x f32 numpy [rows, K] -> (q [rows + 2, K] with two sentinel rows, scale buffer with 64 sentinel bytes)."""
    rows, K = x.shape
    ldx = ldx or K
    buf = np.full((rows, ldx), 7.0, np.float32)
    buf[:, :K] = x
    xt = torch.from_numpy(buf).to(dev)
    if bf16:
        xt = xt.bfloat16()
        assert np.array_equal(xt.float().cpu().numpy()[:, :K], x, equal_nan=True)
    q = torch.full((rows + 2, K), SENT, dtype=torch.uint8, device=dev)
    sc = torch.full((_scale_bytes(rows, K) + 64,), fill, dtype=torch.uint8, device=dev)
    N.check(N.lib().vcap_mx_quantize(N.DT_BF16 if bf16 else N.DT_F32, xt.data_ptr(), ldx, rows, K, q.data_ptr(),
                                     sc.data_ptr(), _s()), "quantize")
    torch.cuda.synchronize()
    return q, sc


def _unpack(sc, rows, K):
    return O.mx_unpack_scales(sc.cpu().numpy()[:_scale_bytes(rows, K)], rows, K)


def _check_quantised(q, sc, x, names):
    rows, K = x.shape
    qo, so = O.mx_quantize(x)
    qg, sg = q.cpu().numpy(), _unpack(sc, rows, K)
    assert np.array_equal(sg, so), MX.first_mismatch(sg, so, names, 1)
    assert np.array_equal(qg[:rows], qo), MX.first_mismatch(qg[:rows], qo, names, 32)
    assert (qg[rows:] == SENT).all(), "q rows >= rows written"
    assert (sc.cpu().numpy()[_scale_bytes(rows, K):] == SENT).all(), "scale bytes past vcap_mx_scale_bytes written"


# ---------------------------------------------------------------------------------------------- 1 quantiser
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_quantize_constructed_blocks(device, bf16):
    """Every constructed block (mx_cases.special_blocks) bit-exact, for both instantiations of
    vcap_mx_quantize_kernel; a failure names the block."""
    x, names = MX.special_rows(256, bf16)
    for ldx in (256, 264):
        q, sc = _quantize(device, x, bf16, ldx)
        _check_quantised(q, sc, x, names)
    print(f"\nmx-quantize {'bf16' if bf16 else 'f32'}: {sum(n != 'random' for r in names for n in r)} constructed blocks", end="")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [256, 512, 1280])
@pytest.mark.parametrize("rows", [1, 3, 255, 256, 257, 513])
def test_quantize_shapes(device, rows, K, bf16):
    x, names = MX.quant_input(rows, K, bf16)
    for ldx in (K, K + 8):
        q, sc = _quantize(device, x, bf16, ldx)
        _check_quantised(q, sc, x, names)
    print(f"\nmx-quantize <{'bf16_t' if bf16 else 'float'}> rows {rows} K {K}: {(rows + 255) // 256} scale group(s), "
          f"grid {(rows + 3) // 4} x {K // 256}", end="")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_quantize_non_finite(device, bf16):
    """include/vcap.h: a NaN is left out of its block's max and stored as an e4m3 NaN; a block holding an
    infinity has scale byte 248 and its finite elements scaled by 2^-121; every other block is untouched and the
    affected bytes are the same on every run.  The byte of the infinity itself is printed and only held to the
    two answers the header leaves open, an e4m3 NaN or 448 (the oracle stores 0x7F / 0xFF)."""
    x = MX.spread(5, 256, 9)
    if bf16:
        x = MX.to_bf16_grid(x)
    y = x.copy()
    y[1, 40], y[2, 70], y[3, 200], y[3, 201] = np.nan, -np.inf, np.inf, np.nan
    q0, sc0 = _quantize(device, x, bf16)
    q1, sc1 = _quantize(device, y, bf16)
    q2, sc2 = _quantize(device, y, bf16)
    assert torch.equal(q1, q2) and torch.equal(sc1, sc2)
    g0, g1 = q0.cpu().numpy()[:5], q1.cpu().numpy()[:5]
    s0, s1 = _unpack(sc0, 5, 256), _unpack(sc1, 5, 256)
    qo, so = O.mx_quantize(y)
    hit = np.zeros((5, 8), bool)
    hit[1, 1], hit[2, 2], hit[3, 6] = True, True, True
    assert np.array_equal(s1[~hit], s0[~hit]) and np.array_equal(g1[~np.repeat(hit, 32, 1)], g0[~np.repeat(hit, 32, 1)])
    assert np.array_equal(s1, so) and s1[1, 1] == s0[1, 1] and s1[2, 2] == 248 and s1[3, 6] == 248
    fin = np.isfinite(y)
    assert np.array_equal(g1[fin], qo[fin])
    assert (g1[1, 40] & 0x7F) == 0x7F and (g1[3, 201] & 0x7F) == 0x7F
    print(f"\nmx-quantize non-finite: -inf -> {g1[2, 70]:#x}, +inf -> {g1[3, 200]:#x} (oracle {qo[2, 70]:#x}, {qo[3, 200]:#x})", end="")
    assert (g1[2, 70] & 0x7F) in (0x7E, 0x7F) and (g1[3, 200] & 0x7F) in (0x7E, 0x7F)


# ---------------------------------------------------------------------------------------------- 2 LayerNorm
def _layernorm_mx(dev, xt, ldx, rows, D, gamma, beta, sc=None, eps=1e-6):
    q = torch.full((rows + 2, D), SENT, dtype=torch.uint8, device=dev)
    if sc is None:
        sc = torch.full((_scale_bytes(rows, D) + 64,), SENT, dtype=torch.uint8, device=dev)
    g = None if gamma is None else torch.from_numpy(gamma).to(dev)
    b = None if beta is None else torch.from_numpy(beta).to(dev)
    N.check(N.lib().vcap_layernorm_mx(xt.data_ptr(), ldx, q.data_ptr(), sc.data_ptr(), g.data_ptr() if gamma is not None else None,
                                      b.data_ptr() if beta is not None else None, rows, D, eps, _s()), "layernorm_mx")
    torch.cuda.synchronize()
    return q, sc


def _check_layernorm(q, sc, x, gamma, beta, tag):
    rows, D = x.shape
    y64, delta = MX.ln_oracle(x, gamma, beta)
    qg = q.cpu().numpy()
    n, bad = MX.check_mx(y64, delta, qg[:rows], _unpack(sc, rows, D))
    print(f"\n{tag}: nv = {D // 256}, {n} / {y64.size} elements decided the other way (cap {MX.cap(y64.size)})", end="")
    assert not bad, (tag, bad)
    assert n <= MX.cap(y64.size), (tag, n)
    assert (qg[rows:] == SENT).all(), tag
    return y64


@pytest.mark.parametrize("rows,D,ld,affine", MX.LN_CASES, ids=[f"r{r}-d{d}-ld{l}-{'affine' if a else 'plain'}"
                                                                for r, d, l, a in MX.LN_CASES])
def test_layernorm_mx(device, rows, D, ld, affine):
    x, gamma, beta = MX.ln_case(rows, D, ld, affine)
    q, sc = _layernorm_mx(device, torch.from_numpy(x).to(device), ld * D, rows, D, gamma, beta)
    _check_layernorm(q, sc, x[:, :D], gamma, beta, f"layernorm-mx r{rows} d{D} ldx {ld * D}")
    assert (sc.cpu().numpy()[_scale_bytes(rows, D):] == SENT).all()
    if rows >= 5:                                         # the constant row: exactly beta, or zero with scale byte 0
        want = np.zeros((1, D), np.float32) if beta is None else beta[None]
        qo, so = O.mx_quantize(want)
        assert np.array_equal(q.cpu().numpy()[1], qo[0]) and np.array_equal(_unpack(sc, rows, D)[1], so[0])


# ---------------------------------------------------------------------------------------------- 3 GEMM
def _operands(dev, family, M, N_, K, seed):
    if family == "rotating":
        a, w = MX.rotating(M, K, seed), MX.rotating(N_, K, seed + 1)
    elif family == "dense":
        a, w = MX.dense(M, K, seed), MX.dense(N_, K, seed + 1)
    else:                                                  # "unit": O(1) pre-activations for the GELU -> MXFP8 epilogue
        a, w = MX.spread(M, K, seed, False), MX.spread(N_, K, seed + 1, False) * np.float32(0.05)
    aq, asc = _quantize(dev, a, fill=0)
    wq, wsc = _quantize(dev, w, fill=0)
    acc, S = MX.gemm_reference(aq.cpu().numpy()[:M], _unpack(asc, M, K), wq.cpu().numpy()[:N_], _unpack(wsc, N_, K))
    return aq, asc, wq, wsc, acc, S


def _gemm_mx(aq, asc, wq, wsc, odt, c, ldc, csc, M, N_, K, bias, act, res):
    N.check(N.lib().vcap_gemm_mx(aq.data_ptr(), asc.data_ptr(), wq.data_ptr(), wsc.data_ptr(), odt, c.data_ptr(), ldc,
                                 None if csc is None else csc.data_ptr(), M, N_, K, None if bias is None else bias.data_ptr(),
                                 act, None if res is None else res.data_ptr(), _s()), "gemm_mx")
    torch.cuda.synchronize()


_GEMM_RUNS = [(f, s) for f in ("rotating", "dense") for s in MX.GEMM_SHAPES]


@pytest.mark.parametrize("family,shape", _GEMM_RUNS, ids=[f"{f}-m{s[0]}-n{s[1]}-k{s[2]}-ldc+{s[3]}" for f, s in _GEMM_RUNS])
def test_gemm_mx_epilogues(device, family, shape):
    """Templates 0..3 of vcap_gemm256_kernel<fp8_t, ...> on one operand pair: no bias, bias, GELU to bf16
    (template 1), residual in place (2) and from a second buffer (3), f32 and bf16 out.  Rows >= M and columns
    [N, ldc) of C keep their sentinel."""
    M, N_, K, pad = shape
    ldc = N_ + pad
    aq, asc, wq, wsc, acc, S = _operands(device, family, M, N_, K, 31 * M + N_)
    g = np.random.default_rng(K + M)
    bias_np = g.standard_normal(N_).astype(np.float32)
    bias = torch.from_numpy(bias_np).to(device)
    res_np = g.standard_normal((M, N_)).astype(np.float32)
    reached = set()
    for name, (out, has_bias, act, res, template) in MX.EPILOGUES.items():
        tdt, odt = (torch.bfloat16, N.DT_BF16) if out == "bf16" else (torch.float32, N.DT_F32)
        c = torch.full((M + 2, ldc), FSENT, dtype=tdt, device=device)
        rbuf = None
        if res == "inplace":
            c[:M, :N_] = torch.from_numpy(res_np).to(device)
            rbuf = c
        elif res == "other":                               # the ABI reads the residual with C's row stride
            rbuf = torch.zeros(M, ldc, dtype=torch.float32, device=device)
            rbuf[:, :N_] = torch.from_numpy(res_np).to(device)
        _gemm_mx(aq, asc, wq, wsc, odt, c, ldc, None, M, N_, K, bias if has_bias else None, act, rbuf)
        want, bound = MX.gemm_expected(acc, S, bias_np if has_bias else None, act, res_np if res else None, out)
        got = c.double().cpu().numpy()
        err = np.abs(got[:M, :N_] - want)
        tag = f"gemm-mx {family} M{M} N{N_} K{K} ldc{ldc} {name}"
        print(f"\n{tag}: template {template}, max err / bound {float((err / bound).max()):.3f}", end="")
        assert template == MX.template_of(out, act, res)
        if (err > bound).any():
            r, col = np.argwhere(err > bound)[0]
            ratio = got[r, col] / want[r, col] if want[r, col] else float("nan")
            pytest.fail(f"{tag}: {(err > bound).sum()} / {err.size} outside the bound; first ({r}, {col}) got {got[r, col]:.9g} "
                        f"want {want[r, col]:.9g} (got / want {ratio:.6g}) bound {bound[r, col]:.3g}")
        assert (got[M:] == FSENT).all() and (got[:M, N_:] == FSENT).all(), tag
        if res == "other":
            assert np.array_equal(rbuf.cpu().numpy()[:, :N_], res_np), tag
        reached.add(template)
    assert reached == {0, 1, 2, 3}


_MX_OUT_RUNS = [(f, s) for f in ("rotating", "unit") for s in MX.GEMM_MX_OUT_SHAPES]


@pytest.mark.parametrize("family,shape", _MX_OUT_RUNS, ids=[f"{f}-m{s[0]}-n{s[1]}-k{s[2]}-ldc+{s[3]}" for f, s in _MX_OUT_RUNS])
def test_gemm_mx_to_mxfp8(device, family, shape):
    """Template 4 (bias + GELU -> MXFP8) at N = 128 / 384 (a 256-column tile half used) and M = 1 / 257: the
    one-step rule and the scale window of mx_cases.check_gemm_mx_out; rows >= M and columns [N, ldc) of C keep
    their sentinel; every scale byte up to vcap_mx_scale_bytes(M, N) is written (the padding rows of the last
    256-row group too, as include/vcap.h says) and none beyond."""
    M, N_, K, pad = shape
    ldc = N_ + pad
    aq, asc, wq, wsc, acc, S = _operands(device, family, M, N_, K, 17 * M + N_)
    bias_np = np.linspace(-0.5, 0.5, N_).astype(np.float32)
    bias = torch.from_numpy(bias_np).to(device)
    c = torch.full((M + 2, ldc), SENT, dtype=torch.uint8, device=device)
    nsc = _scale_bytes(M, N_)
    csc = torch.full((nsc + 64,), 0xFF, dtype=torch.uint8, device=device)
    _gemm_mx(aq, asc, wq, wsc, N.DT_MXFP8, c, ldc, csc, M, N_, K, bias, 1, None)
    g64, bound = MX.gemm_expected(acc, S, bias_np, 1, None, "mx")
    cg, sflat = c.cpu().numpy(), csc.cpu().numpy()
    bad = MX.check_gemm_mx_out(g64, bound, np.ascontiguousarray(cg[:M, :N_]), O.mx_unpack_scales(sflat[:nsc], M, N_))
    print(f"\ngemm-mx {family} M{M} N{N_} K{K} ldc{ldc} gelu->mxfp8: template {MX.template_of('mx', 1, None)}", end="")
    assert not bad, bad
    assert (cg[M:] == SENT).all() and (cg[:M, N_:] == SENT).all()
    assert (sflat[nsc:] == 0xFF).all(), "scale bytes past vcap_mx_scale_bytes written"
    assert (sflat[:nsc] != 0xFF).all(), "a scale byte inside vcap_mx_scale_bytes left unwritten"


# ---------------------------------------------------------------------------------------------- 4 attention
def attention_mx(dev, qkv, frames, n, heads, sc=None):
    M, D = frames * n, heads * 64
    q = torch.full((M + 1, D), SENT, dtype=torch.uint8, device=dev)
    if sc is None:
        sc = torch.full((_scale_bytes(M, D) + 64,), SENT, dtype=torch.uint8, device=dev)
    N.check(N.lib().vcap_vit_attention_mx(qkv.data_ptr(), q.data_ptr(), sc.data_ptr(), frames, n, heads, _s()), "attention_mx")
    torch.cuda.synchronize()
    return q, sc


def check_attention_mx(x, q, sc, tag):
    """x [frames, n, 3, heads, 64] float64 (bf16 values) against the kernel's bytes / scale buffer."""
    frames, n, _, heads, _ = x.shape
    M, D = frames * n, heads * 64
    ref = A.attend(x)
    term = A.tolerance(x, "bf16", ref)
    qg = q.cpu().numpy()
    bad = MX.attention_mx_check(ref.reshape(M, D).numpy(), term, qg[:M], _unpack(sc, M, D))
    print(f"\nattention-mx {tag}: instance {MX.attention_instance(n)}, bf16 term {term:.3e}", end="")
    assert not bad, (tag, bad)
    assert (qg[M:] == SENT).all(), tag


@pytest.mark.parametrize("n", MX.ATTN_TOKENS)
def test_attention_mx_random(device, n):
    frames, heads = 2, 4
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(frames, n, 3, heads, 64, generator=g) * 1.5).bfloat16().double()
    qkv = x.reshape(frames * n, 3 * heads * 64).to(torch.bfloat16).to(device)
    q, sc = attention_mx(device, qkv, frames, n, heads)
    check_attention_mx(x, q, sc, f"random N={n}")
    assert (sc.cpu().numpy()[_scale_bytes(frames * n, heads * 64):] == SENT).all()


# ---------------------------------------------------------------------------------------------- 5 one block
@pytest.mark.parametrize("D,patch,image", [(256, 16, 224), (512, 8, 32)], ids=["d256-n197", "d512-n17"])
def test_one_block_stage_by_stage(device, D, patch, image):
    """LayerNorm -> QKV (bf16) -> attention -> proj (+= residual) -> LayerNorm -> fc1 (GELU -> MXFP8) -> fc2
    (+= residual) through the public entry points, 2 frames, synthetic_vit weights with the sweep's q / k scale.
    Each stage is held to its own rule against the oracle applied to what the GPU actually fed it, so no error
    accumulates; the LayerNorm / attention scale buffer is one buffer reused, as the encode reuses xn_s.  The only
    place these kernels see LayerNorm and GELU distributions (a GELU block sits near -0.17 with many far smaller
    values)."""
    dev, frames = device, 2
    c = ES.Case(0, D, D // 64, patch, image, 1, 1, frames, "one block")
    n, heads = c.tokens, D // 64
    M = frames * n
    sd = weights.synthetic_vit(4242 + D, c.arch, 256)
    b = ES.P + "blocks.0."
    wqkv = sd[b + "attn.qkv.weight"].copy()
    wqkv[:2 * D] *= np.float32(ES.qk_scale(c))
    W = {"qkv": wqkv, "proj": sd[b + "attn.proj.weight"], "fc1": sd[b + "mlp.fc1.weight"], "fc2": sd[b + "mlp.fc2.weight"]}
    Bv = {"qkv": sd[b + "attn.qkv.bias"], "proj": sd[b + "attn.proj.bias"], "fc1": sd[b + "mlp.fc1.bias"], "fc2": sd[b + "mlp.fc2.bias"]}
    Wq = {k: _quantize(dev, np.ascontiguousarray(v, dtype=np.float32), fill=0) for k, v in W.items()}
    Bt = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev) for k, v in Bv.items()}

    def weight_ref(k):
        wq, wsc = Wq[k]
        rows, K = W[k].shape
        return wq.cpu().numpy()[:rows], _unpack(wsc, rows, K)

    def gemm(k, aq, asc, K, odt, cbuf, csc, act, res):
        wq, wsc = Wq[k]
        Nn = W[k].shape[0]
        _gemm_mx(aq, asc, wq, wsc, odt, cbuf, Nn, csc, M, Nn, K, Bt[k], act, res)

    def check_gemm(k, aq_np, as_np, got, act, res_np, out, tag):
        wq_np, ws_np = weight_ref(k)
        acc, S = MX.gemm_reference(aq_np, as_np, wq_np, ws_np)
        want, bound = MX.gemm_expected(acc, S, np.asarray(Bv[k], np.float32), act, res_np, out)
        if out == "mx":
            return want, bound
        err = np.abs(got - want)
        print(f"\nblock d{D} n{n} {tag}: max err / bound {float((err / bound).max()):.3f}", end="")
        assert (err <= bound).all(), (tag, float((err / bound).max()))

    g = np.random.default_rng(D)
    x_np = g.standard_normal((M, D)).astype(np.float32)
    x = torch.from_numpy(x_np).to(dev)
    xn_s = torch.full((_scale_bytes(M, D) + 64,), SENT, dtype=torch.uint8, device=dev)
    # 1 norm1
    xn, _ = _layernorm_mx(dev, x, D, M, D, sd[b + "norm1.weight"], sd[b + "norm1.bias"], sc=xn_s)
    _check_layernorm(xn, xn_s, x_np, sd[b + "norm1.weight"], sd[b + "norm1.bias"], f"block d{D} n{n} norm1")
    xn_np, xs_np = xn.cpu().numpy()[:M], _unpack(xn_s, M, D)
    # 2 QKV -> bf16
    qkv = torch.full((M, 3 * D), FSENT, dtype=torch.bfloat16, device=dev)
    gemm("qkv", xn, xn_s, D, N.DT_BF16, qkv, None, 0, None)
    check_gemm("qkv", xn_np, xs_np, qkv.double().cpu().numpy(), 0, None, "bf16", "qkv")
    # 3 attention -> MXFP8, its scales into the same buffer
    at, _ = attention_mx(dev, qkv, frames, n, heads, sc=xn_s)
    check_attention_mx(qkv.double().cpu().reshape(frames, n, 3, heads, 64), at, xn_s, f"block d{D} N={n}")
    at_np, ats_np = at.cpu().numpy()[:M], _unpack(xn_s, M, D)
    # 4 proj, += into the residual stream
    gemm("proj", at, xn_s, D, N.DT_F32, x, None, 0, x)
    x1_np = x.cpu().numpy()
    check_gemm("proj", at_np, ats_np, x1_np.astype(np.float64), 0, x_np, "f32", "proj")
    # 5 norm2
    xn, _ = _layernorm_mx(dev, x, D, M, D, sd[b + "norm2.weight"], sd[b + "norm2.bias"], sc=xn_s)
    _check_layernorm(xn, xn_s, x1_np, sd[b + "norm2.weight"], sd[b + "norm2.bias"], f"block d{D} n{n} norm2")
    xn_np, xs_np = xn.cpu().numpy()[:M], _unpack(xn_s, M, D)
    # 6 fc1 -> GELU -> MXFP8
    act = torch.full((M, 4 * D), SENT, dtype=torch.uint8, device=dev)
    act_s = torch.full((_scale_bytes(M, 4 * D) + 64,), 0xFF, dtype=torch.uint8, device=dev)
    gemm("fc1", xn, xn_s, D, N.DT_MXFP8, act, act_s, 1, None)
    g64, bound = check_gemm("fc1", xn_np, xs_np, None, 1, None, "mx", "fc1")
    act_np, acts_np = act.cpu().numpy(), _unpack(act_s, M, 4 * D)
    bad = MX.check_gemm_mx_out(g64, bound, act_np, acts_np)
    assert not bad, bad
    assert (act_s.cpu().numpy()[_scale_bytes(M, 4 * D):] == 0xFF).all() and (xn_s.cpu().numpy()[_scale_bytes(M, D):] == SENT).all()
    small = float((np.abs(g64) < 2.0 ** -6 * np.repeat(np.abs(g64).reshape(M, -1, 32).max(-1), 32, 1)).mean())
    print(f"\nblock d{D} n{n} fc1: {small:.1%} of the GELU outputs below 2^-6 of their block max", end="")
    # 7 fc2, += into the residual stream
    gemm("fc2", act, act_s, 4 * D, N.DT_F32, x, None, 0, x)
    check_gemm("fc2", act_np, acts_np, x.double().cpu().numpy(), 0, x1_np, "f32", "fc2")
    assert bool(torch.isfinite(x).all())
