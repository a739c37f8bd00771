"""CPU side of the MXFP8 kernel sweep (tests/mx_cases.py, tests/test_gpu_mx_sweep.py): the oracle is pinned
before it judges a kernel, every "the reference alone stays inside the rule" condition holds, and the
refusals of the MXFP8 entry points come with their documented code and text.

  * torch's CPU float8_e4m3fn cast, which oracle.mx_quantize relies on, equals an exact-rational restatement
    of e4m3fn round-to-nearest-even at every value in [0, 256], every midpoint and both sides of each, both
    signs (962 points, 240 of them exact ties);
  * oracle.mx_quantize equals the exact restatement (scale rule included) on every constructed block, for f32
    and for bf16-valued input, and each block does what its name says;
  * an f32 numpy restatement of vcap_layernorm_mx_kernel's summation order stays inside the LayerNorm
    acceptance rule and the 0.1 % cap on every case (a case that missed would get another seed in
    mx_cases.LN_SEED; none did);
  * the rotating-block GEMM inputs leave one live block per row and every (row % nb, block) pair occurs;
  * vcap_gemm_mx refuses, before any launch, the shapes the sweep's edges sit next to (the refusals of
    vcap_vit_attention_mx - 33, 225, 289 tokens, heads = 3 - are rows of tests/test_cpu_abi_refusals.py)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import mx_cases as MX
from oracle import vcap_oracle as O
from vcap import _native as N


def test_torch_e4m3_cast_is_round_to_nearest_even():
    pts = MX.e4m3_pin_points()
    want = np.array([MX.e4m3_rne(Fraction(float(v)), bool(np.signbit(v))) for v in pts], np.uint8)
    got = MX.torch_e4m3(pts)
    ties = sum(1 for v in pts if any(abs(Fraction(float(v))) * 2 == a + b for a, b in zip(MX.E4M3_POS, MX.E4M3_POS[1:0x79])))
    print(f"\ne4m3 pin: {len(pts)} points, {ties} exact ties, {int((got != want).sum())} mismatches", end="")
    assert ties == 240 and len(pts) == 2 * (0x79 + 3 * 0x78)
    assert np.array_equal(got, want), [(float(p), hex(g), hex(w)) for p, g, w in zip(pts, got, want) if g != w][:5]
    # the format itself: subnormal step 2^-9 below 2^-6, 256 = 0x78, 448 = 0x7E, ties to even on both sides of a binade
    assert MX.E4M3_POS[1] == Fraction(1, 512) and MX.E4M3_POS[8] == Fraction(1, 64)
    assert MX.E4M3_POS[0x78] == 256 and MX.E4M3_POS[0x7E] == 448
    assert MX.e4m3_rne(Fraction(248)) == 0x78 and MX.e4m3_rne(Fraction(232)) == 0x76 and MX.e4m3_rne(Fraction(1, 1024)) == 0


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_oracle_quantiser_equals_the_exact_restatement_on_the_constructed_rows(bf16):
    x, names = MX.special_rows(256, bf16)
    if bf16:
        assert np.array_equal(x, MX.to_bf16_grid(x))
    q, s = O.mx_quantize(x)
    qe, se = MX.mx_quantize_exact(x)
    assert np.array_equal(s, se), MX.first_mismatch(s, se, names, 1)
    assert np.array_equal(q, qe), MX.first_mismatch(q, qe, names, 32)


def _block(name, bf16=False):
    v = dict(MX.special_blocks(bf16))[name]
    q, s = O.mx_quantize(np.tile(v, 8)[None])
    return v, q[0, :32], int(s[0, 0])


def test_constructed_blocks_have_their_property():
    names = [n for n, _ in MX.special_blocks()]
    assert len(names) == len(set(names)) == 40 + 6 + 8
    for k in (-100, -9, 0, 6, 60):                       # every tie pattern in each binade: 120 ties, to even
        seen = []
        for c in range(4):
            v, q, s = _block(f"ties[{30 * c}:{30 * c + 30}] x 2^{k}")
            assert s == 127 + k
            scaled = np.abs(v[1:31].astype(np.float64)) * 2.0 ** -k
            seen += list(scaled)
            assert all((b & 1) == 0 for b in q[1:31]), "a tie goes to the even mantissa"
            vn, qn, sn = _block(f"ties[{30 * c}:{30 * c + 30}] x -2^{k}")
            assert sn == s and np.array_equal(qn ^ 0x80, q)
        assert len(set(seen)) == 120 and max(seen) == 248.0
    assert _block("ties[90:120] x 2^0")[1][30] == 0x78   # 248 -> 256
    for k in (-3, 0, 10):
        v, q, s = _block(f"max=2^{k}")
        assert s == 127 + k - 7 and q[3] == 0x70          # scaled 128
        v, q, s = _block(f"max=2^{k}-ulp")
        assert s == 127 + k - 8 and q[3] == 0xF8          # scaled -255.99.. -> -256
    v, q, s = _block("up-to-256")
    assert s == 127 + 5 and list(q[:5]) == [0x78, 0xF8, 0x77, 0x78, 0xF7]
    assert not _block("zeros")[1].any() and _block("zeros")[2] == 0
    assert (_block("-zeros")[1] == 0x80).all() and _block("-zeros")[2] == 0
    v, q, s = _block("below-2^-120")
    assert s == 0 and q[0] == MX.e4m3_rne(Fraction(96))
    v, q, s = _block("sub-tiny")
    assert s == 0 and list(q[:8]) == [MX.e4m3_rne(Fraction(4)), 3, 2, 0, 0, 1, 0x83, 0x80]
    v, q, s = _block("f32-subnormal")
    assert q[7] == 0 and 0 < v[7] < np.finfo(np.float32).tiny
    v, q, s = _block("FLT_MAX")
    assert s == 247 and q[0] == 0x78
    v, q, s = _block("small")
    assert s == 120 and list(q[:8]) == [0x70, 0x08, 0x01, 0x00, 0x00, 0x01, 0x80, 0x88]


def test_oracle_non_finite_rule():
    """include/vcap.h: a NaN is skipped by the block max; an inf block has scale byte 248."""
    x = MX.spread(2, 256, 3, spread_blocks=False)
    q0, s0 = O.mx_quantize(x)
    y = x.copy()
    y[0, 40], y[1, 70] = np.nan, -np.inf
    q, s = O.mx_quantize(y)
    assert s[0, 1] == s0[0, 1] and s[1, 2] == 248 and (q[0, 40] & 0x7F) == 0x7F
    keep = np.ones_like(x, bool)
    keep[0, 40], keep[1, 64:96] = False, False
    assert np.array_equal(q[keep], q0[keep])
    assert np.array_equal(np.delete(s.ravel(), 8 + 2), np.delete(s0.ravel(), 8 + 2))


@pytest.mark.parametrize("rows,D,ld,affine", MX.LN_CASES, ids=[f"r{r}-d{d}-ld{l}-{'affine' if a else 'plain'}"
                                                                for r, d, l, a in MX.LN_CASES])
def test_f32_layernorm_stays_inside_the_rule(rows, D, ld, affine):
    x, gamma, beta = MX.ln_case(rows, D, ld, affine)
    y64, delta = MX.ln_oracle(x[:, :D], gamma, beta)
    q, s = O.mx_quantize(MX.ln_f32(x[:, :D], gamma, beta))
    n, bad = MX.check_mx(y64, delta, q, s)
    print(f"\nlayernorm-cpu r{rows} d{D}: {n} / {y64.size} elements decided the other way (cap {MX.cap(y64.size)})", end="")
    assert not bad, bad
    assert n <= MX.cap(y64.size)
    if rows >= 5:                                         # the constant row: beta, or zero with scale byte 0
        want = np.zeros(D, np.float32) if beta is None else beta
        assert np.array_equal(MX.ln_f32(x[:, :D], gamma, beta)[1], want)
        assert np.array_equal(y64[1].astype(np.float32), want)
        if not affine:
            assert not s[1].any() and not q[1].any()


def test_check_mx_rejects_what_it_should():
    """The rule is not vacuous: one byte moved two steps, one moved one step away from any boundary, and a
    scale off by one each fail it."""
    x, gamma, beta = MX.ln_case(5, 256, 1, True)
    y64, delta = MX.ln_oracle(x, gamma, beta)
    q, s = O.mx_quantize(y64.astype(np.float32))
    assert MX.check_mx(y64, delta, q, s) == (0, [])
    q2 = q.copy()
    q2[0, 0] += 2
    assert MX.check_mx(y64, delta, q2, s)[1]
    q1 = q.copy()
    q1[3, 7] ^= 1
    assert MX.check_mx(y64, delta, q1, s)[1]
    s1 = s.copy()
    s1[2, 3] += 1
    assert MX.check_mx(y64, delta, MX.quantize_with_scales(y64.astype(np.float32), s1), s1)[1]


@pytest.mark.parametrize("rows,K", [(300, 256), (257, 768), (272, 1280), (16, 512)])
def test_rotating_rows(rows, K):
    x, nb = MX.rotating(rows, K, 1), K // 32
    live = (np.abs(x).reshape(rows, nb, 32).max(-1) > 0)
    assert (live.sum(1) == 1).all()
    r = np.arange(rows)
    assert np.array_equal(live.argmax(1), (r + r // nb) % nb)
    if rows >= nb * nb:
        assert len({(i % nb, b) for i, b in zip(r, live.argmax(1))}) == nb * nb
    q, s = O.mx_quantize(x)
    assert int((s > 0).sum()) == rows and 127 - 12 - 7 - 4 <= s[s > 0].min() and s.max() <= 127 + 12 - 7 + 3


def test_gemm_shape_lists_cover_every_axis_value():
    ms, ns, ks, pads = (set(v) for v in zip(*MX.GEMM_SHAPES))
    assert ms == {1, 16, 255, 257, 300} and ns == {16, 128, 272, 384} and ks == {256, 512, 768, 1280} and pads == {0, 16}
    ms, ns, ks, pads = (set(v) for v in zip(*MX.GEMM_MX_OUT_SHAPES))
    assert {1, 257} <= ms and ns == {128, 384} and pads == {0, 16}
    assert {MX.template_of(o, a, r) for o, _, a, r, _ in MX.EPILOGUES.values()} | {MX.template_of("mx", 1, None)} == {0, 1, 2, 3, 4}
    assert all(MX.template_of(o, a, r) == t for o, _, a, r, t in MX.EPILOGUES.values())
    assert [MX.attention_instance(n) for n in MX.ATTN_TOKENS] == ["<2,2,4>"] * 3 + ["<14,13,8>"] * 2 + ["<14,14,8>"] * 2 + \
        ["<18,17,8>"] * 2 + ["<18,18,8>"] * 2


_BUF = C.create_string_buffer(4096)
P = (C.addressof(_BUF) + 63) & ~63                     # non-null, aligned, never read: every call below is refused
UNSUP = N.E_UNSUPPORTED


def _gemm_mx(out=N.DT_F32, ldc=None, M=32, N_=128, K=256, bias=P, act=0, res=None, csc=None):
    rc = N.lib().vcap_gemm_mx(P, P, P, P, out, P, N_ if ldc is None else ldc, csc, M, N_, K, bias, act, res, None)
    return int(rc), N.lib().vcap_last_error().decode()


# the refusals tests/test_cpu_oracle.py does not pin (it has: misaligned c_scales, MXFP8 out without GELU)
@pytest.mark.parametrize("kw,text", [
    (dict(K=128), "vcap_gemm_mx: K must be a multiple of 256"),
    (dict(N_=24), "vcap_gemm_mx: N and ldc must be multiples of 16"),
    (dict(ldc=136), "vcap_gemm_mx: N and ldc must be multiples of 16"),
    (dict(out=N.DT_MXFP8, N_=64, act=1, csc=P), "vcap_gemm_mx: MXFP8 output needs bias + gelu (act=1), c_scales, N % 128 == 0"),
    (dict(out=N.DT_BF16, res=P), "vcap_gemm_mx: residual needs f32 output"),
], ids=["K128", "N24", "ldc-N+8", "mx-out-N64", "residual-bf16"])
def test_gemm_mx_refusals(kw, text):
    assert _gemm_mx(**kw) == (UNSUP, text)
