"""Shared by test_cpu_mx_cases.py and test_gpu_mx_sweep.py: inputs and oracles of the MXFP8 kernel sweep
(vcap_mx_quantize, vcap_layernorm_mx, vcap_gemm_mx, vcap_vit_attention_mx; DESIGN.md "MXFP8 shapes").

Every tolerance here is zero, or a bound derived below from the arithmetic; none is read off a GPU run.

e4m3 / the quantiser.  e4m3_rne and mx_quantize_exact restate OCP e4m3fn round-to-nearest-even and the block
scale 2^(floor(log2 amax) - 7) (clamped at 2^-127) in exact rationals, written from the format: byte b =
s eeee mmm is (-1)^s m 2^-9 for e = 0 and (-1)^s (8 + m) 2^(e - 10) otherwise.  test_cpu_mx_cases.py holds
torch's CPU float8_e4m3fn cast (what oracle.mx_quantize relies on) to it at every value, midpoint and both
sides of every midpoint up to 256, and oracle.mx_quantize to mx_quantize_exact on the constructed rows.

special_blocks: 32-blocks with one property each, named so that a failure says which:
  ties ...        every midpoint between neighbouring e4m3 values in [0, 256) (120 of them; 248 rounds up to 256),
                  at block scales 2^-100, 2^-9, 1, 2^6 and 2^60, both signs;
  max=2^k         the block max is exactly a power of two (scaled 128); max=2^k-ulp: nextafter(2^k, 0), scaled
                  255.99.. -> 256 under the next smaller scale;
  up-to-256       248 (a tie), 250 and 255 all round up to 256; 247.99 down to 240;
  zeros / -zeros  scale byte 0, bytes 0x00 / 0x80;
  below-2^-120    max 1.5 2^-121: exponent field 6, so the scale byte clamps to 0 and the elements are scaled by
                  2^127; sub-tiny: max 2^-125 with f32-subnormal elements that land on e4m3 subnormals (3 2^-136 ->
                  3 2^-9), on the tie with zero (2^-137) and on zero (2^-149);
  f32-subnormal   one subnormal element in an ordinary block;
  FLT_MAX         scale byte 247, scaled 255.99.. -> 256;
  small           elements 2^-13 .. 2^-18 of a block max of 1.0.  2^-13 of the max is scaled 2^-6, the smallest
                  e4m3 normal, and is kept; 2^-16 is the smallest subnormal 2^-9; 2^-17 is the tie with zero
                  (to even: zero); 2^-18 is the first power of two that rounds to zero outright.
For bf16 input every value is truncated to bf16 first (the ties have <= 5 significant bits and stay ties).

LayerNorm (ln_case / ln_oracle / check_mx).  Oracle: fp64 LayerNorm, cast to f32, mx_quantize.  An f32
LayerNorm cannot decide an element whose fp64 value lies within delta of an e4m3 rounding boundary, nor a scale
when the block max lies within delta of a power of two.  delta is a bound on the f32 arithmetic, per element of
row r: 16 2^-24 (max|x_r| rstd_r |gamma_c| + |beta_c|) - tree sums over <= 1024 elements (10 levels of 2^-24
each on the mean, and on the variance) plus the cancellation in x - mean, which is what max|x| rstd stands
for.  check_mx accepts a difference from the oracle only inside that window and only to the neighbouring e4m3
value on the other side of the boundary, and counts them; the cap is 0.1 % of a case's elements
(tests/test_gpu_mx.py's figure).  ln_f32 restates the kernel's order in f32 numpy (lane partial sums, butterfly
tree); test_cpu_mx_cases.py asserts that it stays inside rule and cap on every case.

GEMM (rotating / dense / gemm_reference / gemm_expected).  Reference: float64 dequant(A) . dequant(W)^T of the
GPU's own quantised operands.  Bound per element, S = sum |a b|:
  f32 out    2e-4 S + 2^-23 |bias|      (tests/test_gpu_mx.py's 2e-4 on the scaled MFMA's internal sum; the bias
                                         add rounds once more, 2^-24 (S + |bias|), the S part inside 2e-4)
  bf16 out   2^-8 S + 2^-8 |bias|       (tests/test_gpu_mx.py's 2^-8: bf16 keeps 8 significant bits, so half an
                                         ulp is at most 2^-8 of the result, and |result| <= S + |bias|)
  residual   + 2^-23 |res|              (one more f32 add)
  GELU       1.13 x the bound on h = acc + bias (|gelu'| <= 1.13), + 2^-20 |h| for the kernel's
             h / (1 + exp2(..)) form (v_exp_f32 and v_rcp_f32 are good to 1 ulp: at most 4 roundings of 2^-23 on
             a result of at most |h|), + the output rounding 2^-8 |gelu(h)| for bf16.
"rotating": row m of A is zero except K-block (m + m // nb) % nb, likewise row n of W, with block scales over
2^+-12: S of an output element is one block's contribution, so the bound binds at every magnitude and a scale
byte taken from the wrong row, K-tile or row group shows as a power-of-two factor.  The + m // nb walks every
(row % nb, block) pair.  "dense": tests/test_gpu_mx.py's _rand.
MXFP8 out: the dequantised output within one top-binade e4m3 step of the quantised exact result (the existing
rule), and the scale byte inside [scale(max(|g| - e)), scale(max(|g| + e))] over the block with e the GELU
bound above: equal to the oracle's unless the accumulator's error can carry the block max across a power of two."""
from __future__ import annotations

import bisect
from fractions import Fraction
from typing import List, Optional, Tuple

import numpy as np
import torch

from oracle import vcap_oracle as O

CAP = 1e-3                                     # share of elements an f32 LayerNorm may decide the other way
FLT_MAX = float(np.finfo(np.float32).max)


# ------------------------------------------------------------------------------------------ e4m3, exactly
def e4m3_value(b: int) -> Fraction:
    """The value of e4m3fn byte b (sign bit clear, b <= 0x7E; 0x7F is NaN)."""
    e, m = (b >> 3) & 15, b & 7
    return Fraction(m, 512) if e == 0 else Fraction(8 + m) * Fraction(2) ** (e - 10)


E4M3_POS = [e4m3_value(b) for b in range(0x7F)]                 # ascending with the byte; [0x78] = 256, [0x7E] = 448


def e4m3_rne(x: Fraction, negative: bool = False) -> int:
    """|x| <= 448 -> the e4m3fn byte nearest to x, ties to the even mantissa (= the even byte)."""
    a = abs(x)
    assert a <= E4M3_POS[-1]
    lo = bisect.bisect_right(E4M3_POS, a) - 1
    b = lo
    if lo < 0x7E:
        d_lo, d_hi = a - E4M3_POS[lo], E4M3_POS[lo + 1] - a
        if d_hi < d_lo or (d_hi == d_lo and lo % 2 == 1):
            b = lo + 1
    return b | (0x80 if (x < 0 or negative) else 0)


def scale_byte_exact(amax: Fraction) -> int:
    """E8M0 byte of the scale 2^(floor(log2 amax) - 7), clamped at 2^-127 (byte 0); amax = 0 gives 0."""
    if amax == 0:
        return 0
    fl = amax.numerator.bit_length() - amax.denominator.bit_length()
    if Fraction(2) ** fl > amax:
        fl -= 1
    return max(fl - 7 + 127, 0)


def mx_quantize_exact(x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """oracle.mx_quantize restated in exact rationals (finite f32 [rows, K])."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, K = x.shape
    q, sb = np.zeros((rows, K), np.uint8), np.zeros((rows, K // 32), np.uint8)
    for r in range(rows):
        for b in range(K // 32):
            blk = x[r, 32 * b:32 * b + 32]
            fr = [Fraction(float(v)) for v in blk]
            s = scale_byte_exact(max(abs(f) for f in fr))
            sb[r, b] = s
            unit = Fraction(2) ** (s - 127)
            q[r, 32 * b:32 * b + 32] = [e4m3_rne(f / unit, bool(np.signbit(v))) for f, v in zip(fr, blk)]
    return q, sb


def e4m3_pin_points() -> np.ndarray:
    """f32: every e4m3 value in [0, 256], every midpoint between neighbours and the f32 on either side of it,
    both signs."""
    vals = [float(v) for v in E4M3_POS[:0x79]]
    mids = np.array([float((E4M3_POS[b] + E4M3_POS[b + 1]) / 2) for b in range(0x78)], np.float32)
    pts = np.concatenate([np.array(vals, np.float32), mids, np.nextafter(mids, np.float32(0)),
                          np.nextafter(mids, np.float32(512))])
    return np.concatenate([pts, -pts])


def torch_e4m3(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


# ------------------------------------------------------------------------------------------ quantiser inputs
def to_bf16_grid(x: np.ndarray) -> np.ndarray:
    """f32 truncated toward zero to a bf16 value (still f32): finite stays finite."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def special_blocks(bf16: bool = False) -> List[Tuple[str, np.ndarray]]:
    g = np.random.default_rng(11)
    ties = np.array([float((E4M3_POS[b] + E4M3_POS[b + 1]) / 2) for b in range(0x78)])
    alt = np.where(np.arange(32) % 2 == 0, 1.0, -1.0)
    out: List[Tuple[str, np.ndarray]] = []
    for k in (-100, -9, 0, 6, 60):
        for c in range(4):
            v = np.concatenate([[192.0], ties[30 * c:30 * c + 30], [1.0]]) * 2.0 ** k * alt
            out += [(f"ties[{30 * c}:{30 * c + 30}] x 2^{k}", v), (f"ties[{30 * c}:{30 * c + 30}] x -2^{k}", -v)]
    for k in (-3, 0, 10):
        v = g.uniform(-0.9, 0.9, 32) * 2.0 ** k
        v[3] = 2.0 ** k
        out.append((f"max=2^{k}", v.copy()))
        v[3] = -float(np.nextafter(np.float32(2.0 ** k), np.float32(0)))
        out.append((f"max=2^{k}-ulp", v.copy()))
    v = g.uniform(-100, 100, 32)
    v[:5] = [248.0, -250.0, 247.99, 255.0, -240.0]
    out.append(("up-to-256", v * 32.0))
    out.append(("zeros", np.zeros(32)))
    out.append(("-zeros", -np.zeros(32)))
    out.append(("below-2^-120", np.concatenate([[1.5], g.uniform(-1.4, 1.4, 31)]) * 2.0 ** -121))
    v = np.zeros(32)
    v[:8] = [2.0 ** -125, 3 * 2.0 ** -136, 5 * 2.0 ** -137, 2.0 ** -149, 2.0 ** -137, 3 * 2.0 ** -138, -3 * 2.0 ** -136,
             -2.0 ** -137]
    out.append(("sub-tiny", v))
    v = g.standard_normal(32)
    v[7] = 2.0 ** -140
    out.append(("f32-subnormal", v))
    v = g.uniform(-0.99, 0.99, 32) * FLT_MAX
    v[0], v[1] = FLT_MAX, -FLT_MAX / 2
    out.append(("FLT_MAX", v))
    v = g.uniform(-0.5, 0.5, 32)
    v[:8] = [1.0, 2.0 ** -13, 2.0 ** -16, 2.0 ** -17, 2.0 ** -18, 3 * 2.0 ** -18, -2.0 ** -17, -2.0 ** -13]
    out.append(("small", v))
    res = []
    for name, v in out:
        v = v.astype(np.float32)
        assert np.isfinite(v).all(), name
        res.append((name, to_bf16_grid(v) if bf16 else v))
    return res


def spread(rows: int, K: int, seed: int, spread_blocks: bool = True) -> np.ndarray:
    """tests/test_gpu_mx.py's _rand: block magnitudes over 2^+-12, one all-zero block, one tiny value."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((rows, K)).astype(np.float32)
    if spread_blocks:
        x *= np.exp2(g.integers(-12, 12, (rows, K // 32, 1))).repeat(32, -1).reshape(rows, K).astype(np.float32)
        x[0, :32] = 0
        x[-1, 5] = 1e-30
    return x


def special_rows(K: int, bf16: bool = False) -> Tuple[np.ndarray, List[List[str]]]:
    """The special blocks packed K / 32 to a row, the last row filled up with random blocks."""
    blocks, nb = special_blocks(bf16), K // 32
    rows = -(-len(blocks) // nb)
    x = spread(rows, K, 5, spread_blocks=False)
    names = [["random"] * nb for _ in range(rows)]
    for i, (name, v) in enumerate(blocks):
        x[i // nb, 32 * (i % nb):32 * (i % nb) + 32] = v
        names[i // nb][i % nb] = name
    return (to_bf16_grid(x) if bf16 else x), names


def quant_input(rows: int, K: int, bf16: bool) -> Tuple[np.ndarray, List[List[str]]]:
    """[rows, K] f32 (on the bf16 grid for bf16): the spread rows, the first rows replaced by special rows."""
    x = spread(rows, K, 1000 * rows + K)
    sx, names = special_rows(K, bf16)
    n = min(rows, len(sx))
    x[:n] = sx[:n]
    names = names[:n] + [["random"] * (K // 32) for _ in range(rows - n)]
    return (to_bf16_grid(x) if bf16 else x), names


def first_mismatch(got: np.ndarray, want: np.ndarray, names, per_block: int) -> str:
    r, c = np.argwhere(got != want)[0]
    return f"row {r} block {c // per_block} ({names[r][c // per_block]}) col {c}: got {got[r, c]:#x}, oracle {want[r, c]:#x}"


# ------------------------------------------------------------------------------------------ LayerNorm
LN_ROWS, LN_DIMS = (1, 5, 257), (256, 512, 768, 1024)
LN_CASES = [(r, d, ld, aff) for d in LN_DIMS for r in LN_ROWS for ld in (1, 3) for aff in (True, False)]
LN_SEED = {}                                                    # (rows, D, ld, affine) -> seed, where 0 misses on the CPU


def ln_case(rows: int, D: int, ld: int, affine: bool, eps: float = 1e-6):
    """-> (x [rows, ld * D] f32 whose first D columns are the rows normalised, gamma, beta | None).  Row 1 is the
    constant 1.5 (rows >= 5): exactly zero variance in f32 too, so the output is beta, or zero with scale byte 0.
    Row 2 (rows = 257) has mean 64 against a spread of 1."""
    g = np.random.default_rng(LN_SEED.get((rows, D, ld, affine), 0) * 7919 + rows * 31 + D + ld)
    x = (g.standard_normal((rows, ld * D)) * 3 + 1).astype(np.float32)
    if rows >= 5:
        x[1, :D] = 1.5
    if rows >= 257:
        x[2, :D] = (64 + g.standard_normal(D)).astype(np.float32)
    gamma = (g.random(D) + 0.5).astype(np.float32) if affine else None
    beta = (g.standard_normal(D) * 0.1).astype(np.float32) if affine else None
    return x, gamma, beta


def ln_oracle(x: np.ndarray, gamma, beta, eps: float = 1e-6):
    """x [rows, D] -> (fp64 LayerNorm [rows, D], delta [rows, D]) (module docstring)."""
    x = x.astype(np.float64)
    mean = x.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(1, keepdims=True) + eps)
    y = (x - mean) * rstd
    ga = np.ones(x.shape[1]) if gamma is None else np.abs(gamma.astype(np.float64))
    be = np.zeros(x.shape[1]) if beta is None else np.abs(beta.astype(np.float64))
    if gamma is not None:
        y = y * gamma.astype(np.float64) + beta.astype(np.float64)
    delta = 16 * 2.0 ** -24 * (np.abs(x).max(1, keepdims=True) * rstd * ga[None] + be[None])
    return y, delta


def _tree(v: np.ndarray) -> np.ndarray:
    """[rows, 64] f32 -> [rows] : the butterfly of wave_sum (pairs, then pairs of pairs, ...)."""
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def ln_f32(x: np.ndarray, gamma, beta, eps: float = 1e-6) -> np.ndarray:
    """vcap_layernorm_mx_kernel's arithmetic in f32 numpy: lane l owns columns 256 i + 4 l .. + 3, sums
    (x0 + x1) + (x2 + x3) over i, the wave sums by a butterfly; two passes; v * rstd, then * gamma + beta as
    separate roundings (the compiler may contract the last two into an fma: inside delta either way)."""
    x = x.astype(np.float32)
    rows, D = x.shape
    nv, f = D // 256, np.float32
    v = x.reshape(rows, nv, 64, 4)
    s = np.zeros((rows, 64), f)
    for i in range(nv):
        s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
    mean = _tree(s) / f(D)
    d = v - mean[:, None, None, None]
    ss = np.zeros((rows, 64), f)
    for i in range(nv):
        e = d[:, i]
        ss = ss + ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + (e[..., 2] * e[..., 2] + e[..., 3] * e[..., 3]))
    rstd = (f(1) / np.sqrt(_tree(ss) / f(D) + f(eps))).astype(f)
    o = (d * rstd[:, None, None, None]).reshape(rows, D)
    if gamma is not None:
        o = o * gamma[None] + beta[None]
    return o.astype(f)


def scale_byte64(v: np.ndarray) -> np.ndarray:
    """mx_scale_byte of float64 magnitudes (0 -> 0)."""
    _, e = np.frexp(np.maximum(v, 0.0))
    return np.where(v > 0, np.clip(e - 1 + 120, 0, 247), 0).astype(np.int64)


def quantize_with_scales(y32: np.ndarray, sb: np.ndarray) -> np.ndarray:
    """e4m3 bytes of y32 under the given scale bytes [rows, K / 32]."""
    rows, K = y32.shape
    inv = ((254 - sb.astype(np.int64)).astype(np.uint32) << 23).view(np.float32)
    return torch_e4m3(y32.reshape(rows, K // 32, 32) * inv[..., None]).reshape(rows, K)


def _code(q: np.ndarray) -> np.ndarray:
    """e4m3 byte -> signed position on the value grid (+-0 both 0): neighbours differ by 1."""
    m = (q & 0x7F).astype(np.int64)
    return np.where(q & 0x80, -m, m)


def check_mx(y64: np.ndarray, delta: np.ndarray, q: np.ndarray, sb: np.ndarray) -> Tuple[int, List[str]]:
    """The acceptance rule of the module docstring.  q [rows, K] bytes and sb [rows, K / 32] unpacked scales of
    the kernel -> (elements that differ from the oracle, violations)."""
    rows, K = y64.shape
    nb = K // 32
    y32 = y64.astype(np.float32)
    qo, so = O.mx_quantize(y32)
    bad: List[str] = []
    a = np.abs(y64).reshape(rows, nb, 32)
    dl = delta.reshape(rows, nb, 32)
    lo, hi = scale_byte64((a - dl).max(-1)), scale_byte64((a + dl).max(-1))
    sg = sb.astype(np.int64)
    for r, b in np.argwhere((sg < lo) | (sg > hi))[:5]:
        bad.append(f"scale row {r} block {b}: got {sg[r, b]}, oracle {so[r, b]}, block max {a[r, b].max():.9g} "
                   f"+- {dl[r, b].max():.3g}")
    qf = quantize_with_scales(y32, sb)
    unit = np.repeat(np.exp2(sg.astype(np.float64) - 127.0), 32, axis=1)
    gv = O.mx_dequantize(q, sb * 0 + 127).astype(np.float64) * unit
    fv = O.mx_dequantize(qf, sb * 0 + 127).astype(np.float64) * unit
    diff = q != qf
    ok = (np.abs(_code(q) - _code(qf)) <= 1) & (np.abs(y64 - (gv + fv) / 2) <= delta)
    for r, c in np.argwhere(diff & ~ok)[:5]:
        bad.append(f"row {r} col {c}: got {q[r, c]:#x} = {gv[r, c]:.9g}, oracle {qf[r, c]:#x} = {fv[r, c]:.9g}, "
                   f"fp64 {y64[r, c]:.9g} +- {delta[r, c]:.3g}")
    n = int(((q != qo) | np.repeat(sb != so, 32, axis=1)).sum())
    return n, bad


def cap(size: int) -> int:
    return int(CAP * size)


# ------------------------------------------------------------------------------------------ GEMM
def rotating(rows: int, K: int, seed: int) -> np.ndarray:
    """Row r is zero except K-block (r + r // nb) % nb, which is randn x 2^randint(-12, 12)."""
    g = np.random.default_rng(seed)
    nb = K // 32
    r = np.arange(rows)
    live = (r + r // nb) % nb
    x = np.zeros((rows, nb, 32), np.float32)
    x[r, live] = (g.standard_normal((rows, 32)) * np.exp2(g.integers(-12, 13, (rows, 1)))).astype(np.float32)
    return x.reshape(rows, K)


def dense(rows: int, K: int, seed: int) -> np.ndarray:
    return spread(rows, K, seed)


def gemm_reference(aq, asb, wq, wsb):
    """e4m3 bytes + unpacked scales of both operands -> (float64 A . W^T, S = |A| . |W|^T)."""
    ad = O.mx_dequantize(aq, asb).astype(np.float64)
    wd = O.mx_dequantize(wq, wsb).astype(np.float64)
    return ad @ wd.T, np.abs(ad) @ np.abs(wd).T


def gelu64(h: np.ndarray) -> np.ndarray:
    return torch.nn.functional.gelu(torch.from_numpy(h), approximate="tanh").numpy()


def gemm_expected(acc: np.ndarray, S: np.ndarray, bias: Optional[np.ndarray], act: int, res: Optional[np.ndarray],
                  out: str) -> Tuple[np.ndarray, np.ndarray]:
    """-> (float64 reference of the epilogue's output before an MXFP8 quantisation, bound) (module docstring).
    out: "f32", "bf16" or "mx" (MXFP8: the bound on the f32 value that is quantised)."""
    b = np.zeros(acc.shape[1]) if bias is None else bias.astype(np.float64)
    h = acc + b[None]
    u = 2.0 ** -8 if out == "bf16" else 2.0 ** -23
    bound = (2.0 ** -8 if out == "bf16" and not act else 2e-4) * S + u * np.abs(b)[None]
    if act:
        g = gelu64(h)
        bound = 1.13 * (2e-4 * S + 2.0 ** -23 * np.abs(b)[None]) + 2.0 ** -20 * np.abs(h)
        if out == "bf16":
            bound = bound + 2.0 ** -8 * np.abs(g) * 1.001
        h = g
    if res is not None:
        h = h + res.astype(np.float64)
        bound = bound + 2.0 ** -23 * np.abs(res)
    return h, bound + 1e-45


def e4m3_step(sb: np.ndarray) -> np.ndarray:
    """One e4m3 step at the top binade of a block (values in [128, 256) x scale): 16 x 2^(scale - 127)."""
    return np.exp2(sb.astype(np.float64) - 127.0) * 16.0


def check_gemm_mx_out(g64: np.ndarray, bound: np.ndarray, q: np.ndarray, sb: np.ndarray) -> List[str]:
    """MXFP8-out rule of the module docstring: g64 the exact GELU output, bound its per-element bound."""
    rows, K = g64.shape
    nb = K // 32
    bad: List[str] = []
    qo, so = O.mx_quantize(g64.astype(np.float32))
    a, e = np.abs(g64).reshape(rows, nb, 32), bound.reshape(rows, nb, 32)
    lo, hi = scale_byte64((a - e).max(-1)), scale_byte64((a + e).max(-1))
    sg = sb.astype(np.int64)
    for r, b in np.argwhere((sg < lo) | (sg > hi))[:5]:
        bad.append(f"scale row {r} block {b}: got {sg[r, b]}, oracle {so[r, b]} (window {lo[r, b]}..{hi[r, b]})")
    got, want = O.mx_dequantize(q, sb).astype(np.float64), O.mx_dequantize(qo, so).astype(np.float64)
    step = np.repeat(e4m3_step(np.maximum(so, sb)), 32, axis=1)
    for r, c in np.argwhere(np.abs(got - want) > step + bound)[:5]:
        bad.append(f"row {r} col {c}: got {got[r, c]:.9g}, oracle {want[r, c]:.9g}, step {step[r, c]:.3g}")
    return bad


# (M, N, K, ldc - N): every axis value of the issue at least once, not a product
GEMM_SHAPES = [(1, 16, 256, 0), (16, 128, 512, 16), (255, 272, 768, 0), (257, 384, 1280, 16), (300, 16, 768, 16),
               (300, 384, 256, 0), (257, 128, 512, 0), (1, 272, 1280, 16)]
# MXFP8 out: N = 128 and 384 (a 256-column tile half used), M = 1 and 257, ldc = N and N + 16
GEMM_MX_OUT_SHAPES = [(1, 128, 256, 0), (257, 384, 768, 16), (257, 128, 1280, 16), (1, 384, 512, 0), (300, 128, 256, 0)]
# name -> (out, bias, act, residual: None | "inplace" | "other"), with the template launch256 picks for it
EPILOGUES = {
    "nobias-f32": ("f32", False, 0, None, 0), "nobias-bf16": ("bf16", False, 0, None, 0),
    "bias-f32": ("f32", True, 0, None, 0), "bias-bf16": ("bf16", True, 0, None, 0),
    "gelu-bf16": ("bf16", True, 1, None, 1), "gelu-nobias-bf16": ("bf16", False, 1, None, 1),
    "res-inplace": ("f32", True, 0, "inplace", 2), "res-other": ("f32", True, 0, "other", 3),
    "gelu-f32": ("f32", True, 1, None, 3),
}


def template_of(out: str, act: int, res) -> int:
    """launch256's choice (csrc/gemm256.hip) restated: which epilogue template of vcap_gemm256_kernel runs.
    A restatement of the dispatcher read from its source, not an observation of the launch: what the tests print
    and collect as "reached" is this function's answer, and would not follow a change of launch256."""
    if out == "mx":
        return 4
    if res is None and act == 0:
        return 0
    if res is None and act == 1 and out == "bf16":
        return 1
    if res == "inplace" and act == 0:
        return 2
    return 3


# ------------------------------------------------------------------------------------------ attention
ATTN_TOKENS = (2, 17, 32, 197, 208, 209, 224, 257, 272, 273, 288)
ATTN_REFUSED = (33, 225, 289)


def attention_instance(n: int) -> str:
    """attn_bf16_dispatch's choice (csrc/vit_attention.hip) restated from its source; like template_of, not
    observed from the launch."""
    kt = 2 * ((n + 31) // 32)
    if kt == 2:
        return "<2,2,4>"
    ke = kt - 1 if n <= (kt - 1) * 16 else kt
    return f"<{kt},{ke},8>"


def attention_mx_check(ref: np.ndarray, term: float, q: np.ndarray, sb: np.ndarray) -> List[str]:
    """ref [rows, D] fp64 attention output, term the bf16 tolerance of the input (attention_edge_cases.tolerance:
    3 x max |bf16 emulation - fp64|, two CPU forwards), q / sb the kernel's bytes and unpacked scales.
    Scale: inside [scale(max - term), scale(max + term)], so within 1 of the reference's and equal wherever the
    reference block max is further than term from a power of two.  Element: within half a top-binade e4m3 step
    of its block (8 x 2^(scale - 127) <= 1 / 16 of the block max) + term, the scale being the reference's - or
    the kernel's where that is the larger of the two, which the scale check has then allowed."""
    rows, D = ref.shape
    a = np.abs(ref).reshape(rows, D // 32, 32).max(-1)
    so = scale_byte64(a)
    lo, hi = scale_byte64(a - term), scale_byte64(a + term)
    sg = sb.astype(np.int64)
    bad: List[str] = []
    for r, b in np.argwhere((sg < lo) | (sg > hi) | (np.abs(sg - so) > 1))[:5]:
        bad.append(f"scale row {r} block {b}: got {sg[r, b]}, reference {so[r, b]}, block max {a[r, b]:.6g} +- {term:.3g}")
    got = O.mx_dequantize(q, sb).astype(np.float64)
    half = np.repeat(e4m3_step(np.maximum(so, sg)) / 2, 32, axis=1)
    for r, c in np.argwhere(np.abs(got - ref) > half + term)[:5]:
        bad.append(f"row {r} col {c}: got {got[r, c]:.6g}, reference {ref[r, c]:.6g}, half step {half[r, c]:.3g} + {term:.3g}")
    return bad


def attention_mx_bound(ref: np.ndarray, term: float) -> np.ndarray:
    """Per-element bound of attention_mx_check with the reference's own scales."""
    rows, D = ref.shape
    so = scale_byte64(np.abs(ref).reshape(rows, D // 32, 32).max(-1))
    return np.repeat(e4m3_step(so) / 2, 32, axis=1) + term
