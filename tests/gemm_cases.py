"""Shared by test_cpu_gemm_cases.py and test_gpu_gemm_sweep.py: inputs, oracle, bounds and the restated
dispatchers of the dense GEMM sweep (vcap_gemm, vcap_gemm_splitk, vcap_linear_bias: the bf16 / f16 / f32
instances of csrc/gemm.hip's 128x128 kernel and csrc/gemm256.hip's 256x256 kernel; DESIGN.md "Dense GEMM shapes").

No bound here comes from a GPU run, and no case excludes an element.

Exact operands (kind "exact").  A and W hold small integers, bias and residual multiples of 1/4, drawn so that
K max|a| max|w| + max|bias| + max|res| < 2^22 (2^15 for f16 operands: nothing reaches the fp16 overflow).  Every
operand is then exact in bf16, f16 and f32, and every product and every partial sum - in any order, in any MFMA
shape, in any split - is an integer below 2^24: the f32 accumulator IS the integer result, acc + bias and the
residual add are exact too, and the only roundings left are the ones the kernels make on purpose.  Rows 0, 3, 6 ..
of A and rows 0, 2, 4 .. of W are non-negative, so a sixth of the outputs is large (about K max|a| max|w| / 4):
with quarter-step biases those are inexact in 16 bits, ties included, which is what exercises the rounding points.
The oracle is float64 (exact: everything stays below 2^53; test_cpu_gemm_cases.py holds it to int64), rounded
exactly where Autocast<T> (csrc/vcap_common.h) and the two epilogues round:
  h = acc + bias;  f16 operands: h = rne_f16(h)  (the Linear's fp16 output; a 16-bit store rounds by itself and
  rounding is idempotent; split-K: after the slab sum + bias, in the reduce kernel)
  GELU: g = gelu_tanh(h); f16 operands with f32 out: g = rne_f16(g)
  res_mode 1: + res[orow(m)]     res_mode 2: + res[(m % G) + roff]      orow(m) = G ? (m / G) Gs + goff + m % G : m
  bf16 / f16 out: round-to-nearest-even of the result.
Tolerance: zero, outputs compared as bit patterns over the whole C buffer (sentinel rows and columns included).
A GELU is the one thing not exact: on exact operands h is exact, so mx_cases' GELU rule leaves 2^-20 |h| (the
kernel's h / (1 + exp2(..)) form: v_exp_f32 and v_rcp_f32 good to 1 ulp, at most 4 roundings of 2^-23 on a
result of at most |h|) plus the output rounding.

Dense operands (kind "dense"): tests/test_gpu_ops.py's _rand scales (A ~ N(0, 1), W ~ 0.05 N(0, 1), bias ~ 0.1
N(0, 1), residual ~ N(0, 1)), rounded to the operand type; reference float64 over the operands as stored.  Bound
per element, S = sum |a w|:
  f32 out    K 2^-23 S + 2^-23 (|bias| + |res|)     K 2^-23 is twice the first-order error K 2^-24 S of a K-term
             f32 sum in any order (each of at most K additions rounds a partial sum of magnitude <= S by 2^-24);
             the products themselves are exact for 16-bit operands and within the same term for f32
  16-bit out + 2^-8 (|result| + e) (bf16: 8 significant bits) or 2^-11 (|result| + e) (f16: 11): half an ulp of the
             kernel's own value, which lies within e - the bound so far - of the reference
  f16 operands: + 2^-11 |h| at the Linear's rounding, + 2^-11 |g| at the GELU's when the output is f32
  (+ 2^-25 absolute at every f16 rounding: half the fp16 subnormal step 2^-24, which 2^-11 |x| does not cover
  below 2^-14 - a GELU's output gets there)
  GELU       1.13 x the bound on h (|gelu'| <= 1.13) + 2^-20 |h| + the output rounding.
A residual added to a GELU's output, on exact operands too: + 2^-23 |res| (the f32 add of an inexact value rounds).
Where a bound applies, the reference is the unrounded float64 value and every rounding is in the bound; a value
that is exact is rounded in the oracle itself, where the kernel rounds it.

template_of restates launch_gemm / gemm_splits / vcap_gemm_dispatch (csrc/gemm.hip) and launch256 / launch256_epi /
vcap_gemm256_ok (csrc/gemm256.hip) from their source: which kernel, which EPI template, which store branch, how
many splits.  It is a restatement, not an observation of the launch: a change of a dispatcher has to be carried
into it (test_cpu_gemm_cases.py keeps the case list from thinning below one case per template).

FAULTS: kernel mistakes injected into the oracle's own arithmetic; test_cpu_gemm_cases.py asserts that for each
one some exact case's bits change, i.e. that the GPU comparison would catch the same mistake in a kernel."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

SENT = -776.0                                  # exact in bf16, f16 and f32
PAD_ROWS = 3
PAIRS = (("bf16", "bf16"), ("bf16", "f32"), ("f16", "f16"), ("f16", "f32"), ("f32", "f32"))
SIZE = {"bf16": 2, "f16": 2, "f32": 4}
TORCH = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}   # half an ulp relative to the value
KRESMAXLD = 1 << 24


def ktile(in_t: str) -> int:
    """Elements of one 128-byte K-tile row."""
    return 128 // SIZE[in_t]


@dataclass(frozen=True)
class Case:
    name: str
    policy: int                 # vcap_set_gemm_policy of the GPU run
    M: int
    N: int
    kt: int                     # K-tiles: K = kt * ktile(operand type)
    bias: bool = True
    act: int = 0
    res: Optional[str] = None   # None | "inplace" (res == C) | "other"
    res_mode: int = 0
    G: int = 0
    Gs: int = 0
    goff: int = 0
    roff: int = 0
    lda_pad: int = 0            # lda = K + lda_pad ...
    ldw_pad: int = 0
    ldc_pad: int = 8            # ldc = N + ldc_pad: 8 sentinel columns unless a case says otherwise (a multiple of 8
                                # keeps the 128x128 vector store and the 256x256 16-byte store where N allows them)
    ldr_pad: Optional[int] = None   # ldr = N + ldr_pad; None: ldc ("inplace") or N + 4 ("other": NaN pad columns)
    c_off: int = 0              # bytes C starts into its allocation
    bias_off: int = 0           # floats the bias / residual start into theirs
    res_off: int = 0
    kind: str = "exact"
    only16: bool = False        # 16-bit outputs only (the case is about their store branch)
    splitk: bool = False        # through vcap_gemm_splitk (in-place residual, workspace)
    fallback: Optional[str] = None   # why vcap_gemm256_ok turns the shape down (policy 2 cases)

    def K(self, in_t: str) -> int:
        return self.kt * ktile(in_t)

    def lda(self, in_t):
        return self.K(in_t) + self.lda_pad

    def ldw(self, in_t):
        return self.K(in_t) + self.ldw_pad

    @property
    def ldc(self):
        return self.N + self.ldc_pad

    @property
    def ldr(self):
        if self.res is None:
            return 0
        if self.ldr_pad is not None:
            return self.N + self.ldr_pad
        return self.ldc if self.res == "inplace" else self.N + 4

    @property
    def rows_out(self):
        if not self.G:
            return self.M
        assert self.goff + self.G <= self.Gs
        return -(-self.M // self.G) * self.Gs

    def pairs(self) -> Tuple[Tuple[str, str], ...]:
        ps = PAIRS
        if self.res_mode:
            ps = tuple(p for p in ps if p[1] == "f32")
        if self.only16:
            ps = tuple(p for p in ps if p[1] != "f32")
        if self.splitk:
            ps = (("bf16", "f32"), ("f16", "f32"))
        return ps


def orow(c: Case, m: np.ndarray) -> np.ndarray:
    return (m // c.G) * c.Gs + c.goff + m % c.G if c.G else m


# ------------------------------------------------------------------------------------------ rounding, exactly
def rne(x: np.ndarray, fmt: str) -> np.ndarray:
    """float64 -> the nearest bf16 / f16 value (float64), ties to even, subnormals kept: written from the formats
    (bf16: 8 significant bits, smallest normal 2^-126; f16: 11 bits, 2^-14).  No overflow handling: asserted."""
    if fmt == "f32":
        return x.astype(np.float32).astype(np.float64)
    bits, emin = (8, -126) if fmt == "bf16" else (11, -14)
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)                                   # |x| = m 2^e, 0.5 <= m < 1
    q = np.ldexp(1.0, np.maximum(e, emin + 1) - bits)    # the spacing of the format at x
    r = np.rint(x / q) * q                               # np.rint rounds half to even; x / q is exact
    assert np.all(np.abs(r) < (65520.0 if fmt == "f16" else 3.4e38))
    return r


def trunc16(x: np.ndarray, fmt: str) -> np.ndarray:
    """(fault) toward zero instead of to nearest."""
    bits, emin = (8, -126) if fmt == "bf16" else (11, -14)
    _, e = np.frexp(x)
    q = np.ldexp(1.0, np.maximum(e, emin + 1) - bits)
    return np.trunc(x / q) * q


def gelu64(h: np.ndarray) -> np.ndarray:
    return torch.nn.functional.gelu(torch.from_numpy(np.ascontiguousarray(h, np.float64)), approximate="tanh").numpy()


# ------------------------------------------------------------------------------------------ operands
def _ranges(K: int, f16: bool) -> Tuple[int, int]:
    limit = (1 << 15) if f16 else (1 << 22)
    for amax, wmax in ((8, 4), (4, 4), (4, 2), (2, 2), (2, 1), (1, 1)):
        if K * amax * wmax + BIAS_MAX + RES_MAX < limit:
            return amax, wmax
    raise AssertionError("K too long for exact operands")


BIAS_MAX, RES_MAX = 8.0, 64.0


def res_rows(c: Case) -> int:
    if c.res_mode == 2:
        return c.G + c.roff
    return c.rows_out


def operands(c: Case, pair: Tuple[str, str]) -> Dict[str, np.ndarray]:
    """-> a [M, K], w [N, K], bias [N] | None, res [res_rows, N] | None, all float64 and exact in the operand type
    (a, w) / in f32 (bias, res)."""
    in_t = pair[0]
    K = c.K(in_t)
    g = np.random.default_rng(zlib.crc32(f"{c.name}/{in_t}".encode()))
    if c.kind == "exact":
        amax, wmax = _ranges(K, in_t == "f16")
        a = g.integers(-amax, amax + 1, (c.M, K)).astype(np.float64)
        w = g.integers(-wmax, wmax + 1, (c.N, K)).astype(np.float64)
        a[0::3] = np.abs(a[0::3])
        w[0::2] = np.abs(w[0::2])
        bias = g.integers(-4 * BIAS_MAX, 4 * BIAS_MAX + 1, c.N) / 4.0
        res = g.integers(-4 * RES_MAX, 4 * RES_MAX + 1, (res_rows(c), c.N)) / 4.0
        assert K * np.abs(a).max() * np.abs(w).max() + BIAS_MAX + RES_MAX < ((1 << 15) if in_t == "f16" else (1 << 22))
    else:
        t = TORCH[in_t]
        a = torch.from_numpy(g.standard_normal((c.M, K)).astype(np.float32)).to(t).double().numpy()
        w = torch.from_numpy((g.standard_normal((c.N, K)) * 0.05).astype(np.float32)).to(t).double().numpy()
        bias = (g.standard_normal(c.N) * 0.1).astype(np.float32).astype(np.float64)
        res = g.standard_normal((res_rows(c), c.N)).astype(np.float32).astype(np.float64)
    return {"a": a, "w": w, "bias": bias if c.bias else None, "res": res if c.res else None}


# ------------------------------------------------------------------------------------------ the restated dispatchers
def ok256(c: Case, pair, bias_aligned=True, res_aligned=True) -> Optional[str]:
    """vcap_gemm256_ok restated: None if the 256x256 kernel takes the shape, else the reason it does not."""
    in_t = pair[0]
    bk, ein = ktile(in_t), 16 // SIZE[in_t]
    if c.K(in_t) % (2 * bk):
        return "K is an odd number of K-tiles"
    if c.N % 16:
        return "N % 16"
    if c.lda(in_t) % ein or c.ldw(in_t) % ein:
        return "lda / ldw not whole 16-byte vectors"
    if c.ldc % 4:
        return "ldc % 4"
    if c.bias and (c.bias_off % 4 or not bias_aligned):
        return "bias not 16-byte aligned"
    if c.res and (c.res_off % 4 or not res_aligned):
        return "residual not 16-byte aligned"
    if c.res and c.ldr % 4:
        return "ldr % 4"
    if offsets_overflow(c.M, c.lda(in_t), c.N, c.ldw(in_t), c.K(in_t), SIZE[in_t]):
        return "operand byte offsets past 2^32"
    return None


def offsets_overflow(M, lda, N, ldw, K, esize) -> bool:
    """The 256x256 kernel keeps a lane's operand byte offset ((row * ld + chunk) * sizeof(T), rows clamped to the
    last) in 32 bits; the K-tile advance is on the 64-bit base."""
    return max((M - 1) * lda, (N - 1) * ldw) * esize + 128 > (1 << 32)


def gemm_splits(nkt: int) -> int:
    """gemm_splits' rule: the largest c <= 8 dividing the K-tile count that leaves >= 3 K-tiles per split."""
    for d in range(8, 1, -1):
        if nkt % d == 0 and nkt // d >= 3:
            return d
    return 1


def colgroup(N: int, K: int, esize: int) -> int:
    """launch256_epi's column-group width of the GELU template (0: row-major order)."""
    tiles_n = -(-N // 256)
    tile_bytes = 256 * K * esize
    w = 0
    for cc in range(tiles_n - 1, 0, -1):
        if tiles_n % cc == 0 and cc * tile_bytes <= 2560 * 1024:
            w = cc
            break
    return w if 0 < w < tiles_n else 0


def _epi(c: Case, pair, k256: bool) -> int:
    in_t, out_t = pair
    plain = c.G == 0
    if plain and c.res_mode == 0 and c.act == 0:
        return 0
    if plain and c.res_mode == 0 and c.act == 1 and (SIZE[in_t] == SIZE[out_t] or (k256 and SIZE[out_t] == 2)):
        return 1
    if (out_t == "f32" and plain and c.res_mode == 1 and c.act == 0 and c.res == "inplace" and c.ldr == c.ldc and
            (not k256 or c.ldr < KRESMAXLD)):
        return 2
    return 3


def _t128(c: Case, pair, M: int, splits: int = 1) -> dict:
    vec = c.N % 4 == 0 and c.ldc % 4 == 0 and (not c.res or c.ldr % 4 == 0)
    return {"kernel": "128", "epi": _epi(c, pair, False), "store": "vec" if vec else "scalar", "splits": splits,
            "colgroup": 0, "prefetch": False, "rows": (0, M)}


def _t256(c: Case, pair, M: int) -> dict:
    in_t, out_t = pair
    epi = _epi(c, pair, True)
    b16 = (SIZE[out_t] == 2 and epi in (0, 1) and c.N % 32 == 0 and c.ldc % 8 == 0 and c.c_off % 16 == 0)
    pf = epi == 2 and SIZE[in_t] == 2 and M >= 256 and c.N >= 256      # some tile lies wholly inside
    return {"kernel": "256", "epi": epi, "store": "16B" if b16 else "8B" if SIZE[out_t] == 2 else "f32x4", "splits": 1,
            "colgroup": colgroup(c.N, c.K(in_t), SIZE[in_t]) if epi == 1 else 0, "prefetch": pf, "rows": (0, M)}


def template_of(c: Case, pair, policy: Optional[int] = None, cus: int = 256) -> List[dict]:
    """vcap_gemm_dispatch restated -> the launches of the case, in order (two for the auto policy's row split)."""
    in_t, out_t = pair
    policy = c.policy if policy is None else policy
    if c.splitk:
        s = gemm_splits(c.kt) if c.N % 4 == 0 and c.ldc % 4 == 0 else 1
        if s > 1:
            return [_t128(c, pair, c.M, s)]
    if policy != 1 and ok256(c, pair) is None:
        if policy == 2:
            return [_t256(c, pair, c.M)]
        tn = -(-c.N // 256)
        tiles = -(-c.M // 256) * tn
        if tiles >= cus:
            rounds = tiles // cus
            rem = tiles - rounds * cus
            plain = c.G == 0 and (c.res_mode == 0 or c.res == "inplace")
            m_full = (rounds * cus // tn) * 256
            if plain and 0 < rem and rem * 4 < cus and 0 < m_full < c.M:
                lo, hi = _t256(c, pair, m_full), _t128(c, pair, c.M - m_full)
                hi["rows"] = (m_full, c.M)
                return [lo, hi]
            return [_t256(c, pair, c.M)]
    return [_t128(c, pair, c.M)]


def describe(ts: List[dict]) -> str:
    return " + ".join(f"{t['kernel']}x{t['kernel']} EPI {t['epi']} {t['store']} rows [{t['rows'][0]}, {t['rows'][1]})"
                      + (f" splits {t['splits']}" if t["splits"] > 1 else "")
                      + (f" colgroup {t['colgroup']}" if t["colgroup"] else "") + (" prefetch" if t["prefetch"] else "")
                      for t in ts)


# ------------------------------------------------------------------------------------------ the oracle
FAULTS = ("last K-tile dropped", "one K-tile summed twice", "bias from the clamped column N - 4 in an edge tile",
          "residual row clamped to M - 1 on a stored row", "goff dropped", "roff dropped",
          "fp16 rounding after the residual add", "fp16 rounding per split-K slab", "16-bit store truncates",
          "colgroup order with the row-major tile count")


def _covered(c: Case, t: dict, fault: Optional[str]) -> np.ndarray:
    """[tiles_m, tiles_n] bool: the tiles some workgroup computes (all of them, unless the fault drops some)."""
    tile = int(t["kernel"])
    tm, tn = -(-c.M // tile), -(-c.N // tile)
    cov = np.ones((tm, tn), bool)
    if fault == FAULTS[9] and t["colgroup"]:
        cov[:] = False
        w = t["colgroup"]
        per = w * tn                                   # the fault: w * tiles_m is right
        for wg in range(tm * tn):
            g_, rem = divmod(wg, per)
            mt, nt = rem // w, g_ * w + rem % w
            if mt < tm and nt < tn:
                cov[mt, nt] = True
    return cov


def oracle(c: Case, pair, d: Dict[str, np.ndarray], fault: Optional[str] = None,
           ts: Optional[List[dict]] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (c_init, expected, bound), each float64 [rows_out + PAD_ROWS, ldc]: the C buffer before the call (the
    sentinel; the residual in its live region for an in-place case), after it, and the per-element bound (zero
    wherever the comparison is bit for bit)."""
    in_t, out_t = pair
    ts = ts or template_of(c, pair)
    t0 = ts[0]
    K, bk = c.K(in_t), ktile(in_t)
    a, w = d["a"], d["w"]
    if fault == FAULTS[0]:
        acc = a[:, :K - bk] @ w[:, :K - bk].T
    elif fault == FAULTS[1]:
        acc = a @ w.T + a[:, :bk] @ w[:, :bk].T
    else:
        acc = a @ w.T
    S = np.abs(a) @ np.abs(w).T
    exact = c.kind == "exact"
    f16 = in_t == "f16"
    bias = np.zeros(c.N) if d["bias"] is None else d["bias"]
    tile = int(t0["kernel"])
    bmat = np.broadcast_to(bias, (c.M, c.N)).copy()
    if fault == FAULTS[2] and c.N % tile and c.N >= 4:
        n0 = c.N - c.N % tile
        bmat[:, n0:] = np.resize(bias[c.N - 4:], c.N - n0)
    h = acc + bmat
    err = np.zeros_like(h) if exact else K * 2.0 ** -23 * S + 2.0 ** -23 * np.abs(bmat)
    slab_fault = fault == FAULTS[7] and f16 and t0["splits"] > 1
    if slab_fault:
        ks = K // t0["splits"]
        h = sum(rne(a[:, i * ks:(i + 1) * ks] @ w[:, i * ks:(i + 1) * ks].T, "f16") for i in range(t0["splits"])) + bmat
    late = fault == FAULTS[6] and f16 and c.res_mode
    # An exact value is rounded where the kernel rounds it (the kernel's input to that rounding is the same number).
    # A value that carries an error is left unrounded - the reference stays the float64 result - and the rounding
    # goes into the bound: half an ulp of the kernel's own value, which is within err of the reference.
    inexact = not exact
    if f16 and not late and not slab_fault:
        if inexact:
            err = err + U16["f16"] * (np.abs(h) + err) + 2.0 ** -25
        else:
            h = rne(h, "f16")
    v = h
    if c.act:
        v = gelu64(h)
        err = 1.13 * err + 2.0 ** -20 * np.abs(h)
        inexact = True
        if f16 and out_t == "f32":
            err = err + U16["f16"] * (np.abs(v) + err) + 2.0 ** -25
    m = np.arange(c.M)
    rows = orow(replace(c, goff=0) if fault == FAULTS[4] else c, m)
    if c.res_mode:
        if c.res_mode == 1:
            rr = rows.copy()
            if fault == FAULTS[3] and c.M % tile:
                rr[c.M - c.M % tile:] = rows[c.M - 1]
        else:
            rr = m % c.G + (0 if fault == FAULTS[5] else c.roff)
        v = v + d["res"][rr]
        if inexact:
            err = err + 2.0 ** -23 * np.abs(d["res"][rr])      # the f32 add rounds once more
        if late:
            v = rne(v, "f16")
    if out_t != "f32":
        if inexact:
            err = err + U16[out_t] * (np.abs(v) + err) + (2.0 ** -25 if out_t == "f16" else 0.0)
        else:
            v = trunc16(v, out_t) if fault == FAULTS[8] else rne(v, out_t)
    elif not inexact:
        assert np.array_equal(v, rne(v, "f32"))          # exact operands: the f32 result is exact
    if not inexact:
        err = np.zeros_like(v)
    ldc, R = c.ldc, c.rows_out + PAD_ROWS
    c_init = np.full((R, ldc), SENT)
    if c.res == "inplace":
        c_init[:c.rows_out, :c.N] = d["res"] if c.res_mode == 1 else SENT
    exp, bound = c_init.copy(), np.zeros((R, ldc))
    cov = np.ones((c.M, c.N), bool)
    for t in ts:
        tl = int(t["kernel"])
        cv = np.kron(_covered(replace(c, M=t["rows"][1] - t["rows"][0]), t, fault), np.ones((tl, tl), bool))
        cov[t["rows"][0]:t["rows"][1]] = cv[:t["rows"][1] - t["rows"][0], :c.N]
    rsel, csel = np.nonzero(cov)
    exp[rows[rsel], csel] = v[rsel, csel]
    bound[rows[rsel], csel] = err[rsel, csel]
    return c_init, exp, bound


def bits(x: np.ndarray, out_t: str) -> np.ndarray:
    """float64 values already on the out_t grid -> their bit patterns."""
    t = torch.from_numpy(np.ascontiguousarray(x, np.float64)).to(TORCH[out_t])
    return t.view(torch.int32 if out_t == "f32" else torch.int16).numpy()


# ------------------------------------------------------------------------------------------ the cases
REMAPS = ((196, 197, 1, 1), (7, 9, 2, 0), (5, 5, 0, 3))         # (G, Gs, goff, roff); 3 groups each


def _cases() -> List[Case]:
    cs: List[Case] = []
    add = lambda name, policy, M, N, kt, **kw: cs.append(Case(f"p{policy}-{name}", policy, M, N, kt, **kw))
    inplace, other = dict(res="inplace", res_mode=1), dict(res="other", res_mode=1)
    # ---- 128x128 kernel
    for M, N, kt in ((1, 4, 1), (127, 8, 2), (128, 124, 3), (129, 128, 6), (257, 132, 1), (129, 200, 2),
                     (1, 5, 3), (257, 130, 2), (127, 203, 6)):
        add(f"bias-{M}x{N}x{kt}", 1, M, N, kt)
    add("bias-ldc+1", 1, 129, 132, 2, ldc_pad=1)
    add("bias-grid3x3", 1, 257, 384, 1)
    add("bias-strides", 1, 129, 132, 2, lda_pad=64, ldw_pad=128)
    add("nobias", 1, 129, 132, 2, bias=False)
    add("nobias-scalar", 1, 127, 130, 1, bias=False)
    add("gelu", 1, 129, 132, 2, act=1)
    add("gelu-scalar", 1, 127, 203, 1, act=1)
    add("gelu-nobias", 1, 1, 8, 3, act=1, bias=False)
    add("inplace-edges", 1, 257, 132, 2, **inplace)             # a partial row tile and a partial column tile
    add("inplace-whole", 1, 128, 128, 1, **inplace)
    add("inplace-nobias", 1, 129, 200, 3, bias=False, **inplace)
    add("inplace-scalar", 1, 129, 130, 2, **inplace)
    add("inplace-ldc+4", 1, 127, 124, 6, ldc_pad=4, **inplace)
    add("res-other", 1, 129, 132, 2, **other)
    add("res-other-ldr+1", 1, 129, 132, 2, ldr_pad=1, **other)  # ldr % 4 != 0: scalar store
    add("res-inplace-ldr!=ldc", 1, 1, 132, 2, ldr_pad=16, **inplace)
    add("res-gelu", 1, 129, 132, 2, act=1, **other)
    for i, (G, Gs, goff, roff) in enumerate(REMAPS):
        N = (132, 8, 130)[i]
        add(f"res2-G{G}", 1, 3 * G, N, (1, 2, 3)[i], res="other", res_mode=2, G=G, Gs=Gs, goff=goff, roff=roff)
    add("remap-res1", 1, 21, 132, 2, G=7, Gs=9, goff=2, **other)
    add("remap-res1-inplace", 1, 21, 128, 2, G=7, Gs=9, goff=2, **inplace)
    add("remap-nores", 1, 15, 132, 2, G=5, Gs=6, goff=1)
    add("remap-nores-scalar", 1, 130, 5, 1, G=5, Gs=6, goff=1)
    # ldc == N (no sentinel columns: a row's overrun lands in the next row), held by a few cases per kernel
    add("bias-ldc=N", 1, 257, 132, 2, ldc_pad=0)
    add("bias-scalar-ldc=N", 1, 127, 203, 1, ldc_pad=0)
    add("inplace-ldc=N", 1, 257, 132, 2, ldc_pad=0, **inplace)
    add("res2-ldc=N", 1, 21, 132, 1, ldc_pad=0, res="other", res_mode=2, G=7, Gs=9, goff=2, roff=0)
    # ---- 256x256 kernel
    for M, N, kt in ((1, 16, 2), (255, 32, 4), (256, 48, 6), (257, 240, 2), (300, 256, 2), (255, 272, 4),
                     (300, 528, 2)):
        add(f"bias-{M}x{N}x{kt}", 2, M, N, kt)
    add("bias-ldc+4", 2, 257, 64, 2, ldc_pad=4, only16=True)    # the 16-byte store branch, each condition defeated
    add("bias-257x64", 2, 257, 64, 2)
    add("bias-c+8B", 2, 257, 32, 2, c_off=8, only16=True)
    add("bias-strides", 2, 257, 272, 2, lda_pad=64, ldw_pad=128)
    add("nobias", 2, 257, 272, 2, bias=False)
    add("nobias-48", 2, 300, 48, 4, bias=False)
    for N in (512, 768, 1024):
        add(f"gelu-fc1-{N}", 2, 300, N, 2, act=1)
    add("gelu", 2, 257, 272, 4, act=1)
    add("gelu-nobias-48", 2, 255, 48, 2, act=1, bias=False)
    add("inplace-512", 2, 512, 512, 2, **inplace)               # four whole tiles: every piece prefetches
    add("inplace-256", 2, 256, 256, 2, **inplace)
    add("inplace-rows", 2, 300, 768, 12, **inplace)
    add("inplace-cols", 2, 511, 272, 4, **inplace)
    add("inplace-longK", 2, 512, 256, 48, **inplace)
    add("inplace-ldc+32", 2, 768, 768, 12, ldc_pad=32, **inplace)
    add("inplace-nobias", 2, 300, 768, 2, bias=False, **inplace)
    add("inplace-small", 2, 1, 16, 2, **inplace)
    add("res-other", 2, 257, 272, 2, **other)
    add("res-other-ldr+4", 2, 300, 48, 4, ldr_pad=4, **other)
    add("res-inplace-ldr!=ldc", 2, 1, 272, 2, ldr_pad=16, **inplace)
    add("res-gelu", 2, 257, 48, 2, act=1, **other)
    for i, (G, Gs, goff, roff) in enumerate(REMAPS):
        N = (272, 16, 48)[i]
        add(f"res2-G{G}", 2, 3 * G, N, (2, 4, 6)[i], res="other", res_mode=2, G=G, Gs=Gs, goff=goff, roff=roff)
    add("remap-res1", 2, 21, 272, 2, G=7, Gs=9, goff=2, **other)
    add("remap-res1-inplace", 2, 300, 256, 2, G=5, Gs=6, goff=1, **inplace)
    add("remap-nores", 2, 15, 48, 2, G=5, Gs=6, goff=1)
    add("bias-ldc=N", 2, 300, 256, 2, ldc_pad=0)
    add("bias-8B-ldc=N", 2, 257, 272, 2, ldc_pad=0)
    add("gelu-fc1-ldc=N", 2, 300, 512, 2, act=1, ldc_pad=0)
    add("inplace-ldc=N", 2, 511, 272, 2, ldc_pad=0, **inplace)
    add("inplace-512-ldc=N", 2, 512, 512, 2, ldc_pad=0, **inplace)
    # ---- policy 2 on shapes vcap_gemm256_ok turns down: the 128x128 kernel
    add("fallback-K", 2, 300, 256, 3, fallback="K is an odd number of K-tiles")
    add("fallback-N", 2, 300, 40, 2, fallback="N % 16")
    add("fallback-ldc", 2, 257, 48, 2, ldc_pad=2, fallback="ldc % 4")
    add("fallback-bias", 2, 257, 48, 2, bias_off=1, fallback="bias not 16-byte aligned")
    add("fallback-res", 2, 257, 48, 2, res_off=1, fallback="residual not 16-byte aligned", **other)
    add("fallback-ldr", 2, 257, 48, 2, ldr_pad=2, fallback="ldr % 4", **other)
    add("fallback-inplace-K", 2, 300, 256, 1, fallback="K is an odd number of K-tiles", **inplace)
    # ---- dense operands, both kernels
    for p, (M, N, kt) in ((1, (257, 200, 3)), (2, (300, 272, 4))):
        add("dense-bias", p, M, N, kt, kind="dense")
        add("dense-gelu", p, M, N, kt, kind="dense", act=1)
        add("dense-inplace", p, M, N, kt, kind="dense", **inplace)
        add("dense-res2", p, 21, N, kt, kind="dense", res="other", res_mode=2, G=7, Gs=9, goff=2, roff=0)
    add("dense-gelu-fc1", 2, 300, 512, 2, kind="dense", act=1)
    add("dense-inplace-512", 2, 512, 512, 12, kind="dense", **inplace)
    return cs


CASES = _cases()

# vcap_gemm_splitk: K-tile counts and the splits the rule gives them
SPLITK_KT = ((3, 1), (5, 1), (6, 2), (9, 3), (12, 4), (15, 5), (18, 6), (21, 7), (24, 8), (48, 8))
_MN = [(m, n) for m in (1, 5, 130) for n in (4, 132, 256)]
SPLITK_CASES = [Case(f"splitk-{kt}kt-{_MN[i % 9][0]}x{_MN[i % 9][1]}", 0, _MN[i % 9][0], _MN[i % 9][1], kt,
                     res="inplace", res_mode=1, splitk=True) for i, (kt, _) in enumerate(SPLITK_KT)]
SPLITK_CASES += [Case("splitk-remap", 0, 15, 132, 12, res="inplace", res_mode=1, splitk=True, G=5, Gs=7),
                 Case("splitk-ldc+4", 0, 5, 256, 24, res="inplace", res_mode=1, splitk=True, ldc_pad=4),
                 Case("splitk-256-shape", 0, 300, 256, 6, res="inplace", res_mode=1, splitk=True)]

# the auto policy's row split on a stream of 16 CUs: 256x256 on rows [0, 4096), 128x128 on the rest
ROWSPLIT_CUS = 16
ROWSPLIT_CASES = [Case("rowsplit-inplace", 0, 4252, 256, 2, res="inplace", res_mode=1),
                  Case("rowsplit-bias", 0, 4252, 256, 2)]

LINEAR_CASE = Case("linear-bias", 0, 5, 200, 4, ldc_pad=0)          # (the entry point has no ldc)


def by_name(name: str) -> Case:
    return next(c for c in CASES + SPLITK_CASES + ROWSPLIT_CASES + [LINEAR_CASE] if c.name == name)
