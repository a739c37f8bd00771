"""Dense GEMM sweep through the C ABI: both tile kernels (csrc/gemm.hip 128x128, csrc/gemm256.hip 256x256), every
epilogue template and store branch, for bf16 / f16 / f32 operands, against the oracle of tests/gemm_cases.py
(tests/test_cpu_gemm_cases.py pins it on the CPU; DESIGN.md "Dense GEMM shapes" lists case against instance).

Exact-operand cases compare the WHOLE C buffer - live elements, the rows a remap skips, PAD_ROWS rows below and the
columns [N, ldc) - as bit patterns: tolerance zero.  Cases with a GELU, and the dense-operand cases, compare the
live elements within the bound gemm_cases derives and everything else bit for bit.  The pad columns of A, W and
of a separate residual hold NaN: reading one poisons an output.  pytest -s prints the instance each case reached,
as gemm_cases.template_of restates the dispatchers (not as observed from the launch).

  1 vcap_gemm under policy 1 (the 128x128 kernel) and policy 2 (the 256x256 kernel where vcap_gemm256_ok takes the
    shape; the fallback cases assert the 128x128 kernel's result under policy 2);
  2 the auto policy's row split (whole 256x256 rounds + a 128x128 remainder) on a stream limited to 16 CUs;
  3 vcap_gemm_splitk: the split-count rule over K-tile counts 3..48, under every policy, on a NaN workspace;
  4 vcap_linear_bias; 5 operand strides past the 256x256 kernel's 32-bit offsets."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_cases as GC
from vcap import _native as N

pytestmark = pytest.mark.gpu
DT = {"bf16": N.DT_BF16, "f16": N.DT_F16, "f32": N.DT_F32}


def _s():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture
def policy():
    def set_policy(p):
        N.check(N.lib().vcap_set_gemm_policy(p), "policy")
    yield set_policy
    N.check(N.lib().vcap_set_gemm_policy(0), "policy")


def _padded(dev, x, ld, tdt, fill=float("nan")):
    rows, cols = x.shape
    buf = np.full((rows, ld), fill)
    buf[:, :cols] = x
    return torch.from_numpy(buf).to(dev).to(tdt)


def _offset(dev, x, off, tdt=torch.float32):
    """A tensor holding x, starting `off` elements into its (16-byte aligned) allocation."""
    flat = torch.zeros(x.size + off + 4, dtype=tdt, device=dev)
    view = flat[off:off + x.size].view(x.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)).to(tdt))
    return flat, view


class Run:
    """One case on the device: operands staged once, launch() callable again (for the repeat checks)."""

    def __init__(self, dev, c, pair, stream=None):
        self.c, self.pair, self.dev, self.stream = c, pair, dev, stream
        in_t, out_t = pair
        self.d = d = GC.operands(c, pair)
        self.a = _padded(dev, d["a"], c.lda(in_t), GC.TORCH[in_t])
        self.w = _padded(dev, d["w"], c.ldw(in_t), GC.TORCH[in_t])
        assert self.a.data_ptr() % 16 == 0 and self.w.data_ptr() % 16 == 0
        self.bias = _offset(dev, d["bias"], c.bias_off) if c.bias else None
        self.res = None
        if c.res == "other":
            r = np.full((d["res"].shape[0], c.ldr), np.nan)
            r[:, :c.N] = d["res"]
            self.res = _offset(dev, r, c.res_off)
            self.res0 = self.res[0].clone()

    def launch(self, c_init, ts=None):
        c, (in_t, out_t) = self.c, self.pair
        esz = GC.SIZE[out_t]
        assert c.c_off % esz == 0
        off = c.c_off // esz
        flat = torch.full((c_init.size + off + 8,), GC.SENT, dtype=GC.TORCH[out_t], device=self.dev)
        out = flat[off:off + c_init.size].view(c_init.shape)
        out.copy_(torch.from_numpy(c_init).to(GC.TORCH[out_t]))
        assert flat.data_ptr() % 16 == 0
        res_ptr = out.data_ptr() if c.res == "inplace" else self.res[1].data_ptr() if self.res else None
        stream = self.stream if self.stream is not None else _s()
        torch.cuda.synchronize()                         # (the staging copies ran on torch's stream)
        N.check(N.lib().vcap_gemm(DT[in_t], DT[out_t], self.a.data_ptr(), c.lda(in_t), self.w.data_ptr(), c.ldw(in_t),
                                  out.data_ptr(), c.ldc, c.M, c.N, c.K(in_t),
                                  self.bias[1].data_ptr() if self.bias else None, c.act, res_ptr, c.ldr, c.res_mode,
                                  c.G, c.Gs, c.goff, c.roff, stream), "vcap_gemm")
        torch.cuda.synchronize()
        if self.res:
            assert torch.equal(self.res[0].view(torch.int32), self.res0.view(torch.int32)), "residual buffer written"
        return flat, out


def _view_bits(t):
    return t.cpu().view(torch.int32 if t.element_size() == 4 else torch.int16).numpy()


def check(c, pair, flat, out, exp, bound, what=""):
    """Bits where the bound is zero, |got - oracle| <= bound elsewhere; the allocation around C untouched."""
    out_t = pair[1]
    got_bits, want_bits = _view_bits(out), GC.bits(exp, out_t)
    strict = bound == 0
    bad = strict & (got_bits != want_bits)
    got = out.double().cpu().numpy()
    assert not bad.any(), (f"{c.name} {pair} {what}: {bad.sum()} of {bad.size} elements differ from the oracle's bits, "
                           f"first at {tuple(np.argwhere(bad)[0])}: got {got[tuple(np.argwhere(bad)[0])]!r}, "
                           f"oracle {exp[tuple(np.argwhere(bad)[0])]!r}")
    if not strict.all():
        err = np.abs(got - exp)
        over = ~strict & ~(err <= bound)
        print(f"    max error / bound {np.max(err[~strict] / bound[~strict]):.3f} over {int((~strict).sum())} elements")
        assert not over.any(), (f"{c.name} {pair} {what}: {over.sum()} elements past the bound, worst "
                                f"{np.max(err[over] / bound[over]):.3g} x at {tuple(np.argwhere(over)[0])}")
    off = c.c_off // GC.SIZE[out_t]
    sent = GC.bits(np.array([GC.SENT]), out_t)[0]
    fb = _view_bits(flat)
    assert (fb[:off] == sent).all() and (fb[off + out.numel():] == sent).all(), "written outside the C buffer"


_PARAMS = [(c, p) for c in GC.CASES for p in c.pairs()]


@pytest.mark.parametrize("c, pair", _PARAMS, ids=[f"{c.name}-{p[0]}-{p[1]}" for c, p in _PARAMS])
def test_gemm_case(device, policy, c, pair):
    ts = GC.template_of(c, pair)
    print(f"\n  {c.name} {pair[0]}->{pair[1]} M={c.M} N={c.N} K={c.K(pair[0])}: {GC.describe(ts)}")
    assert (ts[0]["kernel"] == "128") == (c.policy == 1 or c.fallback is not None)
    run = Run(device, c, pair)
    c_init, exp, bound = GC.oracle(c, pair, run.d, ts=ts)
    policy(c.policy)
    flat, out = run.launch(c_init)
    check(c, pair, flat, out, exp, bound)
    _, again = run.launch(c_init)
    assert np.array_equal(_view_bits(out), _view_bits(again)), "two runs of one call differ"


_ROWSPLIT = [(c, p) for c in GC.ROWSPLIT_CASES for p in c.pairs()]


@pytest.mark.parametrize("c, pair", _ROWSPLIT, ids=[f"{c.name}-{p[0]}-{p[1]}" for c, p in _ROWSPLIT])
def test_auto_policy_row_split(device, policy, c, pair):
    """Policy 0 on a stream of 16 CUs: 17 tiles of 256 rows = one whole round on the 256x256 kernel (rows
    [0, 4096)) and the remaining 156 rows on the 128x128 kernel, the oracle's bits on both sides of the seam."""
    ncu = torch.cuda.get_device_properties(device).multi_processor_count
    ts = GC.template_of(c, pair, cus=GC.ROWSPLIT_CUS)
    print(f"\n  {c.name} {pair[0]}->{pair[1]}: {GC.describe(ts)}")
    assert [(t["kernel"], t["rows"]) for t in ts] == [("256", (0, 4096)), ("128", (4096, 4252))]
    h = C.c_void_p()
    N.check(N.lib().vcap_stream_create_cu_reserved(ncu - GC.ROWSPLIT_CUS, C.byref(h)), "masked stream")
    try:
        run = Run(device, c, pair, stream=h.value)
        c_init, exp, bound = GC.oracle(c, pair, run.d, ts=ts)
        policy(0)
        torch.cuda.synchronize()
        flat, out = run.launch(c_init)
        check(c, pair, flat, out, exp, bound)
    finally:
        torch.cuda.synchronize()
        N.check(N.lib().vcap_stream_destroy(h), "stream destroy")


def _splitk(dev, c, pair, ws_fill=float("nan")):
    in_t = pair[0]
    d = GC.operands(c, pair)
    ts = GC.template_of(c, pair)
    c_init, exp, bound = GC.oracle(c, pair, d, ts=ts)
    a = _padded(dev, d["a"], c.lda(in_t), GC.TORCH[in_t])
    w = _padded(dev, d["w"], c.ldw(in_t), GC.TORCH[in_t])
    bias = torch.from_numpy(d["bias"]).float().to(dev)
    ws = torch.full((8 * c.M * c.N + 16,), ws_fill, device=dev)
    outs = []
    for _ in range(2):
        flat = torch.full((c_init.size + 8,), GC.SENT, device=dev)
        out = flat[:c_init.size].view(c_init.shape)
        out.copy_(torch.from_numpy(c_init).float())
        splits = C.c_int(-1)
        N.check(N.lib().vcap_gemm_splitk(DT[in_t], a.data_ptr(), c.lda(in_t), w.data_ptr(), c.ldw(in_t), out.data_ptr(),
                                         c.ldc, c.M, c.N, c.K(in_t), bias.data_ptr(), c.G, c.Gs, ws.data_ptr(),
                                         8 * c.M * c.N * 4, C.byref(splits), _s()), "vcap_gemm_splitk")
        torch.cuda.synchronize()
        outs.append((flat, out, splits.value))
    assert torch.isnan(ws[8 * c.M * c.N:]).all(), "written past 8 * M * N floats of the workspace"
    return ts, exp, bound, outs


@pytest.mark.parametrize("pol", [0, 1, 2])
@pytest.mark.parametrize("pair", [("bf16", "f32"), ("f16", "f32")], ids="-".join)
@pytest.mark.parametrize("c", GC.SPLITK_CASES, ids=lambda c: c.name)
def test_gemm_splitk(device, policy, c, pair, pol):
    policy(pol)
    ts, exp, bound, outs = _splitk(device, c, pair)
    want = GC.gemm_splits(c.kt)
    print(f"\n  {c.name} {pair[0]} policy {pol}: {want} splits; {GC.describe(GC.template_of(c, pair, policy=pol))}")
    (flat, out, splits), (_, again, splits2) = outs
    assert splits == splits2 == want
    if want > 1:                                         # a launch that splits keeps the 128x128 kernel
        assert GC.template_of(c, pair, policy=pol)[0]["kernel"] == "128"
    check(c, pair, flat, out, exp, bound, f"policy {pol}")
    assert np.array_equal(_view_bits(out), _view_bits(again)), "two runs of one call differ"


def test_gemm_splitk_small_workspace_is_refused(device):
    c = GC.SPLITK_CASES[4]
    a = torch.zeros(c.M, c.K("bf16"), dtype=torch.bfloat16, device=device)
    w = torch.zeros(c.N, c.K("bf16"), dtype=torch.bfloat16, device=device)
    out, bias, ws = (torch.zeros(n, device=device) for n in (c.M * c.N, c.N, 8 * c.M * c.N))
    rc = N.lib().vcap_gemm_splitk(N.DT_BF16, a.data_ptr(), c.K("bf16"), w.data_ptr(), c.K("bf16"), out.data_ptr(), c.N,
                                  c.M, c.N, c.K("bf16"), bias.data_ptr(), 0, 0, ws.data_ptr(), 8 * c.M * c.N * 4 - 4,
                                  None, _s())
    assert rc == N.E_WORKSPACE
    torch.cuda.synchronize()
    assert not bool(out.any())


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_linear_bias_exact(device, policy, dtype):
    c, pair = GC.LINEAR_CASE, (dtype, dtype)
    d = GC.operands(c, pair)
    _, exp, bound = GC.oracle(c, pair, d)
    t = GC.TORCH[dtype]
    x, w = torch.from_numpy(d["a"]).to(device).to(t), torch.from_numpy(d["w"]).to(device).to(t)
    b = torch.from_numpy(d["bias"]).float().to(device)
    flat = torch.full(((c.M + GC.PAD_ROWS) * c.N,), GC.SENT, dtype=t, device=device)
    y = flat.view(c.M + GC.PAD_ROWS, c.N)
    policy(0)
    N.check(N.lib().vcap_linear_bias(DT[dtype], x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), c.M, c.K(dtype),
                                     c.N, _s()), "vcap_linear_bias")
    torch.cuda.synchronize()
    check(c, pair, flat, y, exp, bound)


@pytest.mark.parametrize("side", ["lda", "ldw"])
def test_operand_stride_past_32_bit_offsets(device, policy, side):
    """Operand rows so far apart that the last row starts 2^32 bytes or more into a single ~4 GiB allocation, of
    which only the rows themselves are written: A with M = 2 rows 2^31 + 64 bf16 elements apart, and W with
    N = 16 rows (the 256x256 kernel's smallest N) 2^32 / 30 elements apart.  The 256x256 kernel keeps a lane's
    operand byte offset in 32 bits, so vcap_gemm256_ok turns such a shape down and policy 2 runs the 128x128
    kernel, which addresses with long.  Before that guard the last row's offset wrapped to a few bytes into the
    first row: wrong values from inside the same allocation, no fault."""
    if torch.cuda.mem_get_info()[0] < 8 << 30:
        pytest.skip("needs 8 GiB of free device memory")
    K, nfar = 128, 2 if side == "lda" else 16
    ld = 2 ** 31 + 64 if side == "lda" else (2 ** 32 // 30 // 8 + 8) * 8
    assert (nfar - 1) * ld * 2 >= 2 ** 32 and ld % 8 == 0
    assert GC.offsets_overflow(2, ld, 16, K, K, 2) if side == "lda" else GC.offsets_overflow(48, K, 16, ld, K, 2)
    g = np.random.default_rng(5)
    far = g.integers(-8, 9, (nfar, K)).astype(np.float64)
    near = g.integers(-4, 5, (48 if side == "ldw" else 16, K)).astype(np.float64)
    big = torch.empty((nfar - 1) * ld + K, dtype=torch.bfloat16, device=device)
    big[:4096].zero_()                                   # where a wrapped offset would read
    rows = torch.as_strided(big, (nfar, K), (ld, 1))
    rows.copy_(torch.from_numpy(far).to(torch.bfloat16))
    small = torch.from_numpy(near).to(device).to(torch.bfloat16)
    bias = torch.from_numpy(g.integers(-32, 33, 16) / 4.0).float().to(device)
    if side == "lda":
        M, a, lda, w, ldw, ref = 2, rows, ld, small, K, far @ near.T
    else:
        M, a, lda, w, ldw, ref = 48, small, K, rows, ld, near @ far.T
    ref = ref + bias.double().cpu().numpy()
    out = torch.full((M + 1, 16), GC.SENT, device=device)
    policy(2)
    N.check(N.lib().vcap_gemm(N.DT_BF16, N.DT_F32, a.data_ptr(), lda, w.data_ptr(), ldw, out.data_ptr(), 16, M, 16, K,
                              bias.data_ptr(), 0, None, 0, 0, 0, 0, 0, 0, _s()), "vcap_gemm")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:M].view(np.uint32), ref.astype(np.float32).view(np.uint32))
    assert (got[M:] == GC.SENT).all()
