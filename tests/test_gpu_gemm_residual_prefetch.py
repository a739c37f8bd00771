"""The 256x256 GEMM's in-place f32 residual epilogue fetches its residual tile under the K loop for bf16 and
f16 operands (csrc/gemm256.hip, ResPieces; f32 and MXFP8 operands keep the register epilogue and are held to
the same checks).  It must store the bytes of the plain epilogue:

  * in place (res == C, ldr == ldc) the launch takes the prefetching epilogue; with the residual in one
    buffer and the output in another it takes the same kernel's general epilogue, which applies the same
    formula rnd(acc + bias) + res after the same K loop.  The two outputs are compared bit for bit, for
    bf16, f16 and f32 operands (vcap_gemm, GEMM policy 2) and for MXFP8 operands (vcap_gemm_mx);
  * two runs of one call give the same bytes;
  * rows >= M and columns [N, ldc) of C keep a sentinel.

Shapes: the K loop's only iteration is its last (two K-tiles: K = 128 for the 16-bit types, 64 for f32,
256 for MXFP8), a partial row tile and a partial column tile (tiles with an edge keep the register
epilogue with its M - 1 / N - 4 clamps, next to whole tiles that prefetch, in one launch), a long K,
ldc > N, and a launch without a bias.  MXFP8 needs K % 256 == 0, so its K = 128 case runs at K = 256."""
import numpy as np
import pytest
import torch

from vcap import _native as N

pytestmark = pytest.mark.gpu

SENT = -12345.5
PAD_ROWS = 3

#          M    N    K     ldc
SHAPES = [(256, 256, 128, 256),    # two K-tiles (16-bit operands)
          (300, 768, 768, 768),    # partial row tile
          (511, 272, 256, 272),    # partial column tile
          (512, 256, 3072, 256),   # long K
          (768, 768, 768, 800)]    # ldc > N
TORCH_DT = {"bf16": (torch.bfloat16, N.DT_BF16), "f16": (torch.float16, N.DT_F16), "f32": (torch.float32, N.DT_F32)}


def _s():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture
def policy256():
    assert N.lib().vcap_set_gemm_policy(2) == 0
    yield
    assert N.lib().vcap_set_gemm_policy(0) == 0


def _operands(device, M, N_, K, ldc, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    a = (torch.rand(M, K, generator=g) * 2 - 1).to(device)
    w = ((torch.rand(N_, K, generator=g) * 2 - 1) * 0.05).to(device)
    bias = (torch.rand(N_, generator=g) * 2 - 1).to(device)
    c0 = torch.full((M + PAD_ROWS, ldc), SENT, dtype=torch.float32, device=device)
    c0[:M, :N_] = torch.randn(M, N_, generator=g).to(device)
    return a, w, bias, c0


def _check(run, c0, M, N_):
    """run(C, res) launches the GEMM; c0 holds the residual in [:M, :N_] and the sentinel elsewhere."""
    inplace = c0.clone()
    run(inplace, inplace)
    again = c0.clone()
    run(again, again)
    res, apart = c0.clone(), torch.full_like(c0, SENT)
    run(apart, res)
    torch.cuda.synchronize()
    got, rep, ref = (t.cpu().numpy().view(np.uint32) for t in (inplace, again, apart))
    assert np.array_equal(res.cpu().numpy().view(np.uint32), c0.cpu().numpy().view(np.uint32)), "residual buffer written"
    assert not np.array_equal(got[:M, :N_], c0.cpu().numpy().view(np.uint32)[:M, :N_]), "nothing was added"
    diff = got[:M, :N_] != ref[:M, :N_]
    assert not diff.any(), f"{diff.sum()} of {diff.size} words differ from the general epilogue, first at {np.argwhere(diff)[0]}"
    assert np.array_equal(got, rep), "two runs of one call differ"
    sent = np.float32(SENT).view(np.uint32)
    for name, t in (("in place", got), ("apart", ref)):
        assert (t[M:] == sent).all(), f"{name}: rows >= M written"
        assert (t[:, N_:] == sent).all(), f"{name}: columns [N, ldc) written"


def _run_gemm(dt, a, w, bias, M, N_, K, ldc):
    def run(c, res):
        N.check(N.lib().vcap_gemm(dt, N.DT_F32, a.data_ptr(), K, w.data_ptr(), K, c.data_ptr(), ldc, M, N_, K,
                                  bias.data_ptr() if bias is not None else None, 0, res.data_ptr(), ldc, 1, 0, 0, 0, 0,
                                  _s()), "vcap_gemm")
    return run


# (the two-K-tile shape of f32 operands, K = 64, is no 256x256-kernel shape for the 16-bit types)
@pytest.mark.parametrize("dtype,M,N_,K,ldc", [(d, *sh) for d in ("bf16", "f16", "f32") for sh in SHAPES] +
                         [("f32", 256, 256, 64, 256)])
def test_in_place_residual_matches_general_epilogue(device, policy256, dtype, M, N_, K, ldc):
    tdt, dt = TORCH_DT[dtype]
    a, w, bias, c0 = _operands(device, M, N_, K, ldc, M + K)
    _check(_run_gemm(dt, a.to(tdt), w.to(tdt), bias, M, N_, K, ldc), c0, M, N_)


def test_in_place_residual_without_bias(device, policy256):
    M, N_, K, ldc = 300, 768, 768, 768
    a, w, _, c0 = _operands(device, M, N_, K, ldc, 7)
    _check(_run_gemm(N.DT_BF16, a.bfloat16(), w.bfloat16(), None, M, N_, K, ldc), c0, M, N_)


def _quantize(x):
    rows, K = x.shape
    q = torch.empty(rows, K, dtype=torch.uint8, device=x.device)
    sc = torch.zeros(int(N.lib().vcap_mx_scale_bytes(rows, K)), dtype=torch.uint8, device=x.device)
    N.check(N.lib().vcap_mx_quantize(N.DT_F32, x.data_ptr(), K, rows, K, q.data_ptr(), sc.data_ptr(), _s()), "quantize")
    return q, sc


@pytest.mark.parametrize("M,N_,K,ldc", [(m, n, max(k, 256), ldc) for m, n, k, ldc in SHAPES])
def test_in_place_residual_matches_general_epilogue_mxfp8(device, M, N_, K, ldc):
    a, w, bias, c0 = _operands(device, M, N_, K, ldc, M + K + 1)
    (aq, asc), (wq, wsc) = _quantize(a), _quantize(w)

    def run(c, res):
        N.check(N.lib().vcap_gemm_mx(aq.data_ptr(), asc.data_ptr(), wq.data_ptr(), wsc.data_ptr(), N.DT_F32,
                                     c.data_ptr(), ldc, None, M, N_, K, bias.data_ptr(), 0, res.data_ptr(), _s()),
                "vcap_gemm_mx")
    _check(run, c0, M, N_)
