"""ViT attention on inputs where a key masking or key / row indexing fault is O(|v|) (tests/attention_edge_cases.py
builds them, test_cpu_attention_edges.py checks them and the size of the faults on the CPU), at the token counts
on both sides of every kernel choice of vcap_vit_attention_dispatch:

  bf16 / fp32   1, 2, 17, 32 (kt = 2) | 193, 197, 208 (kt = 14, KE = 13), 209, 224 (KE = 14) | 257, 272 (kt = 18,
                KE = 17), 273, 288 (KE = 18)
  fp16          the same, and the generic kernel at 33, 64 | 65, 128 | 129, 192 | 225, 256
  fused         193, 197, 208 (vcap_vit_qkv_attention_kernel) | 257, 272 (the _l_ kernel), bf16 and fp16, with and
                without cls_only

Patterns: a dominant key j (j over the first and last keys and both sides of the 16- and 32-key tile edges), all
keys equal (the mean of v: a padding key with score 0 would take 0.94 of the weight), and a permutation (row i
picks key (7 i + 3) mod N).  Reference: fp64 softmax(q k^T / 8) v on the same inputs; tolerance f32 1e-5, 2-byte
types 3 x max |emulated - fp64| per input, from the CPU alone (about 3e-4 / 1.4e-3 / 1e-2 for the three patterns
in bf16 at 197 tokens).  The fused kernel must also equal the unfused pair bit for bit, and its cls_only form the
class-token rows of the full run, with nothing written past the compact rows.

  mxfp8         vcap_vit_attention_mx (bf16 in, MXFP8 out) at heads = 4: 2, 17, 32 (<2,2,4>) | 197, 208 (<14,13,8>) |
                209, 224 (<14,14,8>) | 257, 272 (<18,17,8>) | 273, 288 (<18,18,8>); the bound is half an e4m3 step
                of the element's block + the bf16 tolerance, the scales within the window that tolerance leaves
                around a power of two (tests/mx_cases.py attention_mx_check)

These are the first runs of vcap_vit_attention_bf16_kernel<2, 2, 4> and vcap_vit_attention_kernel<float, 2>
outside an encode (tests/test_gpu_encoder_shapes.py case 2 runs them inside one)."""
import pytest
import torch

import attention_edge_cases as A
import mx_cases as MX
from oracle import vcap_oracle as O
from vcap import _native as N

pytestmark = pytest.mark.gpu
DT = {"bf16": N.DT_BF16, "fp16": N.DT_F16, "fp32": N.DT_F32}
RUNS = [(p, n, 2, 2) for p in ("bf16", "fp16", "fp32") for n in A.TOKENS[p]] + \
       [(p, 197, 2, 1) for p in ("bf16", "fp16", "fp32")]
FUSED = [(p, n, 2) for p in ("bf16", "fp16") for n in A.FUSED_TOKENS] + [("bf16", 197, 8), ("fp16", 257, 8)]


def _s():
    return torch.cuda.current_stream().cuda_stream


def _attention(prec, qkv, frames, n, heads):
    out = torch.full((frames * n, heads * 64), float("nan"), dtype=A.TORCH[prec], device=qkv.device)
    N.check(N.lib().vcap_vit_attention(DT[prec], qkv.data_ptr(), out.data_ptr(), frames, n, heads, _s()), "attention")
    return out


def _check(prec, x, got, tag):
    """got [frames * n, D] device tensor against the fp64 reference of x [frames, n, 3, heads, 64]."""
    ref = A.attend(x)
    tol = A.tolerance(x, prec, ref)
    g = got.double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(g).all()), tag
    err = float((g - ref).abs().max())
    print(f"\nattention-gpu {tag}: max|gpu-fp64|={err:.3e} (tol {tol:.3e})", end="")
    assert err <= tol, (tag, err, tol)


@pytest.mark.parametrize("prec,n,frames,heads", RUNS, ids=[f"{p}-n{n}-f{f}-h{h}" for p, n, f, h in RUNS])
def test_attention_edges(device, prec, n, frames, heads):
    for pattern, j in A.variants(n):
        x = A.qkv(pattern, prec, n, frames, heads, j)
        qkv = x.reshape(frames * n, 3 * heads * 64).to(A.TORCH[prec]).to(device)
        _check(prec, x, _attention(prec, qkv, frames, n, heads), f"{prec} N={n} H={heads} {pattern}{'' if j is None else j}")


def _fused(prec, xn, w, b, frames, n, heads, cls_only):
    out = torch.full((frames * n, heads * 64), float("nan"), dtype=xn.dtype, device=xn.device)
    N.check(N.lib().vcap_vit_qkv_attention_dt(DT[prec], xn.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(),
                                              frames, n, heads, cls_only, _s()), "qkv_attention_dt")
    return out


@pytest.mark.parametrize("prec,n,frames", FUSED, ids=[f"{p}-n{n}-f{f}" for p, n, f in FUSED])
def test_fused_attention_edges(device, prec, n, frames):
    heads, d, tdt = 2, 128, A.TORCH[prec]
    for pattern, j in A.variants(n):
        tag = f"fused {prec} N={n} F={frames} {pattern}{'' if j is None else j}"
        xn64, w64, b64, qk = A.fused_inputs(pattern, prec, n, frames, heads, j)
        xn, w, b = xn64.to(tdt).to(device), w64.to(tdt).to(device), b64.float().to(device)
        qkv = torch.empty(frames * n, 3 * d, dtype=tdt, device=device)
        N.check(N.lib().vcap_gemm(DT[prec], DT[prec], xn.data_ptr(), d, w.data_ptr(), d, qkv.data_ptr(), 3 * d,
                                  frames * n, 3 * d, d, b.data_ptr(), 0, None, 0, 0, 0, 0, 0, 0, _s()), "qkv gemm")
        x = qkv.double().cpu().reshape(frames, n, 3, heads, 64)
        assert torch.equal(x[:, :, :2], qk), tag            # the projection gives the pattern's q / k exactly
        unfused = _attention(prec, qkv, frames, n, heads)
        _check(prec, x, unfused, tag)                       # v: the projection's own rounded output
        full = _fused(prec, xn, w, b, frames, n, heads, 0)
        assert torch.equal(full.view(torch.int16), unfused.view(torch.int16)), tag
        cls = _fused(prec, xn, w, b, frames, n, heads, 1)
        want = full.view(frames, n, d)[:, 0].contiguous()
        assert torch.equal(cls[:frames].view(torch.int16), want.view(torch.int16)), tag
        assert bool(torch.isnan(cls[frames:].float()).all()), tag


@pytest.mark.parametrize("n", A.MX_TOKENS)
def test_attention_edges_mxfp8(device, n):
    """The fourth precision: the three patterns through vcap_vit_attention_mx, 2 frames x 4 heads (197 and 257
    tokens cross a 256-row scale group).  Nothing is written past the last row or past vcap_mx_scale_bytes."""
    frames, heads = 2, A.MX_HEADS
    M, D = frames * n, heads * 64
    nsc = int(N.lib().vcap_mx_scale_bytes(M, D))
    for pattern, j in A.variants(n):
        tag = f"mxfp8 N={n} H={heads} {pattern}{'' if j is None else j}"
        x = A.qkv(pattern, "bf16", n, frames, heads, j)
        qkv = x.reshape(M, 3 * D).to(torch.bfloat16).to(device)
        q = torch.full((M + 1, D), 0xA5, dtype=torch.uint8, device=device)
        sc = torch.full((nsc + 64,), 0xA5, dtype=torch.uint8, device=device)
        N.check(N.lib().vcap_vit_attention_mx(qkv.data_ptr(), q.data_ptr(), sc.data_ptr(), frames, n, heads, _s()), "attention_mx")
        torch.cuda.synchronize()
        ref = A.attend(x)
        term = A.tolerance(x, "bf16", ref)
        qg, sflat = q.cpu().numpy(), sc.cpu().numpy()
        bad = MX.attention_mx_check(ref.reshape(M, D).numpy(), term, qg[:M], O.mx_unpack_scales(sflat[:nsc], M, D))
        print(f"\nattention-gpu {tag}: instance {MX.attention_instance(n)}, bf16 term {term:.3e}", end="")
        assert not bad, (tag, bad)
        assert (qg[M:] == 0xA5).all() and (sflat[nsc:] == 0xA5).all(), tag
