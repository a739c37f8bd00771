"""Fused QKV projection + attention (vcap_vit_qkv_attention) against the unfused pair (vcap_gemm with
bias into a qkv buffer, then vcap_vit_attention) at the ViT-B/16 frame shape: bit-identity of the
outputs (all rows, and the class-token-only form) and the median time per launch of each.
Environment: BT (frames, default 256 = one 16-video encode), NT / H (tokens / heads: 197 / 12 = ViT-B/16,
257 / 16 = ViT-L/14), REPS, DTYPES (comma list of bf16 / fp16, default bf16: each listed operand type is
checked and timed in turn in this one process; list a type twice to see the run's drift)."""
import os
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "video-caption-algorithm_amd"))
import torch  # noqa: E402

from vcap import _native as N  # noqa: E402

BT, NT, H = int(os.environ.get("BT", "256")), int(os.environ.get("NT", "197")), int(os.environ.get("H", "12"))
D = H * 64
dev = torch.device("cuda:0")
DT = {"bf16": (N.DT_BF16, torch.bfloat16), "fp16": (N.DT_F16, torch.float16)}


def bench(dname):
    dt, tdt = DT[dname]
    g = torch.Generator(device=dev).manual_seed(0)
    xn = torch.randn(BT * NT, D, generator=g, device=dev).to(tdt)
    w = (0.02 * torch.randn(3 * D, D, generator=g, device=dev)).to(tdt)
    b = 0.02 * torch.randn(3 * D, generator=g, device=dev)
    qkv = torch.empty(BT * NT, 3 * D, device=dev, dtype=tdt)
    ref = torch.empty(BT * NT, D, device=dev, dtype=tdt)
    out = torch.empty(BT * NT, D, device=dev, dtype=tdt)
    s = torch.cuda.current_stream().cuda_stream
    lib = N.lib()

    def unfused():
        N.check(lib.vcap_gemm(dt, dt, xn.data_ptr(), D, w.data_ptr(), D, qkv.data_ptr(), 3 * D, BT * NT,
                              3 * D, D, b.data_ptr(), 0, None, 0, 0, 0, 0, 0, 0, s), "qkv gemm")
        N.check(lib.vcap_vit_attention(dt, qkv.data_ptr(), ref.data_ptr(), BT, NT, H, s), "attn")

    def fused(cls_only=0):
        N.check(lib.vcap_vit_qkv_attention_dt(dt, xn.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), BT, NT, H,
                                              cls_only, s), "qkv_attention")

    unfused()
    fused()
    torch.cuda.synchronize()
    same = torch.equal(out.view(torch.int16), ref.view(torch.int16))
    diff = (out.float() - ref.float()).abs()
    print(f"[{dname}] all rows: bit-identical {same}  max |diff| {float(diff.max()):.3e}  rows differing "
          f"{int((diff.amax(1) > 0).sum())} of {BT * NT}", flush=True)
    fused(1)
    torch.cuda.synchronize()
    cls_ref = ref.view(BT, NT, D)[:, 0]
    same_cls = torch.equal(out[:BT].view(torch.int16), cls_ref.contiguous().view(torch.int16))
    print(f"[{dname}] class-token rows: bit-identical {same_cls}", flush=True)

    def timed(fn, reps):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / 10 * 1e3)
        return statistics.median(ts)

    reps = int(os.environ.get("REPS", "7"))
    tg = timed(lambda: lib.vcap_gemm(dt, dt, xn.data_ptr(), D, w.data_ptr(), D, qkv.data_ptr(), 3 * D,
                                     BT * NT, 3 * D, D, b.data_ptr(), 0, None, 0, 0, 0, 0, 0, 0, s), reps)
    ta = timed(lambda: lib.vcap_vit_attention(dt, qkv.data_ptr(), ref.data_ptr(), BT, NT, H, s), reps)
    tf = timed(fused, reps)
    fl_g = 2.0 * BT * NT * D * 3 * D
    fl_a = 4.0 * BT * H * NT * NT * 64
    print(f"[{dname}] BT={BT}: qkv gemm {tg:.1f} us + attention {ta:.1f} us = {tg + ta:.1f} us | fused {tf:.1f} us "
          f"({(tg + ta) / tf:.3f}x)  fused {(fl_g + fl_a) / tf / 1e6:.0f} TF/s = {(fl_g + fl_a) / tf / 1e6 / 2500:.3f} "
          f"of the 2.5 PF/s dense peak", flush=True)


for _d in [d for d in os.environ.get("DTYPES", "bf16").split(",") if d]:
    bench(_d)
