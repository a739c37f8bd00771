"""Fused ViT token pool + temporal mean on the HIP path (replaces vit_fused_pool_temporal,
core/operators/cupy_vit_pool.py:127-186): returns None on unsupported shape/device, as the
reference does, so a caller can choose its own path; HIP errors raise."""
from __future__ import annotations

import torch

from vcap import _native as N


def vit_fused_pool_temporal(feat: torch.Tensor, bsz: int, timesteps: int, pool: str, force_bf16: bool = False,
                            force_fp16: bool = False):
    """force_fp16 (the reference's argument, its vit_pool_*_f16 kernels) or an fp16 input: the F16 kernel,
    fp32 accumulation, fp16 result."""
    if force_bf16 and force_fp16:
        raise ValueError("vit_fused_pool_temporal: force_bf16 and force_fp16 are exclusive")
    if not feat.is_cuda or feat.ndim != 3 or pool not in {"cls", "gap"}:
        return None
    bt, tokens, channels = feat.shape
    if bt != bsz * timesteps or (pool == "gap" and tokens <= 1):
        return None
    if force_fp16 or (feat.dtype == torch.float16 and not force_bf16):
        dt, tdt = N.DT_F16, torch.float16
    elif force_bf16 or feat.dtype == torch.bfloat16:
        dt, tdt = N.DT_BF16, torch.bfloat16
    else:
        dt, tdt = N.DT_F32, torch.float32
    x = feat.to(tdt).contiguous()
    out = torch.empty(bsz, channels, dtype=tdt, device=feat.device)
    N.check(N.lib().vcap_vit_pool_temporal(dt, x.data_ptr(), out.data_ptr(), bsz, timesteps, tokens, channels,
                                           int(pool == "gap"), torch.cuda.current_stream(feat.device).cuda_stream),
            "vcap_vit_pool_temporal")
    return out
