"""The fp16 ViT precision (the reference's autocast dtype, src/models/video_encoder.py:261-264) on the
host side: the ABI constants, the surface that selects it, and the host-only size arithmetic that must
not read VCAP_DT_F16 as a 4-byte element type."""
import ctypes as C
import re
from pathlib import Path

import pytest

from vcap import _native as N
from vcap import configs

ROOT = Path(__file__).resolve().parents[1]


def test_header_and_binding_agree_on_f16_and_version():
    h = (ROOT / "include" / "vcap.h").read_text()
    assert int(re.search(r"#define VCAP_ABI_VERSION (\d+)", h).group(1)) == 16 == N.ABI_VERSION
    enum = re.search(r"enum \{ VCAP_DT_F32 = 0,[^}]*\}", h).group(0)
    assert int(re.search(r"VCAP_DT_F16 = (\d+)", enum).group(1)) == 3 == N.DT_F16
    assert (N.DT_F32, N.DT_BF16, N.DT_MXFP8) == (0, 1, 2)
    assert N.lib().vcap_abi_version() == 16
    for fn in ("vcap_vit_qkv_attention_dt", "vcap_gemm_splitk"):
        assert fn in h and fn in N.SIGNATURES
    common = (ROOT / "video-caption-algorithm_amd" / "csrc" / "vcap_common.h").read_text()
    assert re.search(r"VCAP_DT_F16 = 3\b", common)


def test_cli_and_config_accept_fp16():
    from core.config import InferenceConfig
    from src.cli.inference import parse
    assert parse(["--video_path", "d", "--precision", "fp16"]).precision == "fp16"
    assert parse(["--video_path", "d"]).precision == "bf16"          # the default stays
    assert InferenceConfig().precision == "bf16"
    assert InferenceConfig(precision="fp16").precision == "fp16"
    with pytest.raises(SystemExit):
        parse(["--video_path", "d", "--decoder_precision", "fp16"])
    # the decoder keeps the reference's fp32 under an fp16 ViT and has no fp16 mode of its own
    from vcap.caption import resolve_decoder_precision
    assert resolve_decoder_precision("fp16") == "fp32"
    assert resolve_decoder_precision("fp16", "bf16") == "bf16"
    for vit in ("fp16", "bf16"):
        with pytest.raises(ValueError):
            resolve_decoder_precision(vit, "fp16")


def test_model_tables_offer_fp16_to_the_vit_only():
    import torch

    from vcap import model
    assert model._VIT_DTYPES["fp16"] == (N.DT_F16, torch.float16)
    assert "fp16" not in model._DTYPES                               # HipGPT2Decoder(..., "fp16") raises
    with pytest.raises(ValueError):
        model._dtype("fp16")


def test_rows_pack_refuses_f16():
    assert N.lib().vcap_rows_packed_bytes(N.DT_F16, 64, 64) == 0
    assert N.lib().vcap_rows_packed_bytes(N.DT_BF16, 64, 64) > 0


def _vit_desc(dt, arch, kpad):
    layers = (N.VitLayer * arch.depth)()
    return N.VitDesc(dtype=dt, dim=arch.dim, depth=arch.depth, heads=arch.heads, patch=arch.patch, image=arch.image,
                     mlp=arch.mlp, video_dim=256, kpad=kpad, ln_eps=arch.ln_eps, layers=layers), layers


def test_vit_workspace_of_f16_equals_bf16():
    """Host-only: a 2-byte operand type sizes the workspace as bf16 does (an `esize` that knows only
    bf16 would size fp16 buffers as f32, or refuse the descriptor and return 0)."""
    arch = configs.vit_arch("vit_base_patch16_224")
    kpad = ((arch.patch_k + 63) // 64) * 64
    sizes = {}
    for dt in (N.DT_BF16, N.DT_F16, N.DT_F32):
        desc, keep = _vit_desc(dt, arch, kpad)
        sizes[dt] = int(N.lib().vcap_vit_workspace_bytes(C.byref(desc), 2, 16))
    assert sizes[N.DT_F16] == sizes[N.DT_BF16] > 0
    assert sizes[N.DT_F32] > sizes[N.DT_BF16]
    desc, keep = _vit_desc(N.DT_F16, arch, kpad)
    assert int(N.lib().vcap_vit_layer_fuses_qkv_attention(C.byref(desc), 0)) == 1     # 197 tokens: fused in fp16 too
    l14 = configs.vit_arch("vit_large_patch14_224")
    desc, keep = _vit_desc(N.DT_F16, l14, ((l14.patch_k + 63) // 64) * 64)
    assert int(N.lib().vcap_vit_layer_fuses_qkv_attention(C.byref(desc), 0)) == 1     # 257 tokens
