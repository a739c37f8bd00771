"""Every argument refusal of the host runtime (csrc/runtime_gpt2.hip, runtime_vit.hip) that returns
before the first launch, called through the C ABI with no GPU: a literal table of (entry point, the one
argument made bad, code, vcap_last_error() text), one row per distinct refusal.  The descriptors carry
dummy non-null pointers; nothing is ever dereferenced on the device because every row is refused.
Also pins the four GPT-2 workspace queries, whose carving the entry points share.

Rows marked "isnew" are refusals that came with the shared prompt checks: vcap_gpt2_sample and
vcap_gpt2_beam_search with no context row (they used to launch on zero rows) and vcap_gpt2_prefill with
a prompt id outside the vocabulary (it used to embed it).  Greedy and sampling decode have no row for a
context above 1024: with at most 512 prefill rows and 64 new tokens no call reaches it.  The "isnew" rows of
vcap_vit_encode came with the encoder shape sweep (tests/encoder_shapes.py): shapes check_vit used to accept and
the encode then failed on after its first launches (-hipErrorInvalidValue from "attention" / "head_prefix").  Those of
vcap_vit_attention_mx came with the MXFP8 kernel sweep (tests/test_gpu_mx_sweep.py): 33..192 and 225..256 tokens
used to come back from the dispatcher as -hipErrorInvalidValue ("invalid argument"), not as a documented code; the
entry point now asks vcap_vit_attention_supported before the dispatcher.  The rows of vcap_gemm / vcap_gemm_splitk came
with the dense GEMM sweep (tests/test_gpu_gemm_sweep.py); "isnew" there: an operand dtype or an (operand, output) pair
the dispatcher used to turn down as -hipErrorInvalidValue, and operands that are not 16-byte aligned with row strides in whole 16-byte vectors,
which used to launch the 128x128 kernel's 16-byte LDS-DMA on misaligned addresses.  The rows of vcap_frames_preprocess,
vcap_jpeg_decode_batch and vcap_jpeg_probe came with the JPEG / preprocess sweep (tests/test_gpu_jpeg_sweep.py,
tests/test_gpu_preprocess.py); "isnew" there: a null workspace, which vcap_frames_preprocess used to hand to its kernels."""
import ctypes as C

import pytest

import jpeg_cases as JC
from vcap import _native as N

ARG, WS, UNSUP = N.E_ARG, N.E_WORKSPACE, N.E_UNSUPPORTED

_BUF = C.create_string_buffer(4096)
P = C.addressof(_BUF)                      # a non-null address no refused call reads
_GLAYERS = (N.GPT2Layer * 2)()
_VLAYERS = (N.VitLayer * 2)()


def _gpt2(**kw):
    f = dict(dtype=N.DT_F32, n_embd=128, n_layer=2, n_head=2, vocab=512, n_positions=64, prefix_len=4, ln_eps=1e-5,
             wte=P, lm_head=P, wpe=P, lnf_g=P, lnf_b=P, layers=_GLAYERS, lm_head_screen=None, screen_bound=0.0)
    f.update(kw)
    return N.GPT2Desc(**f)


def _vit(**kw):
    f = dict(dtype=N.DT_F32, dim=128, depth=2, heads=2, patch=16, image=224, mlp=512, video_dim=256, kpad=768,
             ln_eps=1e-6, patch_w=P, patch_b=P, cls=P, pos=P, norm_g=P, norm_b=P, proj_w=P, proj_b=P, layers=_VLAYERS)
    f.update(kw)
    return N.VitDesc(**f)


def _gen(**kw):
    f = dict(max_new_tokens=8, min_new_tokens=0, no_repeat_ngram_size=0, repetition_penalty=1.0, eos_token_id=511,
             pad_token_id=511, use_graph=0, max_blocks=0)
    f.update(kw)
    return N.GenParams(**f)


def _beam(**kw):
    f = dict(num_beams=3, max_new_tokens=8, min_new_tokens=0, no_repeat_ngram_size=0, repetition_penalty=1.0,
             length_penalty=1.0, early_stopping=0, eos_token_id=511, use_graph=0, max_blocks=0)
    f.update(kw)
    return N.BeamParams(**f)


def _samp(**kw):
    f = dict(temperature=0.7, top_k=50, top_p=0.9, seed=1)
    f.update(kw)
    return N.SampleParams(**f)


BIG = 1 << 30
_MEAN, _STD = (C.c_float * 3)(0.485, 0.456, 0.406), (C.c_float * 3)(0.229, 0.224, 0.225)
_JPEG = JC.case("samp_grey_8x8").data                                  # an accepted 8x8 image
_SHORT_SOS = next(d[1] for d in JC.DAMAGED if d[0] == "sos_without_selectors")
_BLOBS = {k: C.create_string_buffer(v, len(v)) for k, v in (("ok", _JPEG), ("short", _SHORT_SOS))}


def _ptrs(key):
    return (C.c_void_p * 1)(C.cast(_BLOBS[key], C.c_void_p))


_LENS, _NOLEN = (C.c_size_t * 1)(len(_JPEG)), (C.c_size_t * 1)(0)
_SHORT, _SHORT_LENS, _NULL_IMAGE = _ptrs("short"), (C.c_size_t * 1)(len(_SHORT_SOS)), (C.c_void_p * 1)(None)
_NAMED = {id(_NOLEN): "zero", id(_SHORT): "short_sos", id(_SHORT_LENS): "short_sos", id(_NULL_IMAGE): "null_image"}
# entry point -> its parameters in ABI order, each with a value every check accepts
GOOD = {
    "generate": dict(d=_gpt2, gp=_gen, prefix=P, ids=[1], n=1, B=2, out=P, logits=None, ws=P, ws_bytes=BIG, stream=None),
    "sample": dict(d=_gpt2, gp=_gen, sp=_samp, prefix=P, ids=[1], n=1, B=2, out=P, logits=None, warped=None,
                   force=None, ws=P, ws_bytes=BIG, stream=None),
    "beam_search": dict(d=_gpt2, bp=_beam, prefix=P, ids=[1], n=1, B=2, out=P, out_len=P, ws=P, ws_bytes=BIG,
                        stream=None),
    "prefill": dict(d=_gpt2, prefix=P, ids=[1], n=1, B=2, rows=6, max_new=8, logits=P, ws=P, ws_bytes=BIG,
                    stream=None),
    "step": dict(d=_gpt2, tokens=P, rows=2, S0=5, max_new=8, pos=5, logits=P, ws=P, ws_bytes=BIG, stream=None),
    "forward_embeds": dict(d=_gpt2, embeds=P, rows=2, n_tok=5, past=0, S0=5, max_new=8, logits=P, ws=P, ws_bytes=BIG,
                           stream=None),
    "reorder": dict(d=_gpt2, src=P, rows=2, S0=5, max_new=8, length=5, ws=P, ws_bytes=BIG, stream=None),
    "score": dict(d=_gpt2, embeds=P, B=2, S=9, mask=None, targets=P, logits=None, logprob=None, loss=None, ws=P,
                  ws_bytes=BIG, stream=None),
    "decode_attention": dict(dtype=N.DT_BF16, q=P, k=P, v=P, pt=P, maxp=4, out=P, M=2, heads=2, S_new=1, past=8,
                             stream=None),
    "vit_encode": dict(d=_vit, pd=None, frames=P, B=1, T=2, enc=P, prefix_out=None, ws=P, ws_bytes=BIG, stream=None),
    "vit_layer_fuses": dict(d=_vit, layer=0),
    "vit_attention_mx": dict(qkv=P, out=P, scales=P, frames=2, tokens=197, heads=4, stream=None),
    "gemm": dict(in_dt=N.DT_BF16, out_dt=N.DT_F32, A=P, lda=128, W=P, ldw=128, C=P, ldc=16, M=4, N=16, K=128, bias=P,
                 act=0, res=None, ldr=0, res_mode=0, G=0, Gs=0, goff=0, roff=0, stream=None),
    "gemm_splitk": dict(in_dt=N.DT_BF16, A=P, lda=384, W=P, ldw=384, C=P, ldc=16, M=4, N=16, K=384, bias=P, G=0, Gs=0,
                        ws=P, ws_bytes=BIG, splits=None, stream=None),
    "frames_preprocess": dict(frames=P, n=2, in_h=16, in_w=16, out_h=8, out_w=8, mean=_MEAN, std=_STD, out=P, out_u8=None,
                              ws=P, ws_bytes=BIG, stream=None),
    "jpeg_decode_batch": dict(data=_ptrs("ok"), lens=_LENS, n=1, out=P, ws=P, ws_bytes=BIG, stream=None),
    "jpeg_probe": dict(data=_JPEG, len=len(_JPEG), w=None, h=None, c=None),
}
SYMBOL = {"decode_attention": "vcap_decode_attention", "vit_encode": "vcap_vit_encode",
          "vit_layer_fuses": "vcap_vit_layer_fuses_qkv_attention", "vit_attention_mx": "vcap_vit_attention_mx",
          "gemm": "vcap_gemm", "gemm_splitk": "vcap_gemm_splitk", "frames_preprocess": "vcap_frames_preprocess",
          "jpeg_decode_batch": "vcap_jpeg_decode_batch", "jpeg_probe": "vcap_jpeg_probe"}

# (entry point, the argument made bad, code, message, new?)   desc=/gp=/bp=/sp= give descriptor fields
ROWS = [
    # the descriptor checks every GPT-2 launch shares
    ("generate", dict(d=None), ARG, "gpt2 desc is null"),
    ("generate", dict(desc=dict(dtype=N.DT_MXFP8)), ARG, "gpt2 dtype"),
    ("generate", dict(desc=dict(n_embd=192)), UNSUP, "gpt2 head_dim must be 64"),
    ("generate", dict(desc=dict(n_embd=192, n_head=3)), UNSUP, "n_embd must be a multiple of 128"),
    ("generate", dict(desc=dict(n_embd=1152, n_head=18)), UNSUP, "n_embd > 1024 (LayerNorm rows are held in registers)"),
    ("generate", dict(desc=dict(wte=None)), ARG, "gpt2 wte / lm_head / wpe / ln_f pointer is null"),
    ("generate", dict(B=0), ARG, "vcap_gpt2_generate: bad arguments"),
    ("generate", dict(gp=dict(max_new_tokens=0)), ARG, "max_new_tokens must be > 0"),
    ("generate", dict(gp=dict(max_new_tokens=65)), UNSUP,
     "max_new_tokens > 64 (the lm_head stages the processors' history in LDS)"),
    ("generate", dict(B=200), UNSUP, "B*(prefix+prompt) exceeds vcap_gpt2_max_rows()"),
    ("generate", dict(gp=dict(max_new_tokens=60)), UNSUP, "context exceeds n_positions"),
    ("generate", dict(ids=[512]), ARG, "prompt id out of range"),
    ("generate", dict(ws_bytes=16), WS, "vcap_gpt2_generate: workspace too small"),
    ("sample", dict(B=0), ARG, "vcap_gpt2_sample: bad arguments"),
    ("sample", dict(sp=dict(top_k=0)), ARG, "vcap_gpt2_sample: needs temperature > 0, 0 < top_p <= 1, top_k >= 1"),
    ("sample", dict(sp=dict(top_k=129)), UNSUP, "vcap_gpt2_sample: top_k <= 128 and vocab <= 51200"),
    ("sample", dict(gp=dict(max_new_tokens=65)), UNSUP, "max_new_tokens must be in 1..64"),
    ("sample", dict(B=200), UNSUP, "B*(prefix+prompt) exceeds vcap_gpt2_max_rows()"),
    ("sample", dict(gp=dict(max_new_tokens=60)), UNSUP, "context exceeds n_positions"),
    ("sample", dict(ids=[512]), ARG, "prompt id out of range"),
    ("sample", dict(ws_bytes=16), WS, "vcap_gpt2_sample: workspace too small"),
    ("sample", dict(desc=dict(prefix_len=0), ids=[], n=0), ARG, "vcap_gpt2_sample: bad arguments", "isnew"),
    ("beam_search", dict(B=0), ARG, "vcap_gpt2_beam_search: bad arguments"),
    ("beam_search", dict(bp=dict(num_beams=9)), UNSUP,
     "vcap_gpt2_beam_search: needs 2 <= num_beams <= 8, B <= 8, max_new <= 64, prefix + prompt + max_new <= 128"),
    ("beam_search", dict(bp=dict(num_beams=8), B=8, ids=[1] * 5, n=5), UNSUP,
     "B*num_beams*(prefix+prompt) exceeds max rows"),
    ("beam_search", dict(desc=dict(prefix_len=0), ids=[], n=0), UNSUP, "B*num_beams*(prefix+prompt) exceeds max rows",
     "isnew"),
    ("beam_search", dict(bp=dict(early_stopping=1)), UNSUP, "only early_stopping=False (the reference's presets)"),
    ("beam_search", dict(bp=dict(max_blocks=-1)), ARG, "vcap_gpt2_beam_search: max_blocks < 0"),
    ("beam_search", dict(desc=dict(vocab=50257), bp=dict(num_beams=8), B=1), UNSUP,
     "num_beams too large for the vocabulary (candidate registers)"),
    ("beam_search", dict(ids=[512]), ARG, "prompt id out of range"),
    ("beam_search", dict(ws_bytes=16), WS, "vcap_gpt2_beam_search: workspace too small"),
    ("prefill", dict(B=0), ARG, "vcap_gpt2_prefill: bad arguments"),
    ("prefill", dict(B=200, rows=200), UNSUP, "B*(prefix+prompt) exceeds vcap_gpt2_max_rows()"),
    ("prefill", dict(ids=[512]), ARG, "prompt id out of range", "isnew"),
    ("step", dict(pos=4), ARG, "vcap_gpt2_step: bad arguments (S0 <= pos < S0 + max_new_tokens)"),
    ("step", dict(rows=0), ARG, "gpt2 step: bad rows / lengths"),
    ("step", dict(ws_bytes=16), WS, "gpt2 step: workspace too small (vcap_gpt2_beam_workspace_bytes)"),
    ("forward_embeds", dict(rows=0), ARG, "vcap_gpt2_forward_embeds: bad arguments"),
    ("forward_embeds", dict(n_tok=3), ARG,
     "vcap_gpt2_forward_embeds: prefill needs n_tok == S0; a step one token at S0 <= past_len < S0 + max_new_tokens"),
    ("forward_embeds", dict(rows=200), UNSUP, "rows*S0 exceeds vcap_gpt2_max_rows() at prefill"),
    ("reorder", dict(length=0), ARG, "vcap_gpt2_reorder: bad arguments"),
    ("score", dict(B=0), ARG, "vcap_gpt2_score: bad arguments"),
    ("score", dict(targets=None), ARG, "vcap_gpt2_score: neither logits_out nor targets given"),
    ("score", dict(targets=None, logits=P, logprob=P), ARG, "vcap_gpt2_score: logprob_out / loss_out need targets"),
    ("score", dict(B=100), UNSUP, "B*S exceeds vcap_gpt2_max_rows()"),
    ("score", dict(S=65), UNSUP, "S exceeds n_positions"),
    ("score", dict(ws_bytes=16), WS, "vcap_gpt2_score: workspace too small (vcap_gpt2_score_workspace_bytes)"),
    ("decode_attention", dict(M=0), ARG, "vcap_decode_attention: bad arguments"),
    ("decode_attention", dict(dtype=N.DT_F16), ARG, "vcap_decode_attention: dtype"),
    ("decode_attention", dict(past=100, maxp=1), ARG, "vcap_decode_attention: context exceeds the page table"),
    ("decode_attention", dict(pt=None, dtype=N.DT_F32), UNSUP,
     "vcap_decode_attention: a NULL page table needs bf16 and context <= 64"),
    ("vit_encode", dict(d=None), ARG, "vit desc is null"),
    ("vit_encode", dict(desc=dict(dtype=7)), ARG, "vit dtype"),
    ("vit_encode", dict(desc=dict(heads=3)), UNSUP, "vit head_dim must be 64"),
    ("vit_encode", dict(desc=dict(kpad=700)), UNSUP, "vit dims must be multiples of the GEMM K step"),
    ("vit_encode", dict(desc=dict(dtype=N.DT_MXFP8, dim=1280, heads=20, mlp=5120)), UNSUP,
     "MXFP8 LayerNorm holds rows of <= 1024 in registers"),
    ("vit_encode", dict(desc=dict(image=230)), ARG, "image not divisible by patch"),
    ("vit_encode", dict(desc=dict(image=288)), UNSUP, "more than 288 tokens"),
    # shapes the encode used to accept and then fail in the middle of (after patchify, the patch GEMM, LayerNorm and
    # the QKV GEMM, or after the whole encoder): a token count the attention dispatcher serves in fp16 only, in
    # f32 (65), bf16 (226) and MXFP8 (50); rows the head / prefix kernels cannot hold
    ("vit_encode", dict(desc=dict(patch=8, image=64)), UNSUP, "vit attention serves 33..192 and 225..256 tokens in fp16 only",
     "isnew"),
    ("vit_encode", dict(desc=dict(dtype=N.DT_BF16, image=240)), UNSUP,
     "vit attention serves 33..192 and 225..256 tokens in fp16 only", "isnew"),
    ("vit_encode", dict(desc=dict(dtype=N.DT_MXFP8, dim=256, heads=4, mlp=1024, patch=32, kpad=3072)), UNSUP,
     "vit attention serves 33..192 and 225..256 tokens in fp16 only", "isnew"),
    ("vit_encode", dict(desc=dict(dim=1280, heads=20, mlp=5120)), UNSUP, "vit dim > 1024 (the head holds a row in LDS)",
     "isnew"),
    ("vit_encode", dict(desc=dict(video_dim=1025)), UNSUP, "video_dim > 1024", "isnew"),
    ("vit_encode", dict(B=0), ARG, "vcap_vit_encode: bad arguments"),
    ("vit_encode", dict(prefix_out=P), ARG, "vcap_vit_encode: prefix desc missing"),
    ("vit_encode", dict(ws_bytes=16), WS, "vcap_vit_encode: workspace too small"),
    ("vit_layer_fuses", dict(layer=2), ARG, "vcap_vit_layer_fuses_qkv_attention: layer out of range"),
    ("vit_attention_mx", dict(frames=0), ARG, "vcap_vit_attention_mx: bad arguments"),
    ("vit_attention_mx", dict(tokens=289), UNSUP, "vcap_vit_attention_mx: tokens > 288"),
    ("vit_attention_mx", dict(heads=3), UNSUP, "vcap_vit_attention_mx: heads*64 must be a multiple of 256"),
    ("vit_attention_mx", dict(tokens=33), UNSUP, "vcap_vit_attention_mx: serves 1..32, 193..224 and 257..288 tokens", "isnew"),
    ("vit_attention_mx", dict(tokens=225), UNSUP, "vcap_vit_attention_mx: serves 1..32, 193..224 and 257..288 tokens", "isnew"),
    ("gemm", dict(A=None), ARG, "vcap_gemm: bad arguments"),
    ("gemm", dict(K=0), ARG, "vcap_gemm: bad arguments"),
    ("gemm", dict(in_dt=N.DT_MXFP8), ARG, "vcap_gemm: operands must be VCAP_DT_F32, VCAP_DT_BF16 or VCAP_DT_F16", "isnew"),
    ("gemm", dict(K=96, lda=96, ldw=96), UNSUP, "vcap_gemm: K must be a multiple of the K step"),
    ("gemm", dict(in_dt=N.DT_F32, K=48), UNSUP, "vcap_gemm: K must be a multiple of the K step"),
    ("gemm", dict(lda=132), UNSUP, "vcap_gemm: A, W 16-byte aligned; lda, ldw in whole 16-byte vectors", "isnew"),
    ("gemm", dict(ldw=129), UNSUP, "vcap_gemm: A, W 16-byte aligned; lda, ldw in whole 16-byte vectors", "isnew"),
    ("gemm", dict(in_dt=N.DT_F32, lda=130), UNSUP, "vcap_gemm: A, W 16-byte aligned; lda, ldw in whole 16-byte vectors",
     "isnew"),
    ("gemm", dict(A=P + 8), UNSUP, "vcap_gemm: A, W 16-byte aligned; lda, ldw in whole 16-byte vectors", "isnew"),
    ("gemm", dict(W=P + 2), UNSUP, "vcap_gemm: A, W 16-byte aligned; lda, ldw in whole 16-byte vectors", "isnew"),
    ("gemm", dict(res_mode=1), ARG, "vcap_gemm: residual pointer missing"),
    ("gemm", dict(res=P, res_mode=2, ldr=16), ARG, "vcap_gemm: row group G must be > 0"),
    ("gemm", dict(G=-1), ARG, "vcap_gemm: row group G must be > 0"),
    ("gemm", dict(out_dt=N.DT_BF16, res=P, res_mode=1, ldr=16), UNSUP, "vcap_gemm: residual needs f32 output"),
    ("gemm", dict(in_dt=N.DT_F16, out_dt=N.DT_BF16), UNSUP, "vcap_gemm: f16 operands write f16 or f32"),
    ("gemm", dict(out_dt=N.DT_F16), UNSUP, "vcap_gemm: bf16 operands write bf16 or f32", "isnew"),
    ("gemm", dict(out_dt=7), UNSUP, "vcap_gemm: bf16 operands write bf16 or f32", "isnew"),
    ("gemm", dict(in_dt=N.DT_F32, out_dt=N.DT_BF16), UNSUP, "vcap_gemm: f32 operands write f32", "isnew"),
    ("gemm", dict(in_dt=N.DT_F16, out_dt=7), UNSUP, "vcap_gemm: f16 operands write f16 or f32"),
    ("gemm_splitk", dict(bias=None), ARG, "vcap_gemm_splitk: bad arguments"),
    ("gemm_splitk", dict(G=4, Gs=3), ARG, "vcap_gemm_splitk: bad arguments"),
    ("gemm_splitk", dict(in_dt=N.DT_F32), ARG, "vcap_gemm_splitk: operands must be VCAP_DT_BF16 or VCAP_DT_F16"),
    ("gemm_splitk", dict(K=100), UNSUP, "vcap_gemm_splitk: K must be a multiple of 64"),
    ("gemm_splitk", dict(lda=388), UNSUP, "vcap_gemm_splitk: A, W 16-byte aligned; lda, ldw in whole 16-byte vectors",
     "isnew"),
    ("gemm_splitk", dict(W=P + 4), UNSUP, "vcap_gemm_splitk: A, W 16-byte aligned; lda, ldw in whole 16-byte vectors",
     "isnew"),
    ("gemm_splitk", dict(N=18, ldc=18), UNSUP,
     "vcap_gemm_splitk: N, ldc in whole 16-byte vectors; C and workspace 16-byte aligned"),
    ("gemm_splitk", dict(C=P + 4), UNSUP,
     "vcap_gemm_splitk: N, ldc in whole 16-byte vectors; C and workspace 16-byte aligned"),
    ("gemm_splitk", dict(ws_bytes=8 * 4 * 16 * 4 - 4), WS, "vcap_gemm_splitk: workspace < 8*M*N*4 bytes"),
    ("frames_preprocess", dict(frames=None), ARG, "vcap_frames_preprocess: bad arguments"),
    ("frames_preprocess", dict(mean=None), ARG, "vcap_frames_preprocess: bad arguments"),
    ("frames_preprocess", dict(std=None), ARG, "vcap_frames_preprocess: bad arguments"),
    ("frames_preprocess", dict(out=None), ARG, "vcap_frames_preprocess: bad arguments"),       # neither output
    ("frames_preprocess", dict(ws=None), ARG, "vcap_frames_preprocess: bad arguments", "isnew"),
    ("frames_preprocess", dict(n=0), ARG, "vcap_frames_preprocess: bad arguments"),
    ("frames_preprocess", dict(n=-1), ARG, "vcap_frames_preprocess: bad arguments"),
    ("frames_preprocess", dict(out_w=0), ARG, "vcap_frames_preprocess: bad arguments"),
    # the downscale cap: 31 * 8 = 248 is served (tests/test_gpu_preprocess.py), 249 is not, on either axis
    ("frames_preprocess", dict(in_w=249), UNSUP, "vcap_frames_preprocess: downscale factor above 31"),
    ("frames_preprocess", dict(in_h=249), UNSUP, "vcap_frames_preprocess: downscale factor above 31"),
    ("frames_preprocess", dict(in_w=32, out_w=1), UNSUP, "vcap_frames_preprocess: downscale factor above 31"),
    ("frames_preprocess", dict(ws_bytes=255), WS, "vcap_frames_preprocess: workspace too small"),
    ("jpeg_decode_batch", dict(data=None), ARG, "vcap_jpeg_decode_batch: bad arguments"),
    ("jpeg_decode_batch", dict(lens=None), ARG, "vcap_jpeg_decode_batch: bad arguments"),
    ("jpeg_decode_batch", dict(n=0), ARG, "vcap_jpeg_decode_batch: bad arguments"),
    ("jpeg_decode_batch", dict(out=None), ARG, "vcap_jpeg_decode_batch: bad arguments"),
    ("jpeg_decode_batch", dict(ws=None), ARG, "vcap_jpeg_decode_batch: bad arguments"),
    ("jpeg_decode_batch", dict(lens=_NOLEN), ARG, "vcap_jpeg_decode_batch: empty image buffer"),
    ("jpeg_decode_batch", dict(data=_NULL_IMAGE), ARG, "vcap_jpeg_decode_batch: empty image buffer"),
    ("jpeg_decode_batch", dict(ws_bytes=255), WS, "vcap_jpeg_decode_batch: workspace too small"),
    ("jpeg_decode_batch", dict(data=_SHORT, lens=_SHORT_LENS), ARG,
     "vcap_jpeg_decode_batch: image 0: corrupt JPEG: SOS length", "isnew"),
    ("jpeg_probe", dict(data=None), ARG, "vcap_jpeg_probe: bad arguments"),
    ("jpeg_probe", dict(len=0), ARG, "vcap_jpeg_probe: bad arguments"),
]


def _call(entry, bad):
    args, keep = dict(GOOD[entry]), []
    bad = dict(bad)
    for key, fields in (("d", "desc"), ("gp", "gp"), ("bp", "bp"), ("sp", "sp")):
        if callable(args.get(key)):
            args[key] = args[key](**bad.pop(fields, {}))
    args.update(bad)
    out = []
    for k, v in args.items():
        if isinstance(v, C.Structure):
            keep.append(v)
            v = C.byref(v)
        elif k == "ids":
            v = (C.c_int * max(len(v), 1))(*v)
            keep.append(v)
        out.append(v)
    fn = getattr(N.lib(), SYMBOL.get(entry, "vcap_gpt2_" + entry))
    return int(fn(*out)), N.lib().vcap_last_error().decode()


def _ptr(v):
    """An address inside _BUF as "ptr" / "ptr+offset": a test id must not carry a process address."""
    if isinstance(v, int) and not isinstance(v, bool) and P < v < P + 4096:
        return f"ptr+{v - P}"
    return _NAMED.get(id(v), v)


def _id(row):
    entry, bad = row[0], row[1]
    parts = [f"{k}={'+'.join(f'{a}={b}' for a, b in v.items()) if isinstance(v, dict) else _ptr(v)}"
             for k, v in bad.items()]
    return "-".join([entry] + parts + list(row[4:])).replace(str(P), "ptr")


@pytest.mark.parametrize("row", ROWS, ids=_id)
def test_refused_before_any_launch(row):
    entry, bad, code, text = row[:4]
    assert _call(entry, bad) == (code, text)


def test_every_listed_entry_point_has_rows():
    assert {r[0] for r in ROWS} == set(GOOD)


# One descriptor, four queries: the sizes recorded from the library before the carving was shared
# (csrc/runtime_gpt2.hip carve_dec / carve_step / carve_beam / carve_score).  The argmax partials are
# sized for max(..., CU count, 256): 256 is both the no-GPU fallback and what an MI355X reports.
@pytest.mark.parametrize("name, args, expected", [
    ("vcap_gpt2_workspace_bytes", (2, 5, 8), 145152),
    ("vcap_gpt2_beam_workspace_bytes", (6, 5, 8), 497408),
    ("vcap_gpt2_beam_search_workspace_bytes", (2, 3, 5, 8), 415488),
    ("vcap_gpt2_score_workspace_bytes", (2, 9), 217856),
])
def test_workspace_queries_are_pinned(name, args, expected):
    got = int(getattr(N.lib(), name)(C.byref(_gpt2()), *args))
    assert got == expected and got % 256 == 0


@pytest.mark.parametrize("dtype, fields, served", [
    (N.DT_F16, dict(patch=8, image=64), True),                 # 65 tokens: the generic kernel, fp16 only
    (N.DT_F32, dict(patch=8, image=64), False),
    (N.DT_BF16, dict(patch=8, image=64, kpad=192), False),
    (N.DT_BF16, dict(image=240), False),                       # 226 tokens
    (N.DT_F32, dict(patch=8, image=32), True),                 # 17 tokens: a window of every dtype
    (N.DT_F32, dict(dim=1280, heads=20, mlp=5120), False),
    (N.DT_F32, dict(video_dim=1025), False),
    (N.DT_F32, dict(video_dim=1024), True),
])
def test_vit_workspace_query_is_zero_exactly_where_the_encode_refuses(dtype, fields, served):
    desc = _vit(dtype=dtype, **fields)
    assert (int(N.lib().vcap_vit_workspace_bytes(C.byref(desc), 2, 3)) > 0) == served
    assert (int(N.lib().vcap_vit_layer_fuses_qkv_attention(C.byref(desc), 0)) >= 0) == served


def test_frames_and_jpeg_workspace_queries_are_zero_for_bad_arguments():
    lib = N.lib()
    assert lib.vcap_frames_workspace_bytes(2, 16, 16, 8, 8) > 0
    for bad in [(0, 16, 16, 8, 8), (-1, 16, 16, 8, 8), (2, 0, 16, 8, 8), (2, 16, 16, 8, 0)]:
        assert lib.vcap_frames_workspace_bytes(*bad) == 0
    assert lib.vcap_jpeg_workspace_bytes(_JPEG, len(_JPEG), 2) > lib.vcap_jpeg_workspace_bytes(_JPEG, len(_JPEG), 1) > 0
    for bad in [(None, len(_JPEG), 1), (_JPEG, 0, 1), (_JPEG, len(_JPEG), 0), (_JPEG, len(_JPEG), -3),
                (_SHORT_SOS, len(_SHORT_SOS), 1)]:
        assert lib.vcap_jpeg_workspace_bytes(*bad) == 0
