"""Golden fixtures of the teacher-forced entry points, by the REFERENCE's own code: runs
GPT2TextDecoder.forward and VideoCaptionModel.compute_loss (called unbound on a namespace holding
encoder / proj / decoder) on seeded weights and writes tests/golden/score_*.npz|json.

Like make_goldens.py (whose stubs and reference builder it imports) it runs only where the reference
tree is available (VCAP_REFERENCE); the tests read the fixtures alone.

  score_tiny  vit_tiny_test + gpt2_tiny_test, B = 3, 12 tokens: right padding of different lengths, one
              interior masked token, some labels -100 -> full logits, loss, and compute_loss of a
              caption_ids batch that starts with BOS (= EOS = pad: compute_loss hides it)
  score_gpt2  gpt2 (E = 768, V = 50257), B = 2, 10 tokens, seeded video embeddings -> top-64 logits per
              position (topk_pack), per-position target log-prob, loss
"""
from __future__ import annotations

import json
import sys
from pathlib import Path
from types import SimpleNamespace

sys.dont_write_bytecode = True
sys.path.insert(0, str(Path(__file__).resolve().parent))

import make_goldens as G  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vcap import configs, prng, weights  # noqa: E402

OUT = Path(__file__).resolve().parent


def _meta(vit, gpt2, wseed, sd, **kw):
    return dict({"vit": vit, "gpt2": gpt2, "weights_seed": wseed, "weights_sha256": G.weights_digest(sd),
                 "transformers": G.transformers.__version__, "torch": torch.__version__}, **kw)


def tiny_case():
    from src.models.caption_model import VideoCaptionModel
    vit, gpt2, wseed, fseed, B, T, L = "vit_tiny_test", "gpt2_tiny_test", 4, 9, 3, 2, 12
    va, ga = configs.vit_arch(vit), configs.gpt2_arch(gpt2)
    sd = weights.synthetic_state_dict(wseed, va, ga)
    enc, dec = G.build_reference(sd, va, ga)
    video = torch.from_numpy(prng.imagenet_frames(fseed, (B, T, 3, va.image, va.image)))
    pad = ga.eos_token_id
    g = torch.Generator().manual_seed(77)
    input_ids = torch.randint(0, ga.vocab - 1, (B, L), generator=g)
    attention_mask = torch.ones(B, L, dtype=torch.long)
    lengths = [L, L - 3, 5]
    for b, n in enumerate(lengths):
        input_ids[b, n:] = pad
        attention_mask[b, n:] = 0
    attention_mask[0, 6] = 0                       # an interior token hidden from every later query
    labels = input_ids.clone()
    labels[attention_mask == 0] = -100
    labels[1, 2] = labels[2, 0] = -100             # and two visible positions that are not scored
    # compute_loss: <bos> tokens <eos> pad..., bos = eos = pad
    caption_ids = torch.full((B, L), pad, dtype=torch.long)
    caption_ids[:, 0] = ga.bos_token_id
    for b, n in enumerate([10, 7, 3]):
        caption_ids[b, 1:1 + n] = torch.randint(0, ga.vocab - 1, (n,), generator=g)
    with torch.no_grad():
        emb = enc(video)
        out = dec(emb, input_ids, attention_mask, labels)
        out_default = dec(emb, input_ids, None, labels)   # attention_mask = input_ids != pad
        model = SimpleNamespace(encoder=enc, proj=nn.Identity(), decoder=dec)
        closs = VideoCaptionModel.compute_loss(model, video, caption_ids, pad)
    arrays = {"video_emb": emb.numpy(), "input_ids": input_ids.numpy().astype(np.int32),
              "attention_mask": attention_mask.numpy().astype(np.uint8), "labels": labels.numpy().astype(np.int32),
              "logits": out["logits"].numpy(), "caption_ids": caption_ids.numpy().astype(np.int32)}
    meta = _meta(vit, gpt2, wseed, sd, B=B, T=T, frames_seed=fseed, pad_id=int(pad), loss=float(out["loss"]),
                 loss_default_mask=float(out_default["loss"]), compute_loss=float(closs))
    np.savez_compressed(OUT / "score_tiny.npz", **arrays)
    (OUT / "score_tiny.json").write_text(json.dumps(meta, indent=1, sort_keys=True))
    print("score_tiny", out["logits"].shape, meta["loss"], meta["loss_default_mask"], meta["compute_loss"])


def gpt2_case():
    vit, gpt2, wseed, B, L = "vit_tiny_test", "gpt2", 1, 2, 10   # the ViT is not run: seeded embeddings
    va, ga = configs.vit_arch(vit), configs.gpt2_arch(gpt2)
    sd = weights.synthetic_state_dict(wseed, va, ga)
    _, dec = G.build_reference(sd, va, ga)
    g = torch.Generator().manual_seed(123)
    emb = torch.randn(B, configs.VIDEO_DIM, generator=g)
    input_ids = torch.randint(0, ga.vocab - 1, (B, L), generator=g)
    input_ids[:, 0] = 50255                        # a target in the vocabulary's last, 81-column tile
    attention_mask = torch.ones(B, L, dtype=torch.long)
    input_ids[1, 7:] = ga.eos_token_id
    attention_mask[1, 7:] = 0
    labels = input_ids.clone()
    labels[attention_mask == 0] = -100
    with torch.no_grad():
        out = dec(emb, input_ids, attention_mask, labels)
    logits = out["logits"]
    P = dec.prefix_len
    ext = torch.cat([torch.full((B, P), -100, dtype=torch.long), labels], dim=1)
    tgt = torch.cat([ext[:, 1:], torch.full((B, 1), -100, dtype=torch.long)], dim=1)
    lp = F.log_softmax(logits.double(), dim=-1).gather(2, tgt.clamp(min=0)[..., None])[..., 0]
    lp = torch.where(tgt >= 0, lp, torch.zeros_like(lp))
    arrays = {"video_emb": emb.numpy(), "input_ids": input_ids.numpy().astype(np.int32),
              "attention_mask": attention_mask.numpy().astype(np.uint8), "labels": labels.numpy().astype(np.int32),
              "targets": tgt.numpy().astype(np.int32), "target_logprob": lp.numpy()}
    arrays.update({"logits_" + k: v for k, v in G.topk_pack(logits).items()})
    meta = _meta(vit, gpt2, wseed, sd, B=B, loss=float(out["loss"]))
    np.savez_compressed(OUT / "score_gpt2.npz", **arrays)
    (OUT / "score_gpt2.json").write_text(json.dumps(meta, indent=1, sort_keys=True))
    print("score_gpt2", logits.shape, meta["loss"])


def main():
    G.install_stubs(configs.VITS)
    sys.path.insert(0, str(G.REF))
    which = sys.argv[1:] or ["tiny", "gpt2"]
    if "tiny" in which:
        tiny_case()
    if "gpt2" in which:
        gpt2_case()


if __name__ == "__main__":
    main()
