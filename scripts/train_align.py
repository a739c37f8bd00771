"""Train the text/video alignment model on the device path - the reference's src/cli/train_full.py --model vit
--freeze_vit with its flag names.  The frozen ViT runs on the HIP kernels once per clip; vid_proj is a torch
nn.Linear; the whole text tower (txt_emb, txt_enc.layers.*, txt_proj) runs forward and backward on the HIP
kernels (vcap_text_encode_backward, vcap/train_align.py) and is updated by torch's AdamW on
CosineEmbeddingLoss(encode_video, encode_text, +1).

Each clip's feature - the frame mean of the ViT's CLS output, before vid_proj - is computed ONCE, without
gradients; training runs on the cached [vid_dim] features.  Annotations are the reference's annotations.json
records {"video_id", "frames_dir", "captions": [...]}; a record may carry "caption_ids": [[id, ...], ...]
instead of text (no BPE vocabulary ships with the project: pass --tokenizer_dir <dir with vocab.json,
merges.txt> to tokenise "captions").  Captions are truncated to --max_len (at most 64) and right-padded
with the pad id.

Writes <run_dir>/events.csv ("step,loss" per step) and val.csv ("step,val_loss"), and the best checkpoint
{"model_state": vit.* + vid_proj.* + txt_*, "step", "epoch", "best_val", "args"} to <ckpt_dir>/<ckpt_name>,
which scripts/query_text.py and scripts/query_video.py load.

Not supported, refused up front: a run without --freeze_vit (no ViT weight gradients exist on the device)
and --model simple.  Unlike the reference's .train(), the device text tower applies no dropout.

  python -m scripts.train_align --model vit --freeze_vit --ann_train train/annotations.json \\
      --ann_val val/annotations.json --weights_seed 1 --epochs 1
"""
from __future__ import annotations

import argparse
import random
import sys
from pathlib import Path

from scripts._common import read_annotations


def build_argparser():
    p = argparse.ArgumentParser("Train the alignment model (frozen ViT; vid_proj in torch; text tower on the HIP path)")
    p.add_argument("--model", choices=["simple", "vit"], default="vit")
    p.add_argument("--vit_name", default="vit_base_patch16_224")
    p.add_argument("--freeze_vit", action="store_true", default=False)
    p.add_argument("--ann_train", default="./data/processed/msvd/train/annotations.json")
    p.add_argument("--ann_val", default="./data/processed/msvd/val/annotations.json")
    p.add_argument("--batch_size", type=int, default=2)
    p.add_argument("--num_frame", type=int, default=8)
    p.add_argument("--image_size", type=int, default=224)
    p.add_argument("--max_len", type=int, default=32)
    p.add_argument("--epochs", type=int, default=2)
    p.add_argument("--max_steps", type=int, default=0, help="> 0: stop after this many steps")
    p.add_argument("--lr", type=float, default=5e-4)
    p.add_argument("--device", default="cuda")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--run_dir", default="runs/align")
    p.add_argument("--ckpt_dir", default="checkpoints")
    p.add_argument("--ckpt_name", default="msvd_vitalign_best.pt")
    p.add_argument("--val_every", type=int, default=50)
    # this project's additions
    p.add_argument("--ckpt", "--checkpoint", dest="ckpt", default="", help="alignment checkpoint to start from")
    p.add_argument("--weights_seed", type=int, default=None, help="seeded random-init weights when no --ckpt")
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32", "fp8"], help="the frozen ViT's")
    p.add_argument("--text_dtype", default="f32", choices=["f32", "bf16"], help="the text tower's operand dtype")
    p.add_argument("--tokenizer_dir", default="", help="vocab.json + merges.txt for annotations with text captions")
    p.add_argument("--vocab_size", type=int, default=50257)
    p.add_argument("--pad_id", type=int, default=None, help="default: the tokenizer's pad id")
    p.add_argument("--txt_dim", type=int, default=512)
    p.add_argument("--txt_layers", type=int, default=2)
    p.add_argument("--txt_nhead", type=int, default=8)
    p.add_argument("--proj_dim", type=int, default=256)
    return p


def check_args(args) -> None:
    """The refusals, before anything is imported or loaded."""
    if args.model != "vit":
        raise SystemExit("[ERROR] --model simple is not supported: only ViTTextAlignModel (--model vit) is on the "
                         "device path")
    if not args.freeze_vit:
        raise SystemExit("[ERROR] training without --freeze_vit is not supported: the device path has no ViT weight "
                         "gradients (vid_proj and the text tower train)")
    if not 1 <= args.max_len <= 64:
        raise SystemExit("[ERROR] --max_len must be in 1..64: the device text tower takes at most 64 ids")


def caption_rows(anns, tokenizer, max_len: int):
    """[(clip index, [ids...])] - one row per caption, truncated to max_len (no bos / eos, as the reference's
    dataset tokenises for the alignment model)."""
    rows = []
    for i, a in enumerate(anns):
        caps = a.get("caption_ids")
        if caps is None:
            caps = [tokenizer.encode_prompt(c) for c in a.get("captions", []) if c]
        for ids in caps:
            body = [int(t) for t in ids][:max_len]
            if body:
                rows.append((i, body))
    return rows


def batches(rows, feats, batch_size: int, pad_id: int, shuffle: bool, rng: random.Random):
    import torch
    order = list(range(len(rows)))
    if shuffle:
        rng.shuffle(order)
    for b0 in range(0, len(order), batch_size):
        pick = [rows[j] for j in order[b0:b0 + batch_size]]
        width = max(len(ids) for _, ids in pick)
        caps = torch.full((len(pick), width), pad_id, dtype=torch.long)
        for r, (_, ids) in enumerate(pick):
            caps[r, :len(ids)] = torch.tensor(ids, dtype=torch.long)
        yield feats[[i for i, _ in pick]], caps


def main(argv=None) -> int:
    args = build_argparser().parse_args(argv)
    check_args(args)
    import numpy as np
    import torch
    from core.preprocessing.frame_loader import load_video_tensor
    from vcap import configs
    from vcap.model import HipViTEncoder
    from vcap.retrieval import HipTextEmbedder, remap_alignment_state_dict
    from vcap.tokenizer import load_tokenizer
    from vcap.train_align import AlignTrainer, clip_features, synthetic_align_state_dict
    from vcap.weights import synthetic_vit

    random.seed(args.seed)
    torch.manual_seed(args.seed)
    rng = random.Random(args.seed)
    run_dir, ckpt_dir = Path(args.run_dir), Path(args.ckpt_dir)
    run_dir.mkdir(parents=True, exist_ok=True)
    ckpt_dir.mkdir(parents=True, exist_ok=True)

    tok = load_tokenizer(args.tokenizer_dir)
    pad_id = int(tok.pad_token_id if args.pad_id is None else args.pad_id)
    arch = configs.vit_arch(args.vit_name)
    seed = 1 if args.weights_seed is None else int(args.weights_seed)
    # the frozen ViT with an identity encoder.proj: its output is the clip feature vid_proj reads
    vit_sd = synthetic_vit(seed, arch, video_dim=arch.dim)
    align_sd = synthetic_align_state_dict(seed, arch.dim, args.vocab_size, pad_id, args.txt_dim, args.txt_layers,
                                          args.txt_nhead, args.proj_dim)
    vit_ckpt = {}
    if args.ckpt:
        state = torch.load(args.ckpt, map_location="cpu", weights_only=True)
        state = state.get("model_state", state)
        vit_ckpt = {k: v for k, v in state.items() if k.startswith("vit.")}
        remapped = remap_alignment_state_dict(state)
        vit_sd = {k: remapped.get(k, v) for k, v in vit_sd.items()}
        for k in align_sd:
            if k in state:
                align_sd[k] = np.ascontiguousarray(torch.as_tensor(state[k]).float().numpy())
    vit_sd["encoder.proj.weight"] = np.eye(arch.dim, dtype=np.float32)
    vit_sd["encoder.proj.bias"] = np.zeros(arch.dim, np.float32)
    encoder = HipViTEncoder(vit_sd, arch, args.precision, args.device, arch.dim)
    text = HipTextEmbedder.from_state_dict(align_sd, pad_id, args.txt_nhead, args.text_dtype, args.device)

    train_anns, val_anns = read_annotations(args.ann_train), read_annotations(args.ann_val)
    train_rows, val_rows = caption_rows(train_anns, tok, args.max_len), caption_rows(val_anns, tok, args.max_len)
    if not train_rows:
        raise SystemExit(f"[ERROR] {args.ann_train}: no captions")
    print(f"[data] {len(train_anns)} train clips / {len(train_rows)} captions, {len(val_anns)} val clips / "
          f"{len(val_rows)} captions; running the frozen ViT once per clip")

    def features(anns):
        out = [clip_features(encoder, load_video_tensor(str(a["frames_dir"]), args.num_frame, args.image_size,
                                                        args.device)) for a in anns]
        return torch.cat(out, dim=0) if out else torch.zeros(0, arch.dim, device=args.device)

    train_feat, val_feat = features(train_anns), features(val_anns)
    trainer = AlignTrainer(text, align_sd, lr=args.lr)
    n = sum(p.numel() for p in trainer.params) + sum(p.numel() for p in trainer.vid_proj.parameters())
    print(f"[trainable] vid_proj + text tower | params={n:,} | lr={args.lr}")

    def validate() -> float:
        total, k = 0.0, 0
        for feat, caps in batches(val_rows, val_feat, args.batch_size, pad_id, False, rng):
            total += trainer.evaluate(feat, caps)
            k += 1
            if k >= 50:
                break
        return total / max(k, 1)

    def save(step: int, epoch: int, best: float) -> None:
        state = {k: torch.as_tensor(v).clone() for k, v in vit_ckpt.items()}
        if not state:   # seeded ViT: under the alignment model's names
            state = {"vit." + k[len("encoder.backbone."):]: torch.from_numpy(v).clone() for k, v in vit_sd.items()
                     if k.startswith("encoder.backbone.")}
        state.update(trainer.state_dict())
        path = ckpt_dir / args.ckpt_name
        torch.save({"model_state": state, "step": step, "epoch": epoch, "best_val": best, "args": vars(args)}, path)
        print(f"[ckpt] saved best -> {path} (val={best:.4f})")

    best, step, done = float("inf"), 0, False
    for epoch in range(args.epochs):
        for feat, caps in batches(train_rows, train_feat, args.batch_size, pad_id, True, rng):
            loss = trainer.step(feat, caps)
            step += 1
            if step == 1 or step % 10 == 0:
                print(f"[train] step {step:05d} | loss {loss:.4f}")
            with open(run_dir / "events.csv", "a", encoding="utf-8") as f:
                f.write(f"{step},{loss:.6f}\n")
            if args.val_every > 0 and step % args.val_every == 0 and val_rows:
                v = validate()
                print(f"[val]   step {step:05d} | val_loss {v:.4f}")
                with open(run_dir / "val.csv", "a", encoding="utf-8") as f:
                    f.write(f"{step},{v:.6f}\n")
                if v < best:
                    best = v
                    save(step, epoch, best)
            if args.max_steps > 0 and step >= args.max_steps:
                done = True
                break
        v = validate() if val_rows else float(loss)
        print(f"[val][epoch end] epoch {epoch} | val_loss {v:.4f}")
        with open(run_dir / "val.csv", "a", encoding="utf-8") as f:
            f.write(f"{step},{v:.6f}\n")
        if v < best:
            best = v
            save(step, epoch, best)
        if done:
            break
    print("[OK] alignment training finished.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
