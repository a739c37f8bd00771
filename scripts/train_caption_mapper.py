"""Fine-tune decoder.mapper on the device path - the reference's src/cli/train_caption_mapper.py with its flag
names.  The ViT is frozen; it and GPT-2 run on the HIP kernels; the mapper (0.79 M parameters) is a torch
nn.Linear trained with AdamW on the teacher-forced LM loss, its gradient coming from
vcap_gpt2_score_backward (vcap/train.py).  --unfreeze_gpt2_last N also trains every parameter of the last N
GPT-2 blocks, in a second AdamW group at --lr_gpt2, their gradients coming from
vcap_gpt2_score_backward_tail; the device weights are refreshed in place after every step.

Each clip is embedded ONCE with the frozen device encoder, without gradients; training runs on the cached
[video_dim] embeddings.  Annotations are the reference's annotations.json records
{"video_id", "frames_dir", "captions": [...]}; a record may carry "caption_ids": [[id, ...], ...] instead
of text (no BPE vocabulary ships with the project: pass --tokenizer_dir <dir with vocab.json, merges.txt> to
tokenise "captions").  Every caption becomes <bos> ids <eos>, truncated to --max_len and right-padded with
the pad id (= eos).

Writes <run_dir>/events.csv ("step,loss" per step) and val.csv ("step,val_loss"), and the best checkpoint
{"model_state": full state dict with the trained decoder.mapper.0.* (and the trained
decoder.model.transformer.h.{i}.* of an unfrozen tail), "step", "epoch", "best_val", "args"}
to <ckpt_dir>/<ckpt_name>, which load_caption_model(backend="hip") loads.

Not supported, refused up front: --cond_mode bos (the device decoder conditions on a prefix only).  Unlike
the reference's .train() on the whole model, the device GPT-2 applies no dropout noise, in the unfrozen
blocks either; the mapper's own dropout stays.

  python -m scripts.train_caption_mapper --ann_train train/annotations.json --ann_val val/annotations.json \\
      --weights_seed 1 --epochs 1
"""
from __future__ import annotations

import argparse
import random
import sys
from pathlib import Path

from scripts._common import read_annotations


def build_argparser():
    p = argparse.ArgumentParser("Fine-tune the caption model's mapper (frozen ViT and GPT-2 on the HIP path)")
    p.add_argument("--ann_train", default="./data/processed/msvd/train/annotations.json")
    p.add_argument("--ann_val", default="./data/processed/msvd/val/annotations.json")
    p.add_argument("--batch_size", type=int, default=8)
    p.add_argument("--num_frame", type=int, default=8)
    p.add_argument("--image_size", type=int, default=224)
    p.add_argument("--max_len", type=int, default=48)
    p.add_argument("--vit_name", default="vit_base_patch16_224")
    p.add_argument("--gpt2_name", default="gpt2")
    p.add_argument("--cond_mode", choices=["prefix", "bos"], default="prefix")
    p.add_argument("--prefix_len", type=int, default=4)
    p.add_argument("--unfreeze_gpt2_last", type=int, default=0, help="also train the last N GPT-2 blocks")
    p.add_argument("--lr_gpt2", type=float, default=1e-5, help="learning rate of the unfrozen GPT-2 blocks")
    p.add_argument("--epochs", type=int, default=1)
    p.add_argument("--lr", type=float, default=3e-4)
    p.add_argument("--device", default="cuda")
    p.add_argument("--seed", type=int, default=123)
    p.add_argument("--val_every", type=int, default=20)
    p.add_argument("--run_dir", default="runs/mapper_ft")
    p.add_argument("--ckpt_dir", default="checkpoints")
    p.add_argument("--ckpt_name", default="msvd_mapper_finetune.pt")
    # this project's additions
    p.add_argument("--ckpt", "--checkpoint", dest="ckpt", default="", help="checkpoint to start from")
    p.add_argument("--weights_seed", type=int, default=None, help="seeded random-init weights when no --ckpt")
    p.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32", "fp8"], help="the frozen ViT's")
    p.add_argument("--decoder_precision", default="auto", choices=["auto", "fp32", "bf16"])
    p.add_argument("--tokenizer_dir", default="", help="vocab.json + merges.txt for annotations with text captions")
    p.add_argument("--dropout", type=float, default=0.1, help="the mapper's own dropout")
    return p


def caption_rows(anns, tokenizer, max_len: int):
    """[(clip index, [bos, ids..., eos])] - one row per caption, truncated to max_len."""
    bos, eos = tokenizer.bos_token_id, tokenizer.eos_token_id
    rows = []
    for i, a in enumerate(anns):
        caps = a.get("caption_ids")
        if caps is None:
            caps = [tokenizer.encode_prompt(c) for c in a.get("captions", []) if c]
        for ids in caps:
            body = [int(t) for t in ids][: max(max_len - 2, 0)]
            rows.append((i, [bos] + body + [eos]))
    return rows


def embed_clips(model, anns, args):
    """[n_clips, video_dim] f32 on the device: proj(encoder(video)) of every clip, no gradient."""
    import torch
    from core.preprocessing.frame_loader import load_video_tensor
    out = []
    with torch.no_grad():
        for a in anns:
            video = load_video_tensor(str(a["frames_dir"]), args.num_frame, args.image_size, args.device)
            out.append(model.proj(model.encoder(video)).reshape(1, -1).float())
    return torch.cat(out, dim=0)


def batches(rows, emb, batch_size: int, pad_id: int, shuffle: bool, rng: random.Random):
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
        yield emb[[i for i, _ in pick]], caps


def main(argv=None) -> int:
    args = build_argparser().parse_args(argv)
    if args.unfreeze_gpt2_last < 0:
        raise SystemExit("[ERROR] --unfreeze_gpt2_last must be >= 0")
    if args.cond_mode != "prefix":
        raise SystemExit("[ERROR] --cond_mode bos is not supported: the device decoder conditions on a prefix only")
    import torch
    from vcap.caption import HipVideoCaptionModel, build_state_dict
    from vcap.train import MapperTrainer

    random.seed(args.seed)
    torch.manual_seed(args.seed)
    rng = random.Random(args.seed)
    run_dir, ckpt_dir = Path(args.run_dir), Path(args.ckpt_dir)
    run_dir.mkdir(parents=True, exist_ok=True)
    ckpt_dir.mkdir(parents=True, exist_ok=True)

    sd = build_state_dict(args.ckpt, args.vit_name, args.gpt2_name, args.weights_seed, args.prefix_len)
    model = HipVideoCaptionModel(sd, args.vit_name, args.gpt2_name, args.prefix_len, args.precision, args.device,
                                 args.tokenizer_dir, decoder_precision=args.decoder_precision)
    tok = model.decoder.tokenizer
    train_anns, val_anns = read_annotations(args.ann_train), read_annotations(args.ann_val)
    train_rows = caption_rows(train_anns, tok, args.max_len)
    val_rows = caption_rows(val_anns, tok, args.max_len)
    if not train_rows:
        raise SystemExit(f"[ERROR] {args.ann_train}: no captions")
    print(f"[data] {len(train_anns)} train clips / {len(train_rows)} captions, {len(val_anns)} val clips / "
          f"{len(val_rows)} captions; embedding the clips once")
    train_emb, val_emb = embed_clips(model, train_anns, args), embed_clips(model, val_anns, args)

    n_layer = model.decoder.hip.arch.n_layer
    if args.unfreeze_gpt2_last > n_layer:
        raise SystemExit(f"[ERROR] --unfreeze_gpt2_last {args.unfreeze_gpt2_last} exceeds the model's {n_layer} blocks")
    trainer = MapperTrainer(model, sd, pad_id=tok.pad_token_id, lr=args.lr, dropout=args.dropout,
                            unfreeze_gpt2_last=args.unfreeze_gpt2_last, lr_gpt2=args.lr_gpt2)
    n = sum(p.numel() for p in trainer.mapper.parameters())
    print(f"[trainable] decoder.mapper | params={n:,} | lr={args.lr}; grad copies "
          f"{model.decoder.hip.grad_bytes / 2 ** 20:.0f} MiB")
    if trainer.tail:
        n_tail = sum(p.numel() for p in trainer.tail.values())
        print(f"[trainable] gpt2_tail | params={n_tail:,} | lr={args.lr_gpt2}")

    def validate() -> float:
        total, k = 0.0, 0
        for emb, caps in batches(val_rows, val_emb, args.batch_size, tok.pad_token_id, False, rng):
            total += trainer.evaluate(emb, caps)
            k += 1
            if k >= 50:
                break
        return total / max(k, 1)

    def save(step: int, epoch: int, best: float) -> None:
        state = {k: torch.as_tensor(v).clone() for k, v in sd.items()}
        state.update(trainer.state_dict())
        path = ckpt_dir / args.ckpt_name
        torch.save({"model_state": state, "step": step, "epoch": epoch, "best_val": best, "args": vars(args)}, path)
        print(f"[ckpt] saved best -> {path} (val={best:.4f})")

    best, step = float("inf"), 0
    for epoch in range(args.epochs):
        for emb, caps in batches(train_rows, train_emb, args.batch_size, tok.pad_token_id, True, rng):
            loss = trainer.step(emb, caps)
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
        v = validate() if val_rows else float(loss)
        print(f"[val][epoch end] epoch {epoch} | val_loss {v:.4f}")
        with open(run_dir / "val.csv", "a", encoding="utf-8") as f:
            f.write(f"{step},{v:.6f}\n")
        if v < best:
            best = v
            save(step, epoch, best)
    trainer.load_mapper()
    print("[OK] mapper fine-tuning finished.")
    return 0


if __name__ == "__main__":
    sys.exit(main())
