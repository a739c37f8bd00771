"""Build an index with captions in its meta (the reference's scripts/build_index_with_captions.py): every
annotation record's frames_dir is embedded online (encode_video), normalised with the reference's l2norm,
and added to a Flat or IVF_FLAT inner-product index; meta.json = [{"video_id", "caption"}] carries each
record's first caption.  The index directory holds what FlatIPIndex / IVFFlatIPIndex.save write; the FAISS
binary file (video.index) is not reproduced.

    python -m scripts.build_index_with_captions --ann_path annotations.json --out_dir index \
        --ckpt align.pt --num_frame 8 --image_size 224 --index_type IVF_FLAT --nlist 50
"""
from __future__ import annotations

import argparse
from pathlib import Path

from scripts import _common as common


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ann_path", required=True, help="annotations.json: [{video_id, frames_dir, captions}]")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--ckpt", default="", help="caption-model or alignment-model checkpoint")
    ap.add_argument("--num_frame", type=int, default=8)
    ap.add_argument("--image_size", type=int, default=224)
    common.add_index_type_args(ap)
    ap.add_argument("--weights_seed", type=int, default=None, help="seeded random-init weights when no --ckpt")
    ap.add_argument("--vit_name", default="vit_base_patch16_224")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp32", "fp8"])
    ap.add_argument("--storage", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    args.num_frames = args.num_frame          # the name _common's helpers read
    return args


def caption_of(rec) -> str:
    """load_caption_map of the reference: the first of "captions", else the "caption" string, else ""."""
    if isinstance(rec.get("captions"), list) and rec["captions"]:
        return rec["captions"][0]
    return rec["caption"] if isinstance(rec.get("caption"), str) else ""


def main(argv=None) -> int:
    args = parse(argv)
    import torch
    from vcap.retrieval import SCRIPT_L2NORM_EPS, l2_normalize
    out_dir = Path(args.out_dir)
    print(f"[INFO] out_dir={out_dir}")
    print(f"[INFO] ann_path={args.ann_path}")
    emb = common.load_embedder(args)
    embs, metas = [], []
    for rec in common.read_annotations(args.ann_path):
        if not rec.get("video_id"):
            continue
        embs.append(common.embed_frames_dir(emb, rec["frames_dir"], args))
        metas.append({"video_id": rec["video_id"], "caption": caption_of(rec)})
    if not embs:
        raise SystemExit(f"[ERROR] no records in {args.ann_path}")
    feats = l2_normalize(torch.cat(embs), SCRIPT_L2NORM_EPS, 1)
    if args.index_type == "IVF_FLAT" and len(metas) < args.nlist:
        raise SystemExit(f"[ERROR] IVF_FLAT with --nlist {args.nlist} needs at least that many clips, got {len(metas)}")
    index = common.build_index_from(feats, args, normalize=False)
    index.metadata = metas
    index.save(out_dir)
    print(f"[OK] index -> {out_dir / 'vectors.npy'}")
    print(f"[OK] meta  -> {out_dir / 'meta.json'}")
    print(f"[OK] num vectors: {len(metas)} | dim: {feats.shape[1]} | type={args.index_type}")
    return len(metas)


if __name__ == "__main__":
    main()
