"""Flat inner-product index over extracted features (the reference's scripts/build_index.py): the
<video_id>.npy rows of the annotation records that have one, L2-normalised on add (faiss.normalize_L2),
with meta.json = [{"video_id", "caption"}] carrying each record's first caption.  The index directory
holds vectors.npy + index.json + meta.json; the FAISS binary format is not reproduced.  --index_type IVF_FLAT
--nlist N (the flags of the reference's scripts/build_index_with_captions.py) builds an IVFFlatIPIndex instead.

    python -m scripts.build_index --features features --annotations ann.json --out_dir index
"""
from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np

from scripts import _common as common


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--features", required=True)
    ap.add_argument("--annotations", required=True)
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--storage", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--device", default="cuda")
    common.add_index_type_args(ap)
    return ap.parse_args(argv)


def main(argv=None) -> int:
    args = parse(argv)
    from vcap.retrieval import first_caption
    feats, metas = [], []
    for rec in common.read_annotations(args.annotations):
        fpath = Path(args.features) / f"{rec['video_id']}.npy"
        if not fpath.exists():
            continue
        feats.append(np.load(fpath))
        metas.append({"video_id": rec["video_id"], "caption": first_caption(rec)})
    if not feats:
        raise SystemExit(f"[ERROR] no features of {args.annotations} under {args.features}")
    feats = np.stack(feats).astype("float32")
    kind = "flat-IP" if args.index_type == "Flat" else f"IVF-flat-IP (nlist={args.nlist})"
    print(f"[INFO] Building {kind} index with {len(feats)} vectors, dim={feats.shape[1]}")
    index = common.build_index_from(feats, args, normalize=True)
    index.metadata = metas
    index.save(args.out_dir)
    print(f"[OK] index -> {Path(args.out_dir) / 'vectors.npy'}")
    print(f"[OK] meta  -> {Path(args.out_dir) / 'meta.json'}")
    print(f"[OK] num vectors: {len(feats)} dim={feats.shape[1]}")
    return len(feats)


if __name__ == "__main__":
    main()
