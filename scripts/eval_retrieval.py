"""Recall@1 / Recall@5 / MRR of clip-to-index retrieval over an annotations file (the reference's
scripts/eval_retrieval.py): each record's clip is embedded, normalised with the reference's l2norm and
searched; its gold id is its video_id's position in meta.json.

    python -m scripts.eval_retrieval --annotations val.json --index index_dir
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

from scripts import _common as common

KS = (1, 5)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--annotations", required=True)
    ap.add_argument("--index", required=True, help="index directory written by scripts.build_index")
    ap.add_argument("--meta", default="", help="meta.json (default: <index>/meta.json)")
    ap.add_argument("--nprobe", type=int, default=0, help="lists an IVF_FLAT index scans (0: the saved value)")
    common.add_model_args(ap)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    import torch
    from vcap.retrieval import SCRIPT_L2NORM_EPS, l2_normalize, retrieval_metrics
    idx_dir = Path(args.index)
    meta = json.loads((Path(args.meta) if args.meta else idx_dir / "meta.json").read_text("utf-8"))
    id_list = [m["video_id"] for m in meta]
    index = common.load_index_for_query(idx_dir, args)
    emb = common.load_embedder(args)
    queries, gold = [], []
    for rec in common.read_annotations(args.annotations):
        queries.append(l2_normalize(common.embed_frames_dir(emb, rec["frames_dir"], args), SCRIPT_L2NORM_EPS, 1))
        gold.append(id_list.index(rec["video_id"]) if rec["video_id"] in id_list else -2)   # -2: never returned
    if not queries:
        print("[WARN] no samples")
        return None
    _, I = index.search(torch.cat(queries), max(KS))
    m = retrieval_metrics(I.cpu().numpy(), gold, KS)
    print(f"[VAL] N={m['n']}")
    for k in KS:
        print(f"Recall@{k}: {m[f'recall@{k}']:.3f}")
    print(f"MRR: {m['mrr']:.3f}")
    return m


if __name__ == "__main__":
    main()
