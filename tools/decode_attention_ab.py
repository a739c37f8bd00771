"""Bit identity of the decode attention paths between two builds of the library.

  python tools/decode_attention_ab.py run <out.npz>            (library: VCAP_LIB, one process per library)
  python tools/decode_attention_ab.py compare <a.npz> <b.npz> [--write-exclude x.json] [--exclude x.json]

`run` builds a small synthetic decoder (E 128, 2 layers, 2 heads, vocab 1000, 128 positions: the shapes
tests/beam_cases.py uses), zeroes the decoder's workspace before every search and records, per search,
the ids, the lengths and the WHOLE workspace afterwards.  Nothing in the ABI returns an attention
output, but layer 1's K/V at a position are computed from layer 0's attention output at that position,
so equal workspaces mean equal attention outputs at every step, not merely equal tokens.
  beam  bf16 / fp32 x beams 2 / 4 x (S0 = 5, L = 24: the <= 64 ancestry kernel) and (S0 = 64, L = 64:
        the general ancestry kernel), B = 3 - lowered where B * beams * S0 would exceed
        vcap_gpt2_max_rows() (beams 4 at S0 = 64 runs B = 2)
  greedy bf16 / fp32, S0 = 5 (contiguous <= 64 kernel) and S0 = 68 (page-table kernel at every step,
        prefill included), 24 new tokens, B = 3
`compare` is byte for byte.  --write-exclude stores the byte ranges that differ (two runs of the SAME
library: what is not reproducible to begin with); --exclude leaves exactly those ranges out."""
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "video-caption-algorithm_amd"))

E, VOCAB, NPOS, NLAYER, PREFIX_LEN, B0 = 128, 1000, 128, 2, 4, 3


def prompt(n):
    return [VOCAB - 1] + [(37 * i + 11) % (VOCAB - 1) for i in range(n - 1)]


def run(out_path):
    import ctypes as C

    import torch
    from vcap import _native as N
    from vcap import search, weights
    from vcap.configs import GPT2Arch
    from vcap.model import GenConfig, HipGPT2Decoder

    dev = torch.device("cuda:0")
    ar = GPT2Arch("attn_ab", E, NLAYER, E // 64, vocab=VOCAB, n_positions=NPOS, bos_token_id=VOCAB - 1,
                  eos_token_id=VOCAB - 1)
    sd = weights.synthetic_gpt2(5, ar)
    max_rows = int(N.lib().vcap_gpt2_max_rows())
    res = {}
    for prec in ("bf16", "fp32"):
        dec = HipGPT2Decoder(sd, ar, prec, dev)
        desc = C.byref(dec.desc)
        pre3 = 0.1 * torch.randn(B0, PREFIX_LEN, E, generator=torch.Generator().manual_seed(77)).to(dev)

        def record(tag, nbytes, fn):
            dec.ws.buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)   # a fresh buffer: nothing cached
            ids, lens = fn()
            torch.cuda.synchronize()
            res[f"{tag}/ids"] = ids.cpu().numpy()
            res[f"{tag}/lens"] = lens.cpu().numpy()
            res[f"{tag}/ws"] = dec.ws.buf.cpu().numpy()
            print(f"{tag}: B={ids.shape[0]} ws={nbytes} ids[0][:8]={ids[0][:8].tolist()}", flush=True)

        for nb in (2, 4):
            for S0, L in ((5, 24), (64, 64)):
                B = min(B0, max_rows // (nb * S0))
                ids = prompt(S0 - PREFIX_LEN)
                nbytes = int(N.lib().vcap_gpt2_beam_search_workspace_bytes(desc, B, nb, S0, L))
                assert nbytes > 0, (nb, S0, L)

                def beam():
                    search.beam_search_device(dec, pre3[:B], ids, num_beams=nb, max_new_tokens=L, min_new_tokens=8,
                                              no_repeat_ngram_size=3, repetition_penalty=1.1, eos=VOCAB - 1)
                    _, out, lens = dec._beam_bufs[(B, nb, L)]
                    return out, lens
                record(f"beam/{prec}/nb{nb}/S0_{S0}", nbytes, beam)
        for S0 in (5, 68):
            ids = prompt(S0 - PREFIX_LEN)
            cfg = GenConfig(24, 8, 3, 1.1, VOCAB - 1, VOCAB - 1, True)

            def greedy():
                out = torch.empty(B0, 24, dtype=torch.int32, device=dev)
                dec.generate_ids(pre3, ids, cfg, out=out)
                return out, torch.full((B0,), 24, dtype=torch.int32)
            record(f"greedy/{prec}/S0_{S0}", dec.workspace_bytes(B0, len(ids), 24), greedy)
    np.savez_compressed(out_path, **res)
    print(f"{os.environ.get('VCAP_LIB', 'the package library')} -> {out_path}: {len(res)} arrays")


def ranges(mask):
    """[start, end) runs of True in a 1-D bool array."""
    edges = np.flatnonzero(np.diff(np.concatenate(([0], mask.view(np.int8), [0]))))
    return [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]


def compare(a_path, b_path, write_excl=None, excl=None):
    a, b = np.load(a_path), np.load(b_path)
    skip = json.load(open(excl)) if excl else {}
    found, bad = {}, 0
    if sorted(a.files) != sorted(b.files):
        sys.exit(f"different arrays: {sorted(set(a.files) ^ set(b.files))}")
    for k in a.files:
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype:
            print(f"DIFF {k}: shape / dtype {x.shape} {x.dtype} vs {y.shape} {y.dtype}")
            bad += 1
            continue
        d = np.ascontiguousarray(x).view(np.uint8).reshape(-1) != np.ascontiguousarray(y).view(np.uint8).reshape(-1)
        for s, e in skip.get(k, []):
            d[s:e] = False
        r = ranges(d)
        nskip = sum(e - s for s, e in skip.get(k, []))
        if r:
            found[k] = r
            bad += 1
            print(f"DIFF {k}: {int(d.sum())} of {d.size} bytes in {len(r)} ranges, first {r[:4]}")
        else:
            print(f"same {k}: {d.size} bytes" + (f" ({nskip} excluded)" if nskip else ""))
    if write_excl:
        json.dump(found, open(write_excl, "w"))
        print(f"ranges that differ -> {write_excl}")
    print("IDENTICAL" if not bad else f"{bad} arrays differ")
    return bad


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        opt = dict(zip(sys.argv[4::2], sys.argv[5::2]))
        bad = compare(sys.argv[2], sys.argv[3], opt.get("--write-exclude"), opt.get("--exclude"))
        sys.exit(0 if not bad or "--write-exclude" in opt else 1)
    else:
        sys.exit(__doc__)
