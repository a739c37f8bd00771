"""Flat inner-product search cost: vcap_ip_search (vcap.retrieval.ip_search) on unit rows of D = 256 for
N in {2 000, 100 000, 1 000 000, 8 000 000}, nq in {1, 16, 64}, k in {5, 100}, f32 and bf16 storage.

Two lines per shape, timed in one process after a warm-up with device events around `reps` back-to-back
calls, interleaved ABAB over the rounds, medians reported:
  ours   one vcap_ip_search call (scan + merge kernels, caller-owned workspace)
  torch  torch.topk(q @ db.T, k) on the same tensors (bf16 storage: the queries cast to bf16 for the matmul,
         the scores cast back to f32) - the stand-in for FAISS-GPU, which is not installed
and the HBM floor n * dim * bytes / 6.0 TB/s (the measured in-order sweep rate of the chip).  Also printed:
whether the two id sets agree on f32 storage, and per (storage, n, k) the time at nq = 16 over the time at
nq = 1 - the database is read once per call, so that ratio stays near 1 where the scan is HBM-bound.

    python tools/retrieval_bench.py --out profiles/retrieval_bench.txt
"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "video-caption-algorithm_amd"))
import torch  # noqa: E402

from vcap import retrieval as R  # noqa: E402

HBM_SWEEP_BYTES_S = 6.0e12
DIM = 256
NS = (2_000, 100_000, 1_000_000, 8_000_000)
NQS = (1, 16, 64)
KS = (5, 100)


def unit_rows(n, dim, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty(n, dim, device=dev)
    for s in range(0, n, 1 << 20):
        blk = torch.randn(min(1 << 20, n - s), dim, generator=g, device=dev)
        out[s:s + blk.shape[0]] = blk / blk.norm(dim=1, keepdim=True)
    return out


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--ns", default=",".join(map(str, NS)))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# {torch.cuda.get_device_name(0)}; D = {DIM}; medians of {args.rounds} interleaved rounds; floor = "
         f"n * D * bytes / {HBM_SWEEP_BYTES_S / 1e12:.1f} TB/s; one box, one run")
    emit(f"# {'storage':7} {'n':>9} {'nq':>3} {'k':>4} {'ours ms':>9} {'torch ms':>9} {'ours/torch':>10} "
         f"{'floor ms':>9} {'ours/floor':>10}  ids")
    ours_ms, vs_torch = {}, {}
    for n in map(int, args.ns.split(",")):
        base = unit_rows(n, DIM, dev, n)
        for storage in ("f32", "bf16"):
            db = base if storage == "f32" else base.to(torch.bfloat16)
            floor = n * DIM * db.element_size() / HBM_SWEEP_BYTES_S * 1e3
            reps = 20 if n <= 100_000 else 4 if n <= 1_000_000 else 2
            for nq in NQS:
                q = unit_rows(nq, DIM, dev, 7)
                qs = q if storage == "f32" else q.to(torch.bfloat16)
                for k in KS:
                    ws = torch.empty(int(R.N.lib().vcap_ip_search_workspace_bytes(n, DIM, nq, k)), dtype=torch.uint8,
                                     device=dev)

                    def ours():
                        return R.ip_search(db, n, q, k, ws)

                    def ref():
                        return torch.topk((qs @ db.T).float(), k)

                    same = "-"
                    if storage == "f32":
                        same = "equal" if torch.equal(ours()[1], ref()[1]) else "differ"
                    for fn in (ours, ref):
                        event_ms(fn, 2)
                    t = {"ours": [], "torch": []}
                    for _ in range(args.rounds):
                        t["ours"].append(event_ms(ours, reps))
                        t["torch"].append(event_ms(ref, reps))
                    o, r = statistics.median(t["ours"]), statistics.median(t["torch"])
                    ours_ms[(storage, n, nq, k)] = o
                    vs_torch[(storage, n, nq, k)] = o / r
                    emit(f"  {storage:7} {n:9d} {nq:3d} {k:4d} {o:9.4f} {r:9.4f} {o / r:10.2f} {floor:9.4f} "
                         f"{o / floor:10.2f}  {same}")
                    del ws
            if storage == "bf16":
                del db
        del base
        torch.cuda.empty_cache()
    slower = [f"{st} n={n} nq={nq} k={k} ({r:.2f}x)" for (st, n, nq, k), r in vs_torch.items() if r > 1.02]
    emit(f"# slower than torch.topk(q @ db.T) by more than the 2 % box spread: {len(slower)} of {len(vs_torch)} shapes")
    for s in slower:
        emit(f"  {s}")
    emit("# time at nq = 16 over time at nq = 1 (the database is read once per call)")
    for (storage, n, nq, k), o in ours_ms.items():
        if nq == 16:
            emit(f"  {storage:7} {n:9d} k={k:3d}  {o / ours_ms[(storage, n, 1, k)]:.2f}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
