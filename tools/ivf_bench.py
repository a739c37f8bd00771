"""IVF-Flat search cost against the flat search: IVFFlatIPIndex.search and FlatIPIndex.search over the same
vectors, D = 256 unit rows drawn around random unit centres (so the lists are uneven), n in {1 M, 8 M},
nlist in {1024, 4096}, nprobe in {1, 8, 32}, nq in {1, 16, 64}, k in {5, 100}, f32 and bf16 storage.

Per cell, timed in one process after a warm-up with device events around `reps` back-to-back calls,
interleaved ABAB over the rounds, medians reported; `reps` is set per cell and per line from one timed
pair of calls so that every window lasts at least WINDOW_MS.  The repetitions of a window use the same
queries, so they probe the same lists: where the probed rows fit the caches (small nprobe * nq * n / nlist;
the probed bytes are the floor column times 6.0 TB/s) the ivf times, the ivf / flat ratios and the
"ivf/floor" column are WARM-CACHE figures against a floor priced at the HBM rate, while the flat scan's
gigabytes never fit.  A first query against cold lists was not measured.
  ivf     one IVFFlatIPIndex.search call (coarse search + list scan + merge; the index's own workspace)
  flat    one FlatIPIndex.search call on the same vectors (the code that exists without the IVF index)
  coarse  the coarse stage alone (vcap_ip_search over the centroids with k = nprobe)
  recall  |ivf ids & flat ids| / k, mean over the queries
  floor   (the bytes of the probed lists' rows + the centroid table) / 6.0 TB/s
and per index the median / maximum list length and the wall-clock time (host plumbing and synchronisation
included) of train (niter 10) and add.

    python tools/ivf_bench.py --out profiles/ivf_bench.txt
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "video-caption-algorithm_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vcap import retrieval as R  # noqa: E402

HBM_SWEEP_BYTES_S = 6.0e12
DIM = 256
NS = (1_000_000, 8_000_000)
NLISTS = (1024, 4096)
NPROBES = (1, 8, 32)
NQS = (1, 16, 64)
KS = (5, 100)
CENTRES = 3000
WINDOW_MS = 4.0          # least duration of one timed window
MAX_REPS = 400


def clustered_rows(n, dim, dev, seed, centres):
    """Unit rows: a random centre plus noise of about the centre's own length."""
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty(n, dim, device=dev)
    for s in range(0, n, 1 << 20):
        m = min(1 << 20, n - s)
        pick = torch.randint(0, centres.shape[0], (m,), generator=g, device=dev)
        blk = centres[pick] + torch.randn(m, dim, generator=g, device=dev) / dim ** 0.5
        out[s:s + m] = blk / blk.norm(dim=1, keepdim=True)
    return out


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ns", default=",".join(map(str, NS)))
    ap.add_argument("--nlists", default=",".join(map(str, NLISTS)))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")

    emit(f"# {torch.cuda.get_device_name(0)}; D = {DIM}; unit rows around {CENTRES} random unit centres; medians of "
         f"{args.rounds} interleaved rounds of windows >= {WINDOW_MS:.0f} ms; floor = probed bytes / "
         f"{HBM_SWEEP_BYTES_S / 1e12:.1f} TB/s; one box, one run")
    emit("# a window repeats the same queries, so small probed sets are cache-resident: ivf ms, ivf/flat and ivf/floor are "
         "warm-cache figures there; train / add are wall clock with the host plumbing (train: the host's permutation of n "
         "indices where it subsamples), and the first index of the run also pays first-call costs")
    g = torch.Generator(device=dev).manual_seed(1)
    centres = torch.nn.functional.normalize(torch.randn(CENTRES, DIM, generator=g, device=dev), dim=1)
    cells = {}
    for n in map(int, args.ns.split(",")):
        base = clustered_rows(n, DIM, dev, n, centres)
        queries = clustered_rows(max(NQS), DIM, dev, 7, centres)
        for storage in ("f32", "bf16"):
            flat = R.FlatIPIndex(DIM, storage, dev)
            flat.add(base)
            for nlist in map(int, args.nlists.split(",")):
                ivf = R.IVFFlatIPIndex(DIM, nlist, storage, dev)
                t_train = wall_s(lambda: ivf.train(base, niter=10))
                t_add = wall_s(lambda: ivf.add(base))
                sizes = ivf.list_sizes()
                emit(f"# index {storage} n={n} nlist={nlist}: train {t_train:.3f} s (niter 10, {min(n, 256 * nlist)} rows), "
                     f"add {t_add:.3f} s; list length median {int(np.median(sizes))} max {int(sizes.max())} "
                     f"empty {int((sizes == 0).sum())}; objective {ivf.train_objective[0]:.4f} -> {ivf.train_objective[-1]:.4f}")
                emit(f"# {'storage':7} {'n':>8} {'nlist':>5} {'nprobe':>6} {'nq':>3} {'k':>4} {'ivf ms':>8} {'flat ms':>8} "
                     f"{'ivf/flat':>8} {'coarse ms':>9} {'recall':>6} {'floor ms':>9} {'ivf/floor':>9}")
                esz = 4 if storage == "f32" else 2
                for nprobe in NPROBES:
                    ivf.nprobe = nprobe
                    for nq in NQS:
                        q = queries[:nq].contiguous()
                        probed = ivf.probe_lists(q).cpu().numpy()
                        rows = int(sizes[probed[probed >= 0]].sum())
                        floor = (rows * DIM * esz + nlist * DIM * 4) / HBM_SWEEP_BYTES_S * 1e3
                        for k in KS:
                            def run_ivf():
                                return ivf.search(q, k)

                            def run_flat():
                                return flat.search(q, k)

                            def run_coarse():
                                return R.ip_search(ivf.centroids, nlist, q, nprobe)

                            Ii, If = run_ivf()[1], run_flat()[1]
                            hit = (Ii[:, :, None] == If[:, None, :]).any(2).float().sum(1) / k
                            fns = {"ivf": run_ivf, "flat": run_flat, "coarse": run_coarse}
                            reps = {}
                            for key, fn in fns.items():     # warm up, then size the window from a timed pair
                                event_ms(fn, 2)
                                reps[key] = max(3, min(MAX_REPS, int(WINDOW_MS / max(event_ms(fn, 2), 1e-3)) + 1))
                            t = {"ivf": [], "flat": [], "coarse": []}
                            for _ in range(args.rounds):
                                for key, fn in fns.items():
                                    t[key].append(event_ms(fn, reps[key]))
                            a, b, c = (statistics.median(t[key]) for key in ("ivf", "flat", "coarse"))
                            cells[(storage, n, nlist, nprobe, nq, k)] = a / b
                            emit(f"  {storage:7} {n:8d} {nlist:5d} {nprobe:6d} {nq:3d} {k:4d} {a:8.4f} {b:8.4f} {a / b:8.3f} "
                                 f"{c:9.4f} {float(hit.mean()):6.3f} {floor:9.5f} {a / floor:9.1f}")
                del ivf
                torch.cuda.empty_cache()
            del flat
        del base
        torch.cuda.empty_cache()
    slow = [f"{st} n={n} nlist={nl} nprobe={p} nq={nq} k={k} ({r:.2f}x)" for (st, n, nl, p, nq, k), r in cells.items()
            if r > 0.98]
    emit(f"# cells where the IVF search is not faster than the flat search by more than the 2 % box spread: "
         f"{len(slow)} of {len(cells)}")
    for s in slow:
        emit(f"  {s}")


if __name__ == "__main__":
    main()
