"""What the ragged-prompt decode costs and saves, parent commit against this tree, in ONE GPU call.

  tools/ragged_bench.sh prepare | run        (exports the parent tree and builds its library; then runs this)
  python tools/ragged_bench.py <parent-tree> [--rounds 3] [--out profiles/ragged_prompts.txt]

`<parent-tree>` is a checkout of the parent commit with its own libvcap_hip.so built (tools/build_ref_lib.sh).
Every measurement is a fresh child process of `worker` in one of the two trees, parent and new alternating,
`--rounds` times; a process reports the p50 of its device-synchronised, warmed-up repetitions, and the
figure written is the median of the rounds' p50s with their min .. max as the spread of repeated
identical runs.
  1. infer    InferenceEngine.infer_video, default config (S1 / S2 precise beam 3, S3 natural; the two default
              prompts as pre-tokenised ids of their lengths, 9 and 7: no BPE vocab is needed), ViT-B/16 + GPT-2
              synthetic weights, 16 frames, one video: parent (3 decodes) against new (S1 + S2 merged).
  2. ragged   new tree only: one ragged greedy decode of 8 rows with 4 distinct prompts against the sum of
              the 4 uniform 2-row calls it replaces, bf16 and fp32 (GPT-2 small, 24 new tokens, hipGraph).
  3. bench    the `bench.py --gpus 1` default line's captions/s, parent against new (uniform kernels only).
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PROMPTS = ([50256], [50256, 464, 1388, 2223], [50256] + list(range(1000, 1010)), [50256] + list(range(2000, 2019)))


def _p50(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def worker(tree: str, what: str):
    tree = Path(tree).resolve()
    sys.path[:0] = [str(tree / "video-caption-algorithm_amd"), str(tree)]
    import torch
    dev = torch.device("cuda:0")
    if what == "infer":
        from core.config import InferenceConfig
        from core.engine import InferenceEngine
        eng = InferenceEngine(InferenceConfig(num_frames=16, weights_seed=1, device="cuda:0", prompt2="ids:9012 262 1388 2223 287 530 1790 6827 25",
                                              prompt3="ids:16594 257 1790 11 3288 8305 25"))
        video = torch.randn(1, 16, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(dev)
        print(json.dumps({"infer_ms": _p50(lambda: eng.infer_video(video), 5, 30)}))
        return
    from vcap import configs, weights
    from vcap.model import GenConfig, HipGPT2Decoder
    ga = configs.gpt2_arch("gpt2")
    sd = weights.synthetic_gpt2(1, ga)
    out = {}
    for prec in ("bf16", "fp32"):
        dec = HipGPT2Decoder(sd, ga, prec, dev)
        cfg = GenConfig(24, 8, 3, 1.1, ga.eos_token_id, ga.eos_token_id, True)
        pre = 0.1 * torch.randn(8, 4, ga.n_embd, generator=torch.Generator().manual_seed(5)).to(dev)
        rows = [PROMPTS[b // 2] for b in range(8)]
        buf8 = torch.empty(8, 24, dtype=torch.int32, device=dev)
        buf2 = [torch.empty(2, 24, dtype=torch.int32, device=dev) for _ in range(4)]
        pre2 = [pre[2 * k:2 * k + 2].contiguous() for k in range(4)]

        def ragged():
            dec.generate_ids(pre, rows, cfg, out=buf8)

        def uniform4():
            for k in range(4):
                dec.generate_ids(pre2[k], PROMPTS[k], cfg, out=buf2[k])
        out[prec] = {"ragged_ms": _p50(ragged, 5, 30), "uniform4_ms": _p50(uniform4, 5, 30)}
        torch.cuda.synchronize()
        assert torch.equal(buf8, torch.cat(buf2)), "ragged rows differ from the uniform calls'"
    print(json.dumps(out))


def _child(tree, what):
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "ragged_bench.py"), "worker", str(tree), what],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f"worker {tree} {what} failed (rc {r.returncode}):\n{r.stderr[-3000:]}")
    print(f"{Path(tree).name} {what}: {r.stdout.strip().splitlines()[-1]}", flush=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def _bench(tree):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=str(tree),
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f"bench.py in {tree} failed (rc {r.returncode}):\n{r.stderr[-3000:]}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln][-1]
    print(f"{Path(tree).name} bench.py: {json.loads(line)['value']:.3f} captions/s", flush=True)
    return float(json.loads(line)["value"])


def _fmt(xs, unit):
    return f"{statistics.median(xs):.3f} {unit} (min {min(xs):.3f} .. max {max(xs):.3f}, {len(xs)} runs)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench-rounds", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ragged_prompts.txt"))
    a = ap.parse_args()
    parent = Path(a.parent).resolve()
    infer = {"parent": [], "new": []}
    rag = {p: {"ragged_ms": [], "uniform4_ms": []} for p in ("bf16", "fp32")}
    bench = {"parent": [], "new": []}
    for _ in range(a.rounds):
        infer["parent"].append(_child(parent, "infer")["infer_ms"])
        infer["new"].append(_child(ROOT, "infer")["infer_ms"])
        r = _child(ROOT, "ragged")
        for p in rag:
            for k in rag[p]:
                rag[p][k].append(r[p][k])
    for _ in range(a.bench_rounds):
        bench["parent"].append(_bench(parent))
        bench["new"].append(_bench(ROOT))
    med = statistics.median
    lines = ["ragged prompts: parent commit against this tree, one GPU call, parent and new alternating in fresh",
             "processes; each run = p50 of 30 device-synchronised repetitions after 5 warm-ups (bench.py: its own",
             "--steps 20 --warmup 5); figure = median of the runs' p50s with their min .. max (tools/ragged_bench.py)",
             "",
             "1. infer_video, default config, ViT-B/16 + GPT-2 synthetic weights, 16 frames, one video (fp32 decoder)",
             f"   parent (3 decodes)      {_fmt(infer['parent'], 'ms')}",
             f"   new (S1 + S2 merged)    {_fmt(infer['new'], 'ms')}",
             f"   new / parent            {med(infer['new']) / med(infer['parent']):.3f}",
             "",
             "2. greedy decode, GPT-2 small, 24 new tokens, hipGraph: 8 rows with 4 distinct prompts (1 / 4 / 11 / 20 ids)",
             "   in one ragged call against the 4 uniform 2-row calls it replaces (ids checked equal)"]
    for p in ("bf16", "fp32"):
        lines += [f"   {p} ragged (1 call)     {_fmt(rag[p]['ragged_ms'], 'ms')}",
                  f"   {p} uniform (4 calls)   {_fmt(rag[p]['uniform4_ms'], 'ms')}",
                  f"   {p} ragged / uniform    {med(rag[p]['ragged_ms']) / med(rag[p]['uniform4_ms']):.3f}"]
    lines += ["",
              "3. bench.py --gpus 1 --steps 20 --warmup 5 (uniform kernels only), captions/s",
              f"   parent                  {_fmt(bench['parent'], 'captions/s')}",
              f"   new                     {_fmt(bench['new'], 'captions/s')}",
              f"   new / parent            {med(bench['new']) / med(bench['parent']):.3f}", ""]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "worker":
        worker(sys.argv[2], sys.argv[3])
    else:
        main()
