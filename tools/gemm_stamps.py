"""Per-workgroup timeline of the 256x256 ViT GEMM from the stamp build (tools/build_stamps.py; run with
VCAP_LIB=<stamp library>): one launch of each shape at M rows (default 50432, 16 videos), bf16 operands,
then per workgroup the prologue (entry -> first K-tile landed), the K loop, the epilogue issue (K loop
done -> last store issued), the drain (-> loads and stores complete) and, per CU, the gap between one
workgroup's last store issue and the next workgroup's entry.  Units: microseconds (100 MHz clock).
usage: gemm_stamps.py [M] [shape ...]   shapes: qkv proj fc1 fc2 (default proj fc2)"""
import ctypes as C
import sys
from collections import defaultdict
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "video-caption-algorithm_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from vcap import _native as N  # noqa: E402

args = sys.argv[1:]
M = int(args.pop(0)) if args and args[0].isdigit() else 50432
SHAPES = {"qkv": (2304, 768, False, 0), "proj": (768, 768, True, 0), "fc1": (3072, 768, False, 1),
          "fc2": (768, 3072, True, 0)}
dev = torch.device("cuda:0")
s = torch.cuda.current_stream().cuda_stream
g = torch.Generator(device=dev).manual_seed(0)
lib = N.lib()
lib.vcap_diag_stamps_g256.restype = C.c_int
lib.vcap_diag_stamps_g256.argtypes = [C.c_void_p, C.c_int]
assert lib.vcap_set_gemm_policy(2) == 0


def rnd(*shape, scale=1.0, dtype=torch.bfloat16):
    return (torch.rand(*shape, generator=g, device=dev) * 2 - 1).mul_(scale).to(dtype)


q = lambda a: f"{np.median(a):6.2f} (p90 {np.percentile(a, 90):6.2f})"
for name in args or ["proj", "fc2"]:
    n, k, f32, act = SHAPES[name]
    A, W, b = rnd(M, k), rnd(n, k, scale=0.05), rnd(n, scale=0.1, dtype=torch.float32)
    Cc = torch.zeros(M, n, device=dev, dtype=torch.float32 if f32 else torch.bfloat16)

    def launch():
        N.check(lib.vcap_gemm(N.DT_BF16, N.DT_F32 if f32 else N.DT_BF16, A.data_ptr(), k, W.data_ptr(), k, Cc.data_ptr(),
                              n, M, n, k, b.data_ptr(), act, Cc.data_ptr() if f32 else None, n if f32 else 0,
                              1 if f32 else 0, 0, 0, 0, 0, s), name)

    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    lib.vcap_diag_stamps_g256(None, 0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    torch.cuda.synchronize()
    buf = np.zeros((1 << 18, 8), dtype=np.uint64)
    cnt = lib.vcap_diag_stamps_g256(buf.ctypes.data, buf.shape[0])
    r = buf[:cnt].astype(np.int64)
    t = r[:, 2:7] / 100.0
    t -= t[:, 0].min()
    hw, xcc = r[:, 7] & 0xFFFFFFFF, (r[:, 7] >> 32) & 0xF
    unit = xcc * 1000 + ((hw >> 13) & 7) * 100 + ((hw >> 12) & 1) * 10 + ((hw >> 8) & 0xF)
    per = defaultdict(list)
    for i in range(cnt):
        per[int(unit[i])].append(t[i])
    gap_issue, gap_done = [], []
    for rows in per.values():
        rows.sort(key=lambda x: x[0])
        for a_, b_ in zip(rows, rows[1:]):
            gap_issue.append(b_[0] - a_[3])
            gap_done.append(b_[0] - a_[4])
    print(f"== {name} M={M} N={n} K={k}: {cnt} tiles on {len(per)} CUs, event {e0.elapsed_time(e1) * 1e3:.1f} us, "
          f"stamp span {t[:, 4].max():.1f} us (last entry {t[:, 0].max():.1f}, last K-loop end {t[:, 2].max():.1f})")
    print(f"   per WG median: prologue {q(t[:, 1] - t[:, 0])}  K loop {q(t[:, 2] - t[:, 1])}  "
          f"epilogue issue {q(t[:, 3] - t[:, 2])}  drain {q(t[:, 4] - t[:, 3])}  total {q(t[:, 4] - t[:, 0])}")
    if gap_issue:
        print(f"   gap to the next workgroup on the CU: after the last store issue {q(np.array(gap_issue))}, "
              f"after the drain {q(np.array(gap_done))}", flush=True)
