"""profiles/vit_grad_accuracy.txt from the figures tests/test_gpu_vit_grad.py prints before it asserts:

    python -m pytest tests/test_gpu_vit_grad.py -q -s > vit_grad_tests.txt
    python tools/vit_grad_accuracy.py vit_grad_tests.txt profiles/vit_grad_accuracy.txt

Per case, dtype and tensor the largest err / bound over the n_tail runs, the worst ratio per case and dtype,
and for vcap_vit_attention_backward alone the largest ratio per dtype, token count and output over the heads
and frame counts of the sweep."""
import collections
import re
import sys

src, dst = sys.argv[1], sys.argv[2]
rows = collections.OrderedDict()
attn = collections.OrderedDict()
for line in open(src):
    for m in re.finditer(r"VIT_GRAD (f32|bf16) (G\d) n_tail=(\d) (\S+) err (\S+) bound (\S+) ratio (\S+)", line):
        dt, case, nt, name, e, b, r = m.groups()
        key = (case, dt, re.sub(r"encoder\.backbone\.", "", name))
        if key not in rows or float(r) > rows[key][2]:
            rows[key] = (float(e), float(b), float(r), int(nt))
    for m in re.finditer(r"VIT_ATTN_BWD (f32|bf16) N=(\d+) H=(\d+) F=(\d+) (d[qkv]) err (\S+) bound (\S+) ratio (\S+)", line):
        dt, n, h, f, k, e, b, r = m.groups()
        key = (dt, int(n), k)
        if key not in attn or float(r) > attn[key][2]:
            attn[key] = (float(e), float(b), float(r), int(h), int(f))
out = ["# written by tools/vit_grad_accuracy.py from the output of pytest tests/test_gpu_vit_grad.py -s on one MI355X:",
       "# per case, dtype and tensor the largest err / bound over the n_tail runs",
       "# err = max|g - g64| / max|g64| against fp64 autograd of oracle.vcap_oracle.encoder; bound = 10 x torch float32",
       "# autograd's err (f32) or 3 x the bf16 emulation's err (bf16), CPU quantities (tests/vit_grad_cases.py)",
       f"# {'case':4} {'dtype':5} {'tensor':34} {'err':>10} {'bound':>10} {'err/bound':>9} {'n_tail':>6}"]
for (case, dt, name), (e, b, r, nt) in rows.items():
    out.append(f"  {case:4} {dt:5} {name:34} {e:10.3e} {b:10.3e} {r:9.3f} {nt:6d}")
worst = collections.defaultdict(float)
for (case, dt, _), v in rows.items():
    worst[(case, dt)] = max(worst[(case, dt)], v[2])
out.append("# worst err / bound per case and dtype: " + ", ".join(f"{c} {d} {w:.3f}" for (c, d), w in worst.items()))
out.append("# vcap_vit_attention_backward alone: per dtype, token count and output the largest err / bound over heads {1, 3} x frames {1, 3}")
out.append(f"# {'dtype':5} {'tokens':>6} {'out':3} {'err':>10} {'bound':>10} {'err/bound':>9}")
for (dt, n, k), (e, b, r, h, f) in attn.items():
    out.append(f"  {dt:5} {n:6d} {k:3} {e:10.3e} {b:10.3e} {r:9.3f}")
open(dst, "w").write("\n".join(out) + "\n")
print(len(rows), len(attn))
