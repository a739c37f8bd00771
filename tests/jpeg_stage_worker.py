"""Child process of test_gpu_jpeg_sweep.py: the pinned staging buffer of vcap_jpeg_decode, the only state the
decoder carries between calls, from its first allocation in a fresh process.  Decodes, in this order and each
compared with the oracle straight away:
  one 8x8 image (the buffer is allocated small), 16 images of 64x64 (it grows), the 8x8 image (reused, larger
  than needed), the 16 images again (reused as it is);
  the same four calls on a non-default stream;
  two threads at once, four calls each, on different cases (the calls serialise on the buffer's lock).
Every check is an assert; the last line printed is "ok"."""
import sys
import threading
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "video-caption-algorithm_amd", ROOT, ROOT / "tests"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import jpeg_cases as JC  # noqa: E402
from vcap.jpeg import decode_jpegs  # noqa: E402


def check(cases, dev):
    got = decode_jpegs([c.data for c in cases], dev)
    torch.cuda.current_stream(dev).synchronize()
    got = got.cpu().numpy()
    for k, c in enumerate(cases):
        assert np.array_equal(got[k], JC.expected(c)), (k, c.name)


def main():
    dev = torch.device("cuda:0")
    small, big = [JC.case("samp_grey_8x8")], JC.batch("b64") * 4
    assert len(big) == 16
    for c in small + big + JC.batch("b420") + JC.batch("bgrey"):
        JC.expected(c)                                    # the oracle's share, before any thread starts
    sequence = [small, big, small, big]
    for cases in sequence:
        check(cases, dev)
    print("default stream ok", flush=True)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        for cases in sequence:
            check(cases, dev)
    print("side stream ok", flush=True)
    errors = []

    def worker(calls):
        try:
            for cases in calls:
                check(cases, dev)
        except BaseException as e:  # noqa: BLE001
            errors.append(repr(e))

    b420, grey = JC.batch("b420"), JC.batch("bgrey")
    threads = [threading.Thread(target=worker, args=([b420, small, b420[:3], big],)),
               threading.Thread(target=worker, args=([grey, big, grey[:1], [JC.case("amp_all_positions_maximal")]],))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    print("ok")


if __name__ == "__main__":
    main()
