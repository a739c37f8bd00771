"""The decode graph cache (csrc/graph_cache.hip) as a bounded LRU: with VCAP_GRAPH_CACHE_MAX=2 three
greedy prompts, a sampling call and a beam search through one decoder never hold more than two graphs,
an evicted prompt is captured again and replays to the ids of its first run and of the eager run, and
vcap_graph_cache_clear empties the cache.  One child process (tests/graph_cache_worker.py), since the
library reads VCAP_GRAPH_CACHE_MAX once per process."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent


def test_bounded_lru_evicts_and_recaptures():
    env = dict(os.environ, VCAP_GRAPH_CACHE_MAX="2")
    r = subprocess.run([sys.executable, str(HERE / "graph_cache_worker.py")], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok", r.stdout + r.stderr
