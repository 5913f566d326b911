"""bench.py's options on the CPU: a plain run leaves everything besides the headline off, --full turns it on, and the single switches
still win over either."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parsed(*argv):
    code = ("import json, sys, bench\nsys.argv = ['bench.py'] + sys.argv[1:]\na = bench.parse_args()\n"
            "print(json.dumps({k: getattr(a, k) for k in ('full', 'verify', 'config5')}))\n")
    p = subprocess.run([sys.executable, "-c", code, *argv], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout)


@pytest.mark.parametrize("argv, want", [
    ((), {"full": False, "verify": False, "config5": None}),
    (("--full",), {"full": True, "verify": True, "config5": None}),
    (("--full", "--no-verify", "--no-config5"), {"full": True, "verify": False, "config5": False}),
    (("--verify", "--config5"), {"full": False, "verify": True, "config5": True}),
])
def test_full_decides_what_runs_besides_the_headline(argv, want):
    assert parsed("--gpus", "1", "--steps", "4", "--warmup", "2", *argv) == want
