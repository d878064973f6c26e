"""bench.py's command line, no GPU: the options of the plain and the --full
run exist, and an extra measurement asked for without --full is refused
before anything is set up (never quietly left out)."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], capture_output=True, text=True,
                          timeout=60, cwd=REPO)


def test_help_lists_full_and_dump_outputs():
    r = _bench("--help")
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


def test_cpu_baseline_on_needs_full():
    r = _bench("--cpu-baseline", "on")
    assert r.returncode == 2 and "needs --full" in r.stderr
