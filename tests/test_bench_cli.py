"""CPU: bench.py's command line — a plain run is the headline measurement alone, everything else sits behind --full."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=300)


def test_bench_help_lists_full_and_details():
    r = run_bench("--help")
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--details" in r.stdout


def test_bench_details_needs_full():
    r = run_bench("--details", "x.json")           # rejected by the parser, before any device is touched
    assert r.returncode == 2
    assert "--details needs --full" in r.stderr
