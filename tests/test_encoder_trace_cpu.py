"""The encoder's launch sequences, traced on the CPU (tools/encoder_trace.py): csrc/vit.hip compiled host-only against the recording stubs of
tests/encoder_trace/ must reproduce tests/golden/encoder_trace/ call for call - launchers, arguments, streams, events, return codes.  A change
of the encoder's host code that is meant to change a launch sequence regenerates the golden files (--regen) and shows up as their diff."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "encoder_trace.py")


def _tool(*args):
    pr = subprocess.run([sys.executable, TOOL] + list(args), capture_output=True, text=True, cwd=ROOT)
    return pr.returncode, pr.stdout + pr.stderr


def test_traces_match_golden():
    rc, out = _tool("--check")
    assert rc == 0, out[-6000:]
    m = re.search(r"(\d+) of (\d+) scenarios match", out)
    assert m and int(m.group(1)) == int(m.group(2)) > 0, out[-2000:]


def test_sanitized_traces_match_golden():
    """the same program with -fsanitize=address,undefined on the harness and vit.hip: exit 0 and the same output"""
    rc, out = _tool("--sanitize", "--check")
    assert rc == 0, out[-6000:]
