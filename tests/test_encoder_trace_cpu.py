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


def _launches(out, name):
    """the lines of scenario `name` in the tool's output, without the `call ..` lines (which name the entry point)"""
    lines, on = [], False
    for line in out.splitlines():
        if line.startswith("== "):
            on = line[3:].strip() == name
        elif on and not line.startswith("call "):
            lines.append(line)
    assert lines, f"no scenario named {name}"
    return lines


def test_full_range_issues_the_whole_stack_launches():
    """include/mfvit.h: the range [0, depth) through mfvit_vit_forward_seg / _backward_seg issues exactly the launches of mfvit_vit_forward(_drop)
    / mfvit_vit_backward_ex with image_in = 1, and of mfvit_vit_forward_x0 / _backward_x0 with image_in = 0: one run of the driver, the same
    requests through both, equal line for line apart from the lines that name the call"""
    rc, out = _tool()
    assert rc == 0, out[-6000:]
    for seg, whole in (("seg_full_image", "stack_full_image"), ("seg_full_x0", "x0_full")):
        a, b = _launches(out, seg), _launches(out, whole)
        assert len(a) > 100 and all(line.startswith("rc 0") for line in a if line.startswith("rc "))
        assert a == b, f"{seg} differs from {whole}: first at line {next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))}"


def test_sanitized_traces_match_golden():
    """the same program with -fsanitize=address,undefined on the harness and vit.hip: exit 0 and the same output"""
    rc, out = _tool("--sanitize", "--check")
    assert rc == 0, out[-6000:]
