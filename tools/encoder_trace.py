#!/usr/bin/env python3
"""Launch-sequence trace of the encoder's host code (csrc/vit.hip) on the CPU: vit.hip compiled host-only and linked against the recording stubs
and the scenario driver of tests/encoder_trace/.  No GPU is opened; nothing of the trace depends on the machine.

  python3 tools/encoder_trace.py                    print the trace of every scenario
  python3 tools/encoder_trace.py --only NAME        ... of one (--list: the names)
  python3 tools/encoder_trace.py --check            compare with tests/golden/encoder_trace/<name>.txt, unified diff on a mismatch (exit 1)
  python3 tools/encoder_trace.py --regen            rewrite those files
  python3 tools/encoder_trace.py --sanitize         harness and vit.hip built with -fsanitize=address,undefined (host code, stand-alone program)
  python3 tools/encoder_trace.py --source PATH      trace another copy of vit.hip (its includes resolve against csrc/)
"""
import argparse
import difflib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi-feature-vit_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "encoder_trace")
GOLDEN = os.path.join(ROOT, "tests", "golden", "encoder_trace")
BUILD = os.path.join(ROOT, "build", "encoder_trace")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build(source, sanitize):
    """-> path of the driver program"""
    name = "trace_asan" if sanitize else "trace"
    os.makedirs(BUILD, exist_ok=True)
    # host side only: no device code is generated, and none is needed
    flags = ["--offload-arch=gfx950", "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-Wno-unused-value", "-I", CSRC,
             "-I", os.path.join(ROOT, "include")]
    if sanitize:
        flags += ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    objs = []
    for src in (source, os.path.join(HARNESS, "stubs.cpp"), os.path.join(HARNESS, "driver.cpp")):
        obj = os.path.join(BUILD, f"{name}_{os.path.splitext(os.path.basename(src))[0]}.o")
        # vit.hip includes "../../include/mfvit.h" relative to itself: a copy elsewhere finds it through the harness directory
        subprocess.check_call([HIPCC] + flags + ["-I", HARNESS, "-c", src, "-o", obj])
        objs.append(obj)
    exe = os.path.join(BUILD, name)
    # (the stubs define the seven HIP runtime calls vit.hip makes: the HIP runtime library is not linked, so no GPU can be opened)
    link = [HIPCC, "-no-hip-rt", "-o", exe] + objs + ["-pthread"]
    if sanitize:
        link += ["-fsanitize=address,undefined"]
    subprocess.check_call(link)
    return exe


def run(exe, args=()):
    env = dict(os.environ)
    for k in [k for k in env if k.startswith("MFVIT_")]:
        del env[k]
    env["ASAN_OPTIONS"] = "detect_leaks=0"   # (the library's side streams and events live as long as their thread by design)
    pr = subprocess.run([exe] + list(args), env=env, capture_output=True, text=True)
    if pr.returncode != 0:
        sys.stderr.write(pr.stdout[-2000:] + pr.stderr[-8000:])
        raise SystemExit(f"{exe} exited with {pr.returncode}")
    return pr.stdout


def split(out):
    """the driver's output -> {scenario: text}"""
    traces, name = {}, None
    for line in out.splitlines(keepends=True):
        if line.startswith("== "):
            name = line[3:].strip()
            traces[name] = ""
        elif name is not None:
            traces[name] += line
    return traces


def check(traces, complete=True):
    bad = 0
    for name, text in traces.items():
        path = os.path.join(GOLDEN, name + ".txt")
        want = open(path).read() if os.path.exists(path) else None
        if want != text:
            bad += 1
            sys.stdout.writelines(difflib.unified_diff((want or "").splitlines(keepends=True), text.splitlines(keepends=True),
                                                       f"golden/{name}.txt" + ("" if want is not None else " (missing)"), f"traced/{name}"))
    stale = sorted(set(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".txt")) - set(traces)) if complete and os.path.isdir(GOLDEN) else []
    for name in stale:
        print(f"golden/{name}.txt: no scenario of that name")
    print(f"{len(traces) - bad} of {len(traces)} scenarios match" + (f", {len(stale)} stale golden files" if stale else ""))
    return 1 if bad or stale else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--source", default=os.path.join(CSRC, "vit.hip"))
    ap.add_argument("--only")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--regen", action="store_true")
    ap.add_argument("--sanitize", action="store_true")
    a = ap.parse_args()
    exe = build(a.source, a.sanitize)
    if a.list:
        sys.stdout.write(run(exe, ["--list"]))
        return 0
    out = run(exe, ["--only", a.only] if a.only else [])
    traces = split(out)
    if a.regen:
        os.makedirs(GOLDEN, exist_ok=True)
        if not a.only:
            for f in os.listdir(GOLDEN):
                if f.endswith(".txt"):
                    os.remove(os.path.join(GOLDEN, f))
        for name, text in traces.items():
            with open(os.path.join(GOLDEN, name + ".txt"), "w") as f:
                f.write(text)
        print(f"wrote {len(traces)} files, {sum(len(t) for t in traces.values())} bytes")
        return 0
    if a.check:
        return check(traces, complete=not a.only)
    sys.stdout.write(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
