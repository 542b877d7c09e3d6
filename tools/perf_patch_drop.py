"""What patch dropout (timm PatchDropout) buys on the train step (development aid, not the contract bench).

Two steps in one precision, at two batch sizes: the single-stream vit_small step (forward -> head -> cross entropy -> backward) and the two-stream
MF-ViT CA step (two encoders, the exchange, the summed logits, cross entropy, backward), each at patch_drop_rate 0, 0.25, 0.5 and 0.75.  All
configurations of a (step, batch) pair are timed in interleaved rounds on one GPU (A B C D A B C D ...), so a drift of the clock hits all of
them alike; the median of the rounds and their spread are reported.

Every configuration runs in a worker process of its own (one model per process, as a training run has it) and takes its turn inside the same
rounds.  --parent ROOT: the checkout of the parent commit (built: ROOT/multi-feature-vit_amd/mfvit/libmfvit_hip.so) whose rate-0 step is the
baseline: one more worker, on that tree's package and library.

    python tools/perf_patch_drop.py [--parent ROOT] [--batches 128,16] [--precision bf16x3] [--steps 10] [--rounds 5]
                                    [--out profiles/patch_drop_perf.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
RATES = (0.0, 0.25, 0.5, 0.75)
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"


def make_step(kind, rate, batch, precision):
    """A closure that runs one train step of `kind` ('single' | 'ca').  rate None: the constructor is not given the argument at all (the parent)."""
    import importlib
    import torch
    import vits
    from mfvit.losses import cross_entropy
    dev = "cuda:0"
    kw = {} if rate is None else dict(patch_drop_rate=rate)
    torch.manual_seed(0)
    y = torch.randint(0, 3, (batch,), device=dev)
    x = torch.randn(batch, 3, 224, 224, device=dev)
    if kind == "single":
        m = vits.vit_small(num_classes=3, precision=precision, **kw).to(dev).train()

        def step():
            loss, _ = cross_entropy(m(x), y)
            loss.backward()
            m.zero_grad(set_to_none=True)
        return step
    fus = importlib.import_module(FUS_MOD)
    xe = torch.randn(batch, 3, 224, 224, device=dev)
    backs = [vits.vit_small(num_classes=3, precision=precision, **kw).to(dev).train() for _ in range(2)]
    model = fus.Fus_CrossViT(backs[0], backs[1]).to(dev).train()

    def step():
        fused, x_c, x_e = model(backs[0], backs[1], x, xe)
        loss, _ = cross_entropy(fused + x_c + x_e, y)
        loss.backward()
        for mod in (model, backs[0], backs[1]):
            mod.zero_grad(set_to_none=True)
    return step


def time_round(step, steps):
    import torch
    step()                                  # (untimed: workspaces of this configuration back in the pools)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def serve(root):
    """Child process on the tree at `root`: 'make kind batch precision rate' builds one step (rate 'none': the constructor is not given the
    argument - the parent commit), 'round steps' times one round."""
    for p in (root, os.path.join(root, "multi-feature-vit_amd")):
        sys.path.insert(0, p)
    import torch
    step = None
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "make":
            step = None
            torch.cuda.empty_cache()
            step = make_step(cmd[1], None if cmd[4] == "none" else float(cmd[4]), int(cmd[2]), cmd[3])
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            print(json.dumps({"ok": 1, "device": torch.cuda.get_device_name(0)}), flush=True)
        else:
            print(json.dumps({"ms": time_round(step, int(cmd[1]))}), flush=True)


class Worker:
    """One configuration in a process of its own: every configuration - the parent's too - then runs under the same conditions (one model,
    its own streams; several models in one process share the hardware queues and serialise each other's encoder streams at small batches)."""

    def __init__(self, root):
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", os.path.abspath(root)], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True)

    def ask(self, line):
        self.p.stdin.write(line + "\n")
        self.p.stdin.flush()
        while True:
            out = self.p.stdout.readline()
            if not out:
                raise RuntimeError("a worker process ended")
            if out.startswith("{"):
                return json.loads(out)

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=60)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--serve", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--batches", default="128,16")
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.serve:
        return serve(a.serve)
    root = os.path.dirname(HERE)
    configs = ([("parent_rate_0", a.parent, "none")] if a.parent else []) + [(f"rate_{r}", root, str(r)) for r in RATES]
    workers = {name: Worker(r) for name, r, _ in configs}
    res = {"precision": a.precision, "steps_per_round": a.steps, "rounds": a.rounds,
           "baseline": "parent commit, rate 0" if a.parent else "this tree, rate 0", "layout": "one process per configuration, interleaved rounds",
           "runs": []}
    try:
        for kind in ("single", "ca"):
            for batch in [int(b) for b in a.batches.split(",")]:
                for name, _, rate in configs:
                    res["device"] = workers[name].ask(f"make {kind} {batch} {a.precision} {rate}")["device"]
                times = {name: [] for name, _, _ in configs}
                for _ in range(a.rounds):
                    for name, _, _ in configs:
                        times[name].append(workers[name].ask(f"round {a.steps}")["ms"])
                base = statistics.median(times[configs[0][0]])
                run = {"step": kind, "batch": batch, "configs": {}}
                for k, t in times.items():
                    med = statistics.median(t)
                    run["configs"][k] = {"ms_per_step_median": round(med, 3), "ms_per_step_rounds": [round(v, 3) for v in t],
                                         "spread_pct": round(100 * (max(t) - min(t)) / med, 2), "ratio_to_baseline": round(med / base, 4)}
                    print(f"{kind:>6} B={batch:<4} {k:>14}: {med:8.3f} ms/step (rounds {min(t):.3f} .. {max(t):.3f})  x{med / base:.3f} of the baseline",
                          flush=True)
                res["runs"].append(run)
    finally:
        for w in workers.values():
            w.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
