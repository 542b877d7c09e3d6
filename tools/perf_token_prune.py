"""What attention-guided token pruning between blocks (EViT; token_keep_rate < 1) costs and buys (development aid, not the contract bench).

Three steps in one precision, at two batch sizes: the single-stream vit_small train step (forward -> head -> cross entropy -> backward), the
two-stream MF-ViT CA train step, and the eval() forward of one encoder under no_grad - each at token_keep_rate 1.0, 0.7 and 0.5 behind blocks
3, 6 and 9.  All configurations of a (step, batch) pair are timed in interleaved rounds on one GPU (A B C D E A B C D E ...), so a drift of the
clock hits all of them alike; the median of the rounds and their spread are reported.  Every configuration runs in a worker process of its own
(one model per process, as a training run has it).

--parent ROOT: the checkout of the parent commit (built: ROOT/multi-feature-vit_amd/mfvit/libmfvit_hip.so).  It runs THREE times (three workers
on that tree): the spread between them is the noise of the box, against which "rate 1.0 is the parent's step" is read pair by pair, and the
FASTEST of the three is the baseline of every ratio.  (Three, because the first worker of a run has been seen 1.5 - 2.4 x slow for a whole (step,
batch) pair, cause not determined: with three, every pair still has two healthy parent runs.  All medians are in the file, `parent_spread` per
pair is the second fastest over the fastest.  A worker can also change between a fast and a slow state from round to round; interference
only ever adds time, so beside the median every configuration's best round is kept, with its ratio to the parent's best round.)

The launches of the stages themselves (score, select, reorganise forward and backward) are timed apart, with device events over repeated
launches at each stage's shape, on buffers of the right size (their contents do not matter to the time).

    python tools/perf_token_prune.py [--parent ROOT] [--batches 128,16] [--precision bf16x3] [--steps 10] [--rounds 5]
                                     [--out profiles/token_prune_perf.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
RATES = (1.0, 0.7, 0.5)
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"


def make_step(kind, rate, batch, precision):
    """A closure that runs one step of `kind` ('single' | 'ca' | 'eval').  rate None: the constructor is not given the argument (the parent)."""
    import importlib
    import torch
    import vits
    from mfvit.losses import cross_entropy
    dev = "cuda:0"
    kw = {} if rate is None else dict(token_keep_rate=rate)
    torch.manual_seed(0)
    y = torch.randint(0, 3, (batch,), device=dev)
    x = torch.randn(batch, 3, 224, 224, device=dev)
    if kind in ("single", "eval"):
        m = vits.vit_small(num_classes=3, precision=precision, **kw).to(dev).train(kind == "single")

        def step():
            loss, _ = cross_entropy(m(x), y)
            loss.backward()
            m.zero_grad(set_to_none=True)

        def fwd():
            with torch.no_grad():
                m(x)
        return step if kind == "single" else fwd
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


def stage_launch_times(batch, precision, rate, reps=50):
    """Microseconds per launch of the four stage calls at every stage of a vit_small at 224^2 (device events over `reps` launches)."""
    import torch
    import vits
    from mfvit import _lib
    from mfvit._lib import check, lib, ptr, stream
    dev = "cuda:0"
    m = vits.vit_small(num_classes=3, precision=precision, token_keep_rate=rate)
    sched, fuse, D, H = m.token_schedule(), int(m.token_fuse), m.embed_dim, m.num_heads
    qdt = lib().mfvit_attention_qkv_dtype(_lib.dtype_code(precision), sched[0], D // H)
    out = []

    def timed(fn):
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) / reps * 1e3, 2)
    for T, Tn in zip(sched, sched[1:]):
        K = Tn - 1 - fuse
        qkv = torch.zeros(batch * T * 3 * D * 4, device=dev, dtype=torch.uint8)
        lse = torch.zeros(batch, H, T, device=dev)
        probs, score = torch.empty(batch, T, device=dev), torch.rand(batch, T - 1, device=dev)
        ik = torch.empty(batch, K, device=dev, dtype=torch.int32)
        idr = torch.empty(batch, T - 1 - K, device=dev, dtype=torch.int32)
        w = torch.empty(batch, T - 1 - K, device=dev)
        x, xo = torch.randn(batch, T, D, device=dev), torch.empty(batch, Tn, D, device=dev)
        dx = torch.empty_like(x)
        err = torch.zeros(1, device=dev, dtype=torch.int32)
        keep_score = score.clone()
        row = {"tokens_in": T, "keep": K, "tokens_out": Tn}
        row["score_us"] = timed(lambda: check(lib().mfvit_token_score(qdt, ptr(qkv), ptr(lse), batch, T, H, D // H, ptr(probs), ptr(score), stream()), "score"))
        row["select_us"] = timed(lambda: check(lib().mfvit_token_select(ptr(keep_score), T - 1, batch, T - 1, K, None, ptr(ik), ptr(idr), ptr(w), None,
                                                                        stream()), "select"))
        row["reorg_fwd_us"] = timed(lambda: check(lib().mfvit_token_reorg_fwd(ptr(x), ptr(ik), ptr(idr), ptr(w), ptr(xo), batch, T, D, K, fuse, ptr(err),
                                                                              stream()), "reorg_fwd"))
        row["reorg_bwd_us"] = timed(lambda: check(lib().mfvit_token_reorg_bwd(ptr(xo), ptr(ik), ptr(idr), ptr(w), ptr(dx), batch, T, D, K, fuse, ptr(err),
                                                                              stream()), "reorg_bwd"))
        assert int(err.item()) == 0
        out.append(row)
    return out


def serve(root):
    """Child process on the tree at `root`: 'make kind batch precision rate' builds one step (rate 'none': the constructor is not given the
    argument - the parent commit), 'round steps' times one round, 'stages batch precision rate' times the stage launches."""
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
        elif cmd[0] == "stages":
            print(json.dumps({"stages": stage_launch_times(int(cmd[1]), cmd[2], float(cmd[3]))}), flush=True)
        else:
            print(json.dumps({"ms": time_round(step, int(cmd[1]))}), flush=True)


class Worker:
    """One configuration in a process of its own: every configuration - the parent's too - then runs under the same conditions."""

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


def schedule_of(rate):
    """Tokens per segment of a vit_small at 224^2, prune blocks (3, 6, 9), fused row on: host arithmetic only."""
    import math
    out = [197]
    for _ in range(3):
        K = math.ceil(rate * (out[-1] - 1))
        if K < out[-1] - 1:
            out.append(K + 2)
    return out


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
    parents = [("parent", a.parent, "none"), ("parent_again", a.parent, "none"), ("parent_third", a.parent, "none")] if a.parent else []
    configs = parents + [(f"keep_{r}", root, str(r)) for r in RATES]
    workers = {name: Worker(r) for name, r, _ in configs}
    batches = [int(b) for b in a.batches.split(",")]
    res = {"precision": a.precision, "steps_per_round": a.steps, "rounds": a.rounds, "prune_blocks": [3, 6, 9], "token_fuse": True,
           "baseline": "parent commit, the fastest of its three workers (parent_spread: the second fastest over the fastest)" if a.parent
           else "this tree, keep rate 1.0",
           "layout": "one process per configuration, interleaved rounds", "tokens_per_segment": {f"keep_{r}": schedule_of(r) for r in RATES},
           "runs": [], "stage_launches_us": []}
    try:
        for kind in ("single", "ca", "eval"):
            for batch in batches:
                for name, _, rate in configs:
                    res["device"] = workers[name].ask(f"make {kind} {batch} {a.precision} {rate}")["device"]
                times = {name: [] for name, _, _ in configs}
                for _ in range(a.rounds):
                    for name, _, _ in configs:
                        times[name].append(workers[name].ask(f"round {a.steps}")["ms"])
                pm = sorted(statistics.median(times[name]) for name, _, _ in (parents or configs[:1]))
                base = pm[0]
                best = min(min(times[name]) for name, _, _ in (parents or configs[:1]))
                run = {"step": kind, "batch": batch, "configs": {}}
                if parents:
                    run["parent_spread"] = round(pm[1] / pm[0], 4)
                for k, t in times.items():
                    med = statistics.median(t)
                    run["configs"][k] = {"ms_per_step_median": round(med, 3), "ms_per_step_rounds": [round(v, 3) for v in t],
                                         "spread_pct": round(100 * (max(t) - min(t)) / med, 2), "ratio_to_baseline": round(med / base, 4),
                                         "ms_per_step_best": round(min(t), 3), "ratio_best_to_best": round(min(t) / best, 4)}
                    print(f"{kind:>6} B={batch:<4} {k:>14}: {med:8.3f} ms/step (rounds {min(t):.3f} .. {max(t):.3f})  x{med / base:.3f} of the baseline, "
                          f"best round x{min(t) / best:.3f} of the parent's best", flush=True)
                res["runs"].append(run)
        last = workers[configs[-1][0]]
        for batch in batches:
            for r in RATES[1:]:
                res["stage_launches_us"].append({"batch": batch, "keep_rate": r, "stages": last.ask(f"stages {batch} {a.precision} {r}")["stages"]})
                print(json.dumps(res["stage_launches_us"][-1]), flush=True)
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
