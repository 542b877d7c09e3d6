"""What layer-wise learning-rate decay costs on the train step, per group and in one launch (development aid, not the contract bench).

The two-stream MF-ViT CA step (two vit_small encoders, the exchange, the summed logits, cross entropy, backward) with mfvit.amp.GradScaler and
clip_grad_norm_ on, AdamW, at two batch sizes.  Four configurations:

    a1, a2   bench.py's 3 param groups (fusion + heads, encoder, encoder) - on the tree given by --parent (the parent commit, built:
             ROOT/multi-feature-vit_amd/mfvit/libmfvit_hip.so) when there is one - run TWICE: the ratio of the two is the session's spread
    b        param_groups_layer_decay([fusion, vit_cxr, vit_enh]) on the per-group path: a launch per group per operation
    c        the same groups with single_launch=True

Every configuration runs in a worker process of its own and takes its turn inside the same interleaved rounds (A B C D A B C D ...), so a drift
of the clock hits all of them alike; medians over the rounds are reported.  Per configuration: the whole step (queued back to back, one
synchronisation per round), and the optimizer part on its own - unscale_, clip_grad_norm_, scaler.step, scaler.update - measured from a drained
GPU: its span on the GPU between two events and the host time until the last launch is queued (GradScaler.step reads the found-inf flag, so
the host waits for the unscale pass in every configuration).

    python tools/perf_optim_groups.py [--parent ROOT] [--batches 16,128] [--precision bf16x3] [--steps 10] [--rounds 5]
                                      [--out profiles/optim_groups_bench.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"


def make_step(config, batch, precision):
    """(forward + backward, optimizer part, number of param groups) of one configuration: 'bench3' | 'layer_decay' | 'layer_decay_single'."""
    import importlib
    import torch
    import vits_returnftrs as vits
    from mfvit import optim
    from mfvit.amp import GradScaler
    from mfvit.losses import cross_entropy
    dev = "cuda:0"
    torch.manual_seed(0)
    fus = importlib.import_module(FUS_MOD)
    backs = []
    for _ in range(2):
        m = vits.vit_small(precision=precision)
        m.head = torch.nn.Linear(m.head.in_features, 3)
        backs.append(m.to(dev).train())
    model = fus.Fus_CrossViT(backs[0], backs[1]).to(dev).train()
    x = torch.randn(batch, 3, 224, 224, device=dev)
    xe = torch.randn(batch, 3, 224, 224, device=dev)
    y = torch.randint(0, 3, (batch,), device=dev)
    if config == "bench3":
        heads = {id(p) for m in backs for p in m.head.parameters()}
        groups = [{"params": list(model.parameters()) + [p for m in backs for p in m.head.parameters()]}]
        groups += [{"params": [p for p in m.parameters() if p.requires_grad and id(p) not in heads]} for m in backs]
        opt = optim.AdamW(groups, lr=1e-4, weight_decay=0.05)
    else:
        groups = optim.param_groups_layer_decay([model, backs[0], backs[1]], 1e-4, weight_decay=0.05, layer_decay=0.75)
        opt = optim.AdamW(groups, lr=1e-4, single_launch=config == "layer_decay_single")
    scaler = GradScaler(init_scale=2.0 ** 10)

    def fwd_bwd():
        opt.zero_grad(set_to_none=True)
        fused, x_c, x_e = model(backs[0], backs[1], x, xe)
        loss, _ = cross_entropy(fused + x_c + x_e, y)
        scaler.scale(loss).backward()

    def optimizer_part():
        scaler.unscale_(opt)
        optim.clip_grad_norm_(opt, 1.0)
        scaler.step(opt)
        scaler.update()

    return fwd_bwd, optimizer_part, len(opt.param_groups)


def time_round(fwd_bwd, optimizer_part, steps):
    """One round: `steps` whole steps back to back, then `steps` steps with the optimizer part measured from a drained GPU."""
    import torch
    fwd_bwd()
    optimizer_part()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fwd_bwd()
        optimizer_part()
    torch.cuda.synchronize()
    whole = (time.perf_counter() - t0) / steps * 1e3
    gpu, host = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(steps):
        fwd_bwd()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        optimizer_part()
        e1.record()
        host.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        gpu.append(e0.elapsed_time(e1))
    return {"step_ms": whole, "optim_gpu_ms": statistics.median(gpu), "optim_host_ms": statistics.median(host)}


def serve(root):
    """Child process on the tree at `root`: 'make config batch precision' builds one step, 'round steps' times one round."""
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
            step = make_step(cmd[1], int(cmd[2]), cmd[3])
            for _ in range(3):
                step[0]()
                step[1]()
            torch.cuda.synchronize()
            print(json.dumps({"ok": 1, "device": torch.cuda.get_device_name(0), "groups": step[2]}), flush=True)
        else:
            print(json.dumps(time_round(step[0], step[1], int(cmd[1]))), flush=True)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--serve", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--batches", default="16,128")
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.serve:
        return serve(a.serve)
    root = os.path.dirname(HERE)
    base = a.parent or root
    where = "parent commit" if a.parent else "this tree"
    configs = [("a1", base, "bench3", f"3 groups as bench.py, {where}"), ("a2", base, "bench3", f"3 groups as bench.py, {where}, again"),
               ("b", root, "layer_decay", "layer decay, a launch per group"), ("c", root, "layer_decay_single", "layer decay, single_launch=True")]
    workers = {name: Worker(r) for name, r, _, _ in configs}
    lines, res = [], {"precision": a.precision, "steps_per_round": a.steps, "rounds": a.rounds, "runs": []}
    keys = ("step_ms", "optim_gpu_ms", "optim_host_ms")
    try:
        for batch in [int(b) for b in a.batches.split(",")]:
            info = {name: workers[name].ask(f"make {cfg} {batch} {a.precision}") for name, _, cfg, _ in configs}
            res["device"] = info["a1"]["device"]
            rounds = {name: [] for name, _, _, _ in configs}
            for _ in range(a.rounds):
                for name, _, _, _ in configs:
                    rounds[name].append(workers[name].ask(f"round {a.steps}"))
            med = {name: {k: statistics.median(r[k] for r in rs) for k in keys} for name, rs in rounds.items()}
            spread = {k: max(med["a1"][k], med["a2"][k]) / min(med["a1"][k], med["a2"][k]) for k in keys}
            lines.append(f"two-stream CA step, {a.precision}, B = {batch}, AdamW + GradScaler + clip_grad_norm_  ({res['device']}; medians of {a.rounds} "
                         f"interleaved rounds of {a.steps} steps, one process per configuration)")
            lines.append(f"  {'':4}{'configuration':<48}{'groups':>7}{'step ms':>10}{'optimizer GPU ms':>18}{'optimizer host ms':>19}")
            for name, _, _, text in configs:
                m = med[name]
                lines.append(f"  {name:<4}{text:<48}{info[name]['groups']:>7}{m['step_ms']:>10.3f}{m['optim_gpu_ms']:>18.3f}{m['optim_host_ms']:>19.3f}")
            lines.append(f"  spread of the two (a) runs: step x{spread['step_ms']:.3f}, optimizer GPU x{spread['optim_gpu_ms']:.3f}, "
                         f"optimizer host x{spread['optim_host_ms']:.3f}")
            worst_a = {k: max(med["a1"][k], med["a2"][k]) for k in keys}
            for name in ("b", "c"):
                lines.append(f"  {name} / slower (a): step x{med[name]['step_ms'] / worst_a['step_ms']:.3f}, optimizer GPU "
                             f"x{med[name]['optim_gpu_ms'] / worst_a['optim_gpu_ms']:.3f}, optimizer host "
                             f"x{med[name]['optim_host_ms'] / worst_a['optim_host_ms']:.3f}")
            lines.append("")
            res["runs"].append({"batch": batch, "groups": {n: info[n]["groups"] for n in info}, "median": med, "spread_of_a": spread,
                                "rounds": rounds})
            print("\n".join(lines[-(len(configs) + 6):]), flush=True)
    finally:
        for w in workers.values():
            w.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
