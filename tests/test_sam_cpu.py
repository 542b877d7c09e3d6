"""CPU: the references and the host contract of mfvit.optim.SAM (tests/sam_ref.py).
  - the float64 restatement equals a plain-torch SAM written here (davda54/sam's wrapper, per tensor, float64) over torch.optim.SGD, for
    adaptive in {False, True} and two param groups with different rho;
  - the float32 restatements of the adaptive norm and of the element-wise pass sit under the gates the GPU test uses;
  - an adaptive-norm restatement with a dropped head, tail or second 16-byte group breaks the TOTAL's gate on the GPU test's inputs; an
    element-wise restatement that skips the head or the tail or forgets w * w differs in bits;
  - the wrapper refuses what it cannot do, keeps its call order, and its state dict is the base optimizer's (round trip with a plain Adam);
    the C ABI declares the four entry points."""
import math
import os

import pytest
import torch

import sam_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TorchSAM(torch.optim.Optimizer):
    """davda54/sam, restated: one norm over all groups, rho per group."""

    def __init__(self, params, base_optimizer, rho=0.05, adaptive=False, **kwargs):
        super().__init__(params, dict(rho=rho, adaptive=adaptive, **kwargs))
        self.base_optimizer = base_optimizer(self.param_groups, **kwargs)
        self.param_groups = self.base_optimizer.param_groups

    def _grad_norm(self):
        return torch.norm(torch.stack([((p.abs() if g["adaptive"] else 1.0) * p.grad).norm(p=2) for g in self.param_groups for p in g["params"]
                                       if p.grad is not None]), p=2)

    @torch.no_grad()
    def first_step(self):
        norm = self._grad_norm()
        for g in self.param_groups:
            scale = g["rho"] / (norm + 1e-12)
            for p in g["params"]:
                if p.grad is None:
                    continue
                self.state[p]["old_p"] = p.data.clone()
                p.add_((p.pow(2) if g["adaptive"] else 1.0) * p.grad * scale.to(p))

    @torch.no_grad()
    def second_step(self):
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is not None:
                    p.data = self.state[p]["old_p"]
        self.base_optimizer.step()


def second_gradient(w, i):
    """A gradient that depends on where it is taken: the loss 0.5 (i + 1) |w|^2 + <w, 1>."""
    return (i + 1) * w + 1.0


@pytest.mark.parametrize("adaptive", [False, True], ids=["sam", "asam"])
def test_the_restatement_is_a_plain_torch_sam_in_float64(adaptive):
    from oracle import ref_optim
    counts = [1, 5, 257, 1153, ref.CHUNK + 7]
    ws, gs = ref.inputs(counts)
    split, rhos = 2, [0.05] * 2 + [0.3] * 3
    lr, mom, wd = 0.1, 0.9, 0.01
    ps = [torch.nn.Parameter(w.double().clone()) for w in ws]
    frozen = torch.nn.Parameter(torch.ones(4, dtype=torch.float64))                  # never gets a gradient
    opt = TorchSAM([dict(params=ps[:split] + [frozen], rho=0.05), dict(params=ps[split:], rho=0.3)], torch.optim.SGD, adaptive=adaptive,
                   lr=lr, momentum=mom, weight_decay=wd)
    for p, g in zip(ps, gs):
        p.grad = g.double().clone()
    norm, inv, es, pert = ref.first_step_ref(ws, gs, rhos, [adaptive] * len(ws))
    torch.testing.assert_close(opt._grad_norm(), norm, rtol=1e-13, atol=0)
    opt.first_step()
    for p, want, w, e in zip(ps, pert, ws, es):
        torch.testing.assert_close(p.detach(), want, rtol=1e-13, atol=0)
        assert not torch.equal(p.detach(), w.double())
    g2 = [second_gradient(p.detach(), i) for i, p in enumerate(ps)]
    for p, g in zip(ps, g2):
        p.grad = g.clone()
    opt.second_step()
    want = ref.second_step_ref(ws, lambda i, w: ref_optim.sgd_step(w, second_gradient(pert[i], i), torch.zeros_like(w), lr, mom, wd, first_step=True)[0])
    for p, r in zip(ps, want):
        torch.testing.assert_close(p.detach(), r, rtol=1e-12, atol=0)
    assert torch.equal(frozen.detach(), torch.ones(4, dtype=torch.float64))


def test_a_non_finite_norm_moves_nothing_in_the_restatement():
    ws, gs = ref.inputs([5, 257])
    gs[1][100] = float("inf")
    norm, inv, es, pert = ref.first_step_ref(ws, gs, [0.05, 0.05], [False, True])
    assert float(norm) == math.inf and float(inv) == 0.0
    gs[1][100] = float("nan")
    norm, inv, _, _ = ref.first_step_ref(ws, gs, [0.05, 0.05], [False, True])
    assert math.isnan(float(norm)) and float(inv) == 0.0


def f32_total(ws, gs, phase, mutate=None):
    acc, dropped = 0.0, False
    for w, g in zip(ws, gs):
        s, d = ref.adaptive_norm_sq_f32(w, g, phase, mutate)
        acc += s
        dropped |= d
    return math.sqrt(acc), dropped


def test_float32_floor_sits_under_each_gate_and_the_total_gate_catches_a_dropped_head_tail_or_second_group():
    ws, gs = ref.inputs()
    n = len(ws)
    rho = float(torch.tensor(0.05, dtype=torch.float32))          # the float the C ABI carries is the input of both sides
    norm, inv, es, pert = ref.first_step_ref(ws, gs, [rho] * n, [True] * n)
    for phase in range(4):
        got, _ = f32_total(ws, gs, phase)
        e_n = ref.rel_ratio(torch.tensor(got), norm, ref.NORM_RTOL)
        inv32 = float(torch.tensor(1.0 / (got + 1e-12)).float())
        e_i = ref.rel_ratio(torch.tensor(inv32), inv, ref.INV_RTOL)
        e_w = max(ref.perturbed_ratio(ref.perturb_f32(w, g, inv32, rho, True, phase), p, e) for w, g, p, e in zip(ws, gs, pert, es))
        print(f"phase {phase}: float32 floor norm {e_n:.3f} inv {e_i:.3f} perturbed w {e_w:.3f} of their gates")
        assert 0.0 < max(e_n, e_i) <= 1.0 and 0.0 < e_w <= 1.0, (phase, e_n, e_i, e_w)
        for m in ref.NORM_MUTATIONS:
            bad, dropped = f32_total(ws, gs, phase, m)
            assert dropped == (m != "skip_head" or phase != 0)
            e = ref.rel_ratio(torch.tensor(bad), norm, ref.NORM_RTOL)
            if dropped:
                assert e > 2.0, (m, phase, e)
            else:
                assert bad == got


def test_elementwise_mutations_differ_in_bits():
    ws, gs = ref.inputs()
    inv32, rho = 3.0e-3, 0.05
    for adaptive in (False, True):
        for phase in range(4):
            hit = {m: 0 for m in ref.ELEM_MUTATIONS}
            for w, g in zip(ws, gs):
                for a in range(0, w.numel(), ref.CHUNK):           # CHUNK % 4 == 0: every row of a tensor has its phase
                    wr, gr = w[a:a + ref.CHUNK], g[a:a + ref.CHUNK]
                    good = ref.perturb_f32(wr, gr, inv32, rho, adaptive, phase)
                    n = wr.numel()
                    head = min((4 - phase) % 4, n)
                    for m in ref.ELEM_MUTATIONS:
                        bad = ref.perturb_f32(wr, gr, inv32, rho, adaptive, phase, m)
                        reaches = dict(skip_head=head > 0, skip_tail=(n - head) % 4 > 0, forget_ww=adaptive)[m]
                        assert torch.equal(bad, good) != reaches, (m, adaptive, phase, n)
                        hit[m] += reaches
            assert hit["skip_tail"] >= 5 and (hit["skip_head"] >= 10) == (phase != 0) and (hit["forget_ww"] > 0) == adaptive


def test_wrapper_refusals_call_order_and_state_dict_round_trip():
    from mfvit import optim
    ps = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2))]
    for bad in (torch.optim.SGD, optim.Adam(ps), "Adam", optim.SAM):
        with pytest.raises(TypeError, match="chunk tables"):
            optim.SAM(ps, bad, lr=0.1)
    with pytest.raises(ValueError, match="rho"):
        optim.SAM(ps, optim.SGD, rho=-1.0, lr=0.1)
    for cls in (optim.Adam, optim.AdamW, optim.SGD, optim.LARS):
        assert isinstance(optim.SAM(ps, cls, lr=0.1).base_optimizer, cls)
    sam = optim.SAM([dict(params=ps[:1]), dict(params=ps[1:], rho=0.3, adaptive=True)], optim.Adam, rho=0.1, lr=1e-2, weight_decay=0.5)
    assert sam.param_groups is sam.base_optimizer.param_groups and isinstance(sam, optim._TableOptimizer) and sam.state_names == ("old_p",)
    assert [(g["rho"], g["adaptive"], g["lr"], g["weight_decay"], g["betas"]) for g in sam.param_groups] == \
        [(0.1, False, 1e-2, 0.5, (0.9, 0.999)), (0.3, True, 1e-2, 0.5, (0.9, 0.999))]
    with pytest.raises(RuntimeError, match="first_step"):
        sam.second_step()
    with pytest.raises(RuntimeError, match="closure"):
        sam.step()
    sam.first_step()                                   # no gradient anywhere: nothing to launch, but the call order still holds
    with pytest.raises(RuntimeError, match="twice"):
        sam.first_step()
    assert sam.second_step() is None and all(torch.equal(p.detach(), torch.ones_like(p)) for p in ps) and len(sam.state) == 0
    with pytest.raises(RuntimeError, match="first_step"):
        sam.second_step()
    # the state dict is the base optimizer's: a plain Adam's loads into SAM and back, old_p is never part of it
    plain = optim.Adam([dict(params=ps[:1]), dict(params=ps[1:])], lr=3e-3)
    for i, p in enumerate(ps):
        plain.state[p] = dict(step=torch.tensor(7.0), exp_avg=torch.full_like(p, 0.5 + i), exp_avg_sq=torch.full_like(p, 2.0 + i))
    sam.state[ps[0]]["old_p"] = torch.zeros(3)
    sam.load_state_dict(plain.state_dict())
    assert sam.param_groups is sam.base_optimizer.param_groups and len(sam.param_groups) == 2
    assert [(g["lr"], g["rho"], g["adaptive"]) for g in sam.param_groups] == [(3e-3, 0.1, False), (3e-3, 0.3, True)]
    sd = sam.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][1]["exp_avg"][0, 0]) == 1.5
    again = optim.Adam([dict(params=ps[:1]), dict(params=ps[1:])], lr=1.0)
    again.load_state_dict(sd)                          # (the rho / adaptive keys of the groups ride along, as any extra key does)
    assert again.param_groups[0]["lr"] == 3e-3 and float(again.state[ps[1]]["exp_avg_sq"][1, 1]) == 3.0 and float(again.state[ps[0]]["step"]) == 7.0
    assert callable(sam.clip_grad_norm_)


def test_entry_points_are_declared_exported_and_bound():
    from mfvit import _lib
    text = open(os.path.join(ROOT, "include", "mfvit.h")).read()
    h = _lib.lib()
    for name, arity in (("mfvit_sam_norm_partials", 5), ("mfvit_sam_scale", 5), ("mfvit_sam_perturb", 5), ("mfvit_sam_restore", 4)):
        assert f"int {name}(" in text and hasattr(h, name) and len(_lib.SIGNATURES[name][1]) == arity, name
    assert h.mfvit_abi_version() == 5
    # argument checks run before any launch: null pointers and empty tables are refused on the host
    assert h.mfvit_sam_norm_partials(None, 1, 0, None, None) != 0 and h.mfvit_sam_scale(None, 0, None, None, None) != 0
    assert h.mfvit_sam_perturb(None, 1, None, 0.05, None) != 0 and h.mfvit_sam_restore(None, 1, None, None) != 0
