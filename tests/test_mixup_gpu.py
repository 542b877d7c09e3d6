"""GPU: mfvit_batch_mix (random erasing + Mixup / CutMix of one or two streams in one launch) and mfvit_cross_entropy_soft against a plain-torch
CPU restatement written here: index assignment for erase / cutmix, lam * a + (1 - lam) * b in float64 for mixup, and
-(y * log_softmax).sum(1).mean() in float64 for the loss.

Bounds.  Copy, erase and CutMix elements are moves and zeros: bit-exact.  A Mixup element is two products and a sum rounded to f32 (with or
without FMA contraction): |out - ref64| <= 2^-23 (|lam a| + |(1 - lam) b|).  The loss and its gradient carry the tolerances tests/test_ops_gpu.py
applies to mfvit_cross_entropy: 1e-6 max(1, |loss|) and 1e-6 of the gradient's scale."""
import importlib

import pytest
import torch

from conftest import rng_tensor

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FUS_MOD = "model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_changemodelinputlocation_std002_sum"


def row(j, mode, cut=(0, 0, 0, 0), erase=None):
    return [j, mode, *cut, int(erase is not None), *(erase or (0, 0, 0, 0)), 0]


def tables(rows, lams):
    return torch.tensor(rows, dtype=torch.int32), torch.tensor(lams, dtype=torch.float32)


def erased(x, desc):
    """E(x_k): every sample with its OWN erase box filled with 0."""
    e = x.clone()
    for k in range(x.shape[0]):
        if int(desc[k, 6]):
            yl, yh, xl, xh = desc[k, 7:11].tolist()
            e[k, :, yl:yh, xl:xh] = 0.0
    return e


def check_mix(out, x, desc, lam):
    """out (device result, moved to the CPU) against the restatement; returns the largest mixup error in units of its bound (printed)."""
    out = out.cpu()
    e = erased(x, desc)
    worst = 0.0
    for i in range(x.shape[0]):
        j, mode = int(desc[i, 0]), int(desc[i, 1])
        if mode == 1:
            l = lam[i].double()
            t1, t2 = l * e[i].double(), (1.0 - l) * e[j].double()
            err, bound = (out[i].double() - (t1 + t2)).abs(), 2.0 ** -23 * (t1.abs() + t2.abs())
            assert bool((err <= bound).all()), f"sample {i}: mixup error {float((err - bound).max()):.3e} above its bound"
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            continue
        ref = e[i].clone()
        if mode == 2:
            yl, yh, xl, xh = desc[i, 2:6].tolist()
            ref[:, yl:yh, xl:xh] = e[j][:, yl:yh, xl:xh]
        assert torch.equal(out[i].view(torch.int32), ref.view(torch.int32)), f"sample {i} (mode {mode}) is not bit-exact"
    return worst


def run_mix(x, desc, lam, x2=None):
    from mfvit import ops
    from mfvit.mixup import check_params
    check_params(desc, lam, x.shape[0], x.shape[2], x.shape[3])
    r = ops.batch_mix(x.to(DEV), desc.to(DEV), lam.to(DEV), None if x2 is None else x2.to(DEV))
    torch.cuda.synchronize()
    return r


def box(H, W, yl, yh, xl, xh):
    """The box clipped to the image (small test images keep the same table recipe)."""
    yl, xl = min(max(yl, 0), H), min(max(xl, 0), W)
    return yl, min(max(yh, yl), H), xl, min(max(xh, xl), W)


def hand_tables(n, H, W):
    """n >= 5 samples with the flip partner: every mode, an empty box with lam = 1, a full box with lam = 0, boxes with odd edges that cut
    through a 16-byte vector, a partner whose erase box overlaps the cut box, an erased mixup pair.  (CutMix ignores lam in the image; the
    table carries the corrected value all the same.)"""
    rows = [row(n - 1, 2, box(H, W, 3, H - 5, 5, W - 1), erase=box(H, W, 1, 9, 2, 11)),      # odd edges; own erase box overlaps the cut box
            row(n - 2, 1, erase=box(H, W, 0, H, 1, 6)),                                      # mixup of an erased sample
            row(n - 3, 0, erase=box(H, W, H // 2, H // 2 + 3, 1, W - 1)),                    # copy + erase (n = 5: its own partner)
            row(n - 4, 2, (0, 0, 0, 0)),                                                     # empty box, lam = 1
            row(n - 5, 2, (0, H, 0, W), erase=box(H, W, 2, 7, 3, W - 2))]                    # full box, lam = 0; its partner is read erased
    for i in range(5, n):
        mode = (1, 2, 0)[i % 3]
        rows.append(row(n - 1 - i, mode, box(H, W, i, H - i, 2 * i + 1, W - 3) if mode == 2 else (0, 0, 0, 0),
                        erase=box(H, W, i, i + 4, 1, 2 + i) if i % 2 else None))
    lams = []
    for r in rows:
        lams.append(0.6180339887 if r[1] == 1 else 1.0 - ((r[3] - r[2]) * (r[5] - r[4])) / (H * W) if r[1] == 2 else 1.0)
    lams[1] = 0.3
    return tables(rows, lams)


@pytest.mark.parametrize("shape", [(5, 3, 30, 34), (8, 3, 30, 34), (5, 3, 224, 224), (6, 3, 224, 224), (7, 1, 19, 8)])
def test_batch_mix_hand_built_tables(shape):
    n, _, H, W = shape
    x = rng_tensor(70 + n, shape)
    desc, lam = hand_tables(n, H, W)
    worst = check_mix(run_mix(x, desc, lam), x, desc, lam)
    print(f"batch_mix {shape}: largest mixup error = {worst:.3f} of its bound")


def test_batch_mix_mixup_with_lam_zero_and_one_and_an_unaligned_base():
    """lam = 1 / lam = 0 in mixup mode, and a W % 4 == 0 batch whose base address is not 16-byte aligned (the scalar path)."""
    from mfvit import ops
    n, C, H, W = 4, 3, 16, 16
    x = rng_tensor(81, (n, C, H, W))
    desc, lam = tables([row(3, 1), row(2, 1), row(1, 1), row(0, 2, (1, 6, 3, 9), erase=(3, 9, 5, 10))], [1.0, 0.0, 0.37, 0.25])
    out = run_mix(x, desc, lam)
    check_mix(out, x, desc, lam)
    assert torch.equal(out[0].cpu(), x[0]) and torch.equal(out[1].cpu(), x[2])
    buf = torch.zeros(x.numel() + 4, device=DEV)
    xs = buf[1:1 + x.numel()].view(n, C, H, W)
    xs.copy_(x)
    assert xs.data_ptr() % 16 == 4 and xs.is_contiguous()
    out_s = ops.batch_mix(xs, desc.to(DEV), lam.to(DEV))
    assert torch.equal(out_s, out)


@pytest.mark.parametrize("n", [1, 2])
def test_batch_mix_self_partner(n):
    """n = 1: the sample is its own partner in every mode."""
    H, W = 30, 36
    for mode, l in ((0, 1.0), (1, 0.4), (2, 0.5)):
        x = rng_tensor(90 + mode, (n, 3, H, W))
        desc, lam = tables([row(n - 1 - i, mode, (4, 20, 7, 29) if mode == 2 else (0, 0, 0, 0), erase=(10, 15, 5, 30)) for i in range(n)], [l] * n)
        check_mix(run_mix(x, desc, lam), x, desc, lam)


@pytest.mark.parametrize("shape,mode", [((7, 3, 32, 36), "elem"), ((7, 3, 30, 34), "elem"), ((9, 3, 64, 64), "pair"), ((16, 3, 224, 224), "batch")])
def test_batch_mix_sampled_tables(shape, mode):
    """Tables as Mixup.sample_params draws them: a random permutation partner (elem), the flip partner with n odd (pair), erase boxes."""
    from mfvit.mixup import Mixup
    n, _, H, W = shape
    m = Mixup(mode=mode, partner="perm" if mode == "elem" else "flip", erase_prob=0.5)
    x = rng_tensor(100 + n, shape)
    for seed in (0, 1):
        desc, lam = m.sample_params(n, H, W, torch.Generator().manual_seed(seed))
        worst = check_mix(run_mix(x, desc, lam), x, desc, lam)
        print(f"batch_mix sampled {shape} {mode} seed {seed}: modes {sorted(set(desc[:, 1].tolist()))}, mixup error {worst:.3f} of its bound")


@pytest.mark.parametrize("shape", [(5, 3, 30, 34), (6, 3, 224, 224)])
def test_two_streams_equal_two_one_stream_calls(shape):
    n, _, H, W = shape
    x, x2 = rng_tensor(111, shape), rng_tensor(112, shape)
    desc, lam = hand_tables(n, H, W)
    oa, ob = run_mix(x, desc, lam, x2)
    assert torch.equal(oa.view(torch.int32), run_mix(x, desc, lam).view(torch.int32))
    assert torch.equal(ob.view(torch.int32), run_mix(x2, desc, lam).view(torch.int32))
    check_mix(ob, x2, desc, lam)


# ------------------------------------------------------------------------------------------------------- soft-target cross entropy
def rel_err(got, ref):
    ref, got = ref.double().cpu(), got.double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def first_argmax(logits):
    C = logits.shape[1]
    top = logits == logits.max(1, keepdim=True)[0]
    return torch.where(top, torch.arange(C).expand_as(logits), torch.full_like(logits, C, dtype=torch.long)).min(1)[0]


def ce_case(B, C, with_partner, seed=29):
    g = torch.Generator().manual_seed(seed + B + C)
    logits = torch.randn(B, C, generator=g) * 3.0
    logits[4] = 0.5
    logits[4, C // 3] = logits[4, C - 1] = 1.0                    # a tie row: the first maximum wins
    target = torch.randint(0, C, (B,), generator=g)
    partner = lam = None
    if with_partner:
        partner = torch.randperm(B, generator=g).int()
        lam = torch.rand(B, generator=g)
        lam[0], lam[1] = 1.0, 0.0
    return logits, target, partner, lam


def ce_oracle(logits, target, partner, lam, smoothing):
    B, C = logits.shape
    s = torch.full((B, C), smoothing / C, dtype=torch.float64)
    s[torch.arange(B), target] += 1.0 - smoothing
    y = s if partner is None else lam.double()[:, None] * s + (1.0 - lam.double()[:, None]) * s[partner.long()]
    ld = logits.double().requires_grad_(True)
    loss = -(y * torch.log_softmax(ld, 1)).sum(1).mean()
    loss.backward()
    return float(loss.detach()), ld.grad


def to_dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


@pytest.mark.parametrize("with_partner", [False, True])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
@pytest.mark.parametrize("B", [9, 257])
@pytest.mark.parametrize("C", [3, 64])
def test_cross_entropy_soft_matches_the_float64_oracle(C, B, smoothing, with_partner):
    from mfvit import ops
    logits, target, partner, lam = ce_case(B, C, with_partner)
    lr, gr = ce_oracle(logits, target, partner, lam, smoothing)
    loss, dlogits, preds = ops.cross_entropy_soft(*to_dev(logits, target, partner, lam), smoothing=smoothing)
    e_l, e_g = abs(float(loss) - lr), rel_err(dlogits, gr)
    print(f"cross_entropy_soft C={C} B={B} smoothing={smoothing} partner={with_partner}: loss err {e_l:.2e} (loss {lr:.4f}), dlogits rel err {e_g:.2e}")
    assert e_l <= 1e-6 * max(1.0, abs(lr))
    assert e_g < 1e-6
    assert preds.cpu().tolist() == first_argmax(logits).tolist()
    assert int(preds[4]) == C // 3
    # the same input, the same bits; and the loss alone (no gradient asked)
    loss2, dlogits2, preds2 = ops.cross_entropy_soft(*to_dev(logits, target, partner, lam), smoothing=smoothing)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(dlogits.view(torch.int32), dlogits2.view(torch.int32))
    assert torch.equal(preds, preds2)
    loss3, none, _ = ops.cross_entropy_soft(*to_dev(logits, target, partner, lam), smoothing=smoothing, want_grad=False)
    assert none is None and torch.equal(loss.view(torch.int32), loss3.view(torch.int32))


@pytest.mark.parametrize("B", [9, 257])
@pytest.mark.parametrize("C", [3, 64])
def test_cross_entropy_soft_without_smoothing_or_partner_agrees_with_cross_entropy(C, B):
    from mfvit import ops
    logits, target, _, _ = ce_case(B, C, False)
    loss, dlogits, preds = ops.cross_entropy_soft(*to_dev(logits, target), smoothing=0.0)
    loss_h, dlogits_h, preds_h = ops.cross_entropy(*to_dev(logits, target))
    e_l, e_g = abs(float(loss) - float(loss_h)), rel_err(dlogits, dlogits_h)
    print(f"cross_entropy_soft vs cross_entropy C={C} B={B}: loss diff {e_l:.2e}, dlogits rel diff {e_g:.2e}")
    assert e_l <= 1e-6 * max(1.0, abs(float(loss_h)))
    assert e_g < 1e-6
    assert torch.equal(preds, preds_h)


def test_soft_cross_entropy_autograd_and_plain_targets():
    """losses.soft_cross_entropy: a MixTarget, and a plain int64 target with smoothing = nn.CrossEntropyLoss(label_smoothing=...)."""
    from mfvit.losses import soft_cross_entropy
    from mfvit.mixup import MixTarget
    logits, target, partner, lam = ce_case(9, 3, True)
    lr, gr = ce_oracle(logits, target, partner, lam, 0.1)
    z = logits.to(DEV).requires_grad_(True)
    loss, preds = soft_cross_entropy(z, MixTarget(*to_dev(target, partner, lam), smoothing=0.1))
    (2.0 * loss).backward()
    assert abs(float(loss.detach()) - lr) <= 1e-6 * max(1.0, abs(lr)) and rel_err(z.grad, 2.0 * gr) < 1e-6
    assert not preds.requires_grad and preds.cpu().tolist() == first_argmax(logits).tolist()
    ld = logits.double().requires_grad_(True)
    ref = torch.nn.CrossEntropyLoss(label_smoothing=0.1)(ld, target)
    ref.backward()
    z = logits.to(DEV).requires_grad_(True)
    loss, _ = soft_cross_entropy(z, target.to(DEV), smoothing=0.1)
    loss.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-6 * max(1.0, abs(float(ref.detach()))) and rel_err(z.grad, ld.grad) < 1e-6


# ------------------------------------------------------------------------------------------------------- end to end
def test_two_stream_train_step_with_mixup_and_soft_targets():
    import vits_returnftrs as vits
    from mfvit.losses import soft_cross_entropy
    from mfvit.mixup import Mixup, MixTarget
    from oracle import ref_fusion, ref_vit
    fus = importlib.import_module(FUS_MOD)
    depth, B = 2, 4
    backs = []
    for i in range(2):
        m = vits.vit_small(num_classes=3, depth=depth)
        m.load_state_dict(ref_vit.seeded_params(7 + i, num_classes=3, depth=depth))
        backs.append(m.to(DEV).train())
    model = fus.Fus_CrossViT(backs[0], backs[1])
    model.load_state_dict(ref_fusion.seeded_fusion_params(9))
    model = model.to(DEV).train()
    x, xe = rng_tensor(121, (B, 3, 224, 224)), rng_tensor(122, (B, 3, 224, 224))
    target = torch.tensor([1, 2, 0, 1])
    mix = Mixup(mode="elem", label_smoothing=0.1, num_classes=3, erase_prob=0.5).train()
    desc, lam = mix.sample_params(B, 224, 224, torch.Generator().manual_seed(5))
    xm, xem, y = mix(x.to(DEV), target.to(DEV), xe.to(DEV), params=(desc, lam))
    assert isinstance(y, MixTarget) and y.smoothing == 0.1 and y.partner.tolist() == desc[:, 0].tolist() and torch.equal(y.lam.cpu(), lam)
    check_mix(xm, x, desc, lam)
    check_mix(xem, xe, desc, lam)
    # a generator reproduces the batch
    a1, b1, y1 = mix(x.to(DEV), target.to(DEV), xe.to(DEV), generator=torch.Generator().manual_seed(5))
    assert torch.equal(a1, xm) and torch.equal(b1, xem) and torch.equal(y1.lam, y.lam)
    fused, x_c, x_e = model(backs[0], backs[1], xm, xem)
    out = fused + x_c + x_e
    out.retain_grad()
    loss, preds = soft_cross_entropy(out, y)
    loss.backward()
    torch.cuda.synchronize()
    lr, gr = ce_oracle(out.detach().cpu(), target, desc[:, 0], lam, 0.1)
    assert abs(float(loss.detach()) - lr) <= 1e-6 * max(1.0, abs(lr))
    assert rel_err(out.grad, gr) < 1e-6
    assert preds.cpu().tolist() == first_argmax(out.detach().cpu()).tolist()
    for name, mod in (("fusion", model), ("cxr", backs[0]), ("enh", backs[1])):
        grads = [p.grad for p in mod.parameters() if p.grad is not None]
        assert grads, name
        assert all(bool(torch.isfinite(g).all()) for g in grads), name
        assert sum(float(g.abs().sum()) for g in grads) > 0.0, name
    # eval(): the inputs come back untouched, with a plain hard target
    mix.eval()
    xd, xed = x.to(DEV), xe.to(DEV)
    a, b, yh = mix(xd, target.to(DEV), xed)
    assert a.data_ptr() == xd.data_ptr() and b.data_ptr() == xed.data_ptr()
    assert yh.partner is None and yh.lam is None and yh.smoothing == 0.0
