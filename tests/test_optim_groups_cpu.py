"""CPU: host logic of layer-wise learning-rate decay and ModelEma (mfvit.optim.param_groups_layer_decay, mfvit.schedules.adjust_learning_rate,
mfvit.optim.ModelEma) and the references of tests/test_optim_groups_gpu.py (tests/optim_groups_ref.py): pinned to torch.optim.AdamW / SGD built
from the same groups, and shown to fail the GPU test's gate when every row takes its neighbour's hyper entry."""
import importlib
import math

import pytest
import torch

import optim_groups_ref as ref
from test_optim_kernels_gpu import ADAM_ATOL, ADAM_RTOL       # the gate of the GPU tests (importing the module needs no GPU)

FUS_MOD = ("model.crossvit_2vits_2additionaloutputs_changenormlayer_location_removeextralclayer_"
           "changemodelinputlocation_std002_sum")
D = ref.LAYER_DECAY
BLOCK_DECAY = ["attn.qkv.weight", "attn.proj.weight", "mlp.fc1.weight", "mlp.fc2.weight"]
BLOCK_NO_DECAY = ["norm1.weight", "norm1.bias", "attn.qkv.bias", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.bias", "mlp.fc2.bias"]


def small_vit(**kw):
    from mfvit.encoder import VisionTransformerMoCo
    return VisionTransformerMoCo(depth=3, embed_dim=384, num_heads=12, img_size=32, num_classes=3, **kw)


def expected_map(stop_grad_conv1=False):
    """(layer id, lr scale, decays?, names) of every group of a depth-3 encoder, written out: 5 layer ids, scales d^4 .. 1."""
    rows = []
    if not stop_grad_conv1:
        rows.append((0, D ** 4, True, ["patch_embed.proj.weight"]))
    rows.append((0, D ** 4, False, ["cls_token"] + ([] if stop_grad_conv1 else ["patch_embed.proj.bias"])))
    for i, scale in enumerate((D ** 3, D ** 2, D)):
        rows.append((i + 1, scale, True, [f"blocks.{i}.{n}" for n in BLOCK_DECAY]))
        rows.append((i + 1, scale, False, [f"blocks.{i}.{n}" for n in BLOCK_NO_DECAY]))
    rows.append((4, 1.0, True, ["head.weight"]))
    rows.append((4, 1.0, False, ["norm.weight", "norm.bias", "head.bias"]))
    return rows


def check_vit_groups(groups, model, lr, wd, stop_grad_conv1):
    want = expected_map(stop_grad_conv1)
    assert len(groups) == len(want)
    named = dict(model.named_parameters())
    for g, (layer, scale, decays, names) in zip(groups, want):
        assert g["layer_id"] == layer and g["lr_scale"] == scale and g["lr"] == lr * scale
        assert g["weight_decay"] == (wd if decays else 0.0)
        assert g["param_names"] == names and len(g["params"]) == len(names)
        assert all(p is named[n] for p, n in zip(g["params"], names))
        assert set(g) == {"params", "lr", "lr_scale", "weight_decay", "layer_id", "param_names"}


@pytest.mark.parametrize("stop", [False, True], ids=["all_trainable", "stop_grad_conv1"])
def test_layer_map_of_a_depth_3_encoder(stop):
    from mfvit import optim
    m = small_vit(stop_grad_conv1=stop)
    groups = optim.param_groups_layer_decay(m, 1e-3, weight_decay=0.05, layer_decay=D)
    check_vit_groups(groups, m, 1e-3, 0.05, stop)
    assert sorted({g["layer_id"] for g in groups}) == [0, 1, 2, 3, 4]
    listed = [n for g in groups for n in g["param_names"]]
    assert "pos_embed" not in listed and (not stop or not any(n.startswith("patch_embed") for n in listed))
    trainable = [n for n, p in m.named_parameters() if p.requires_grad]
    assert sorted(listed) == sorted(trainable) and len(set(listed)) == len(listed)             # every trainable parameter exactly once
    ids = [id(p) for g in groups for p in g["params"]]
    assert len(set(ids)) == len(ids)


def test_lora_tensors_follow_their_block_and_frozen_parameters_are_skipped():
    from mfvit import lora, optim
    m = small_vit()
    lora.add_lora(m, rank=4, targets=("q", "proj"), blocks=[1])
    groups = optim.param_groups_layer_decay(m, 1e-3)
    by_name = {n: g for g in groups for n in g["param_names"]}
    assert sorted(by_name) == sorted(n for n, p in m.named_parameters() if p.requires_grad)
    adapters = [n for n in by_name if "lora_" in n]
    assert len(adapters) == 4 and all(n.startswith("blocks.1.") and by_name[n]["layer_id"] == 2 and by_name[n]["lr_scale"] == D ** 2 for n in adapters)
    assert all(by_name[n]["weight_decay"] == 0.05 for n in adapters)                           # 2-D tensors: they decay
    assert by_name["head.weight"]["layer_id"] == 4 and not any(n.startswith("blocks.0.") for n in by_name)


def test_two_stream_map_fusion_at_scale_one_and_equal_encoders():
    from mfvit import optim
    fus = importlib.import_module(FUS_MOD)
    a, b = small_vit(stop_grad_conv1=True), small_vit(stop_grad_conv1=True)
    f = fus.Fus_CrossViT(a, b)
    groups = optim.param_groups_layer_decay([f, a, b], 2e-3, weight_decay=0.1, layer_decay=D)
    nf = 2
    assert [g["layer_id"] for g in groups[:nf]] == [None, None] and all(g["lr_scale"] == 1.0 and g["lr"] == 2e-3 for g in groups[:nf])
    assert [g["weight_decay"] for g in groups[:nf]] == [0.1, 0.0]
    fused = [n for g in groups[:nf] for n in g["param_names"]]
    assert sorted(fused) == sorted(n for n, _ in f.named_parameters()) and len(fused) == 22
    per = (len(groups) - nf) // 2
    assert len(groups) == nf + 2 * per
    check_vit_groups(groups[nf:nf + per], a, 2e-3, 0.1, True)
    check_vit_groups(groups[nf + per:], b, 2e-3, 0.1, True)
    # plain values: an optimizer state dict over these groups pickles, and torch.optim.AdamW takes the groups as they are
    import pickle
    pickle.loads(pickle.dumps(torch.optim.AdamW(groups).state_dict()))


# ------------------------------------------------------------------------------------------------ the reference, pinned to torch.optim
PIN_COUNTS = [5, 1153, ref.CHUNK + 7, 3, 2 * ref.CHUNK, 257, 64, 1027, 6]      # nine tensors, two of them over several table rows


def _pin_setup():
    from conftest import rng_tensor
    P = [rng_tensor(8100 + i, (c,), dtype=torch.float64) for i, c in enumerate(PIN_COUNTS)]
    grads = [[rng_tensor(8200 + 10 * s + i, (c,), dtype=torch.float64) for i, c in enumerate(PIN_COUNTS)] for s in range(3)]
    rows = ref.rows_of(PIN_COUNTS)
    group_of = {i: k for k, idx in enumerate(ref.SIX_GROUPS) for i in idx}
    return P, grads, rows, [group_of[t] for t, _, _ in rows]


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_row_by_row_adam_reference_equals_torch_on_the_same_groups(decoupled):
    from mfvit.schedules import adjust_learning_rate
    P, grads, rows, entry_of_row = _pin_setup()
    params = [torch.nn.Parameter(p.clone()) for p in P]
    groups = ref.six_groups(params)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(groups, lr=ref.BASE_LR, betas=(0.9, 0.999), eps=1e-8)
    M, V = [torch.zeros_like(p) for p in P], [torch.zeros_like(p) for p in P]
    for s, epoch in enumerate(ref.SCHEDULE_EPOCHS):
        adjust_learning_rate(opt, epoch, ref.BASE_LR, ref.EPOCHS, ref.WARMUP)
        entries = [dict(lr=g["lr"], beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=g["weight_decay"], decoupled=decoupled, step=s + 1)
                   for g in opt.param_groups]
        assert len({e["lr"] for e in entries}) == 6
        P, M, V = ref.adam_rows_ref(rows, entry_of_row, entries, P, grads[s], M, V)
        for p, g in zip(params, grads[s]):
            p.grad = g.clone()
        opt.step()
        for i, p in enumerate(params):
            assert ref.rel(P[i], p.detach()) < ref.PIN
            assert ref.rel(M[i], opt.state[p]["exp_avg"]) < ref.PIN
            assert ref.rel(V[i], opt.state[p]["exp_avg_sq"]) < ref.PIN


@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_row_by_row_sgd_reference_equals_torch_on_the_same_groups(momentum):
    from mfvit.schedules import adjust_learning_rate
    P, grads, rows, entry_of_row = _pin_setup()
    params = [torch.nn.Parameter(p.clone()) for p in P]
    opt = torch.optim.SGD(ref.six_groups(params), lr=ref.BASE_LR, momentum=momentum)
    B = [torch.zeros_like(p) for p in P]
    for s, epoch in enumerate(ref.SCHEDULE_EPOCHS):
        adjust_learning_rate(opt, epoch, ref.BASE_LR, ref.EPOCHS, ref.WARMUP)
        entries = [dict(lr=g["lr"], momentum=momentum, weight_decay=g["weight_decay"]) for g in opt.param_groups]
        assert len({e["lr"] for e in entries}) == 6                            # the schedule kept every group's own scale
        P, B = ref.sgd_rows_ref(rows, entry_of_row, entries, P, grads[s], B)
        for p, g in zip(params, grads[s]):
            p.grad = g.clone()
        opt.step()
        for i, p in enumerate(params):
            assert ref.rel(P[i], p.detach()) < ref.PIN
            if momentum:
                assert ref.rel(B[i], opt.state[p]["momentum_buffer"]) < ref.PIN


def test_gate_sees_a_row_that_took_its_neighbours_entry():
    """Layer-decay groups of the depth-3 encoder: neighbouring layers differ by 25 % in lr, the two groups of a layer in weight decay.  With every
    row's entry index off by one, every group leaves the Adam gate of tests/test_optim_groups_gpu.py: a group that lands on its layer's other
    group (the same lr, no weight decay) by lr * wd * |p|, one that lands on the next layer by a quarter of its update."""
    from conftest import rng_tensor
    from mfvit import optim
    from oracle import ref_optim
    m = small_vit()
    groups = optim.param_groups_layer_decay(m, 1e-3, weight_decay=0.05, layer_decay=D)
    counts = [p.numel() for g in groups for p in g["params"]]
    group_of_tensor = [k for k, g in enumerate(groups) for _ in g["params"]]
    rows = ref.rows_of(counts)
    entry_of_row = [group_of_tensor[t] for t, _, _ in rows]
    entries = ref.entries_of_groups(groups, [1] * len(groups))
    P = [rng_tensor(8300 + i, (c,), scale=0.1) for i, c in enumerate(counts)]
    G = [rng_tensor(8400 + i, (c,), scale=0.01) for i, c in enumerate(counts)]
    Z = [torch.zeros_like(p) for p in P]
    good = ref.adam_rows_ref(rows, entry_of_row, entries, P, G, Z, Z)[0]
    bad = ref.adam_rows_ref(rows, entry_of_row, entries, P, G, Z, Z, shift=1)[0]
    worst = {}
    for t, k in enumerate(group_of_tensor):
        assert ref_optim.gate_ratio(good[t].float(), good[t], ADAM_RTOL, ADAM_ATOL) <= 1.0        # float32 storage of the right answer passes
        worst[k] = max(worst.get(k, 0.0), ref_optim.gate_ratio(bad[t].float(), good[t], ADAM_RTOL, ADAM_ATOL))
    assert len(worst) == len(groups) and min(worst.values()) > 1.0, worst
    assert min(worst[k] for k in range(1, len(groups), 2)) > 100.0, worst                           # another lr: far outside


# ------------------------------------------------------------------------------------------------ schedule
class _Groups:
    def __init__(self, groups):
        self.param_groups = groups


@pytest.mark.parametrize("kw", [dict(cos=True), dict(cos=False, schedule=(3, 6))], ids=["cosine", "milestones"])
def test_schedule_scales_groups_that_carry_lr_scale_and_no_others(kw):
    from mfvit.schedules import adjust_learning_rate
    scales = [D ** 4, D, 1.0]
    for epoch in (0.0, 0.5, 1.999, 2.0, 3.0, 5.5, 6.0, 7.25, 9.99):                 # warm-up, its end, cosine; both sides of each milestone
        want = ref.lr_at(epoch, 0.03, 10, 2, **kw)
        plain = _Groups([{"lr": -1.0}, {"lr": -1.0, "weight_decay": 0.1}])
        assert adjust_learning_rate(plain, epoch, 0.03, 10, 2, **kw) == want
        assert [g["lr"] for g in plain.param_groups] == [want, want]                # without the key: the value itself, not a product
        assert all("lr_scale" not in g for g in plain.param_groups)
        mixed = _Groups([{"lr": -1.0, "lr_scale": s} for s in scales] + [{"lr": -1.0}])
        assert adjust_learning_rate(mixed, epoch, 0.03, 10, 2, **kw) == want        # returns the unscaled value
        assert [g["lr"] for g in mixed.param_groups] == [want * s for s in scales] + [want]
    assert adjust_learning_rate(None, 3.0, 0.03, 10, 2, **kw) == ref.lr_at(3.0, 0.03, 10, 2, **kw)
    assert ref.lr_at(1.0, 0.03, 10, 2) == 0.015 and ref.lr_at(10.0, 0.03, 10, 2) == 0.0 and math.isclose(ref.lr_at(6.0, 0.03, 10, 2), 0.015)


# ------------------------------------------------------------------------------------------------ ModelEma host logic
def test_model_ema_decay_sequence_copies_and_refusals():
    from mfvit import optim
    m = small_vit()
    ema = optim.ModelEma(m, decay=0.9998, warmup=True)
    assert [ema.decay_at(t) for t in range(21)] == [min(0.9998, (1.0 + t) / (10.0 + t)) for t in range(21)]
    assert ema.decay_at(0) == 0.1 and ema.decay_at(20) == 0.7 and ema.decay_at(10 ** 6) == 0.9998
    const = optim.ModelEma(m, decay=0.99)
    assert [const.decay_at(t) for t in range(21)] == [0.99] * 21
    assert ema.module is ema.modules[0] and ema.module is not m and not ema.module.training and m.training
    assert not any(p.requires_grad for p in ema.module.parameters()) and any(p.requires_grad for p in m.parameters())
    assert ema.module._arena_intact() and ema.module.flat_parameters().data_ptr() != m.flat_parameters().data_ptr()
    assert all(torch.equal(a, b) for a, b in zip(ema.module.state_dict().values(), m.state_dict().values()))
    sd = ema.state_dict()
    assert sd["t"] == 0 and len(sd["modules"]) == 1 and list(sd["modules"][0]) == list(m.state_dict())
    sd["t"] = 7
    const.load_state_dict(sd)
    assert const.t == 7
    with pytest.raises(TypeError, match="flat arena"):
        optim.ModelEma(torch.nn.Linear(4, 3))
    with pytest.raises(ValueError):
        optim.ModelEma([])
    # copied together: the copy of a Fus_CrossViT drives the copies of its encoders
    fus = importlib.import_module(FUS_MOD)
    a, b = small_vit(), small_vit()
    three = optim.ModelEma([fus.Fus_CrossViT(a, b), a, b])
    assert three.modules[0].vit_features_cxr.__self__ is three.modules[1] and three.modules[0].vit_features_enh.__self__ is three.modules[2]
    with pytest.raises(ValueError, match="3 modules"):
        three.update([a, b])


def test_group_entries_are_declared_and_refuse_bad_arguments_without_a_gpu():
    """The MFVIT_EINVAL cases return before any HIP call, so they hold on a host without a GPU too."""
    import ctypes
    from mfvit import _lib
    h = _lib.lib()
    assert ctypes.sizeof(_lib.AdamGroup) == 32 and ctypes.sizeof(_lib.SgdGroup) == 16 and _lib.OPTIM_GROUPS_PER_LAUNCH == ref.CAP
    table = (ctypes.c_int64 * 7)()
    ok = ref.adam_hyper(ref.adam_entries(2, True))
    addr = ctypes.addressof(table)
    assert h.mfvit_adam_step_groups(None, 1, ok, 2, None) == ref.EINVAL
    assert h.mfvit_adam_step_groups(addr, 1, None, 2, None) == ref.EINVAL
    assert h.mfvit_adam_step_groups(addr, 0, ok, 2, None) == ref.EINVAL
    assert h.mfvit_adam_step_groups(addr, 1, ok, 0, None) == ref.EINVAL
    ok[1].step = 0
    assert h.mfvit_adam_step_groups(addr, 1, ok, 2, None) == ref.EINVAL
    sg = ref.sgd_hyper(ref.sgd_entries(2, 0.9))
    assert h.mfvit_sgd_step_groups(None, 1, sg, 2, None) == ref.EINVAL
    assert h.mfvit_sgd_step_groups(addr, 1, None, 2, None) == ref.EINVAL
    assert h.mfvit_sgd_step_groups(addr, -1, sg, 2, None) == ref.EINVAL
    assert h.mfvit_sgd_step_groups(addr, 1, sg, -1, None) == ref.EINVAL
    assert h.mfvit_abi_version() == 5                            # additive
