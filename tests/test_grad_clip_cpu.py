"""CPU: the references and the host contract of gradient-norm clipping (mfvit.optim.clip_grad_norm_ / grad_norm; tests/grad_clip_ref.py).
  - clip_ref equals torch.nn.utils.clip_grad_norm_ run in float64, for the L2 and the inf norm, the all-zero case, one inf and one NaN;
  - a float32 restatement of the norm pass's row split (head / 16-byte groups / tail) passes the per-tensor gate the GPU test uses, and a
    dropped head, tail or second group of a pair fails it, on the inputs the GPU test uses;
  - the public functions exist and refuse what they cannot do; the C ABI declares the three entry points."""
import math
import os

import pytest
import torch

import grad_clip_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


def counts():
    from oracle import ref_optim
    return list(ref_optim.ADAM_COUNTS) + [3 * ref.CHUNK + 5]


def torch_clip(grads, max_norm, norm_type):
    ps = [torch.nn.Parameter(torch.zeros_like(g, dtype=torch.float64)) for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.double().clone()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=norm_type)
    return total, [p.grad for p in ps]


@pytest.mark.parametrize("norm_type", [2.0, INF], ids=["l2", "inf"])
@pytest.mark.parametrize("case", ["clips", "does_not_clip", "zeros", "one_inf", "nan_last"])
def test_clip_ref_is_torchs_clip_grad_norm_in_float64(case, norm_type):
    grads = ref.inputs([1, 3, 5, 257, 1153, ref.CHUNK + 7])
    if case == "zeros":
        grads = [torch.zeros_like(g) for g in grads]
    elif case == "one_inf":
        grads[3][100] = INF
    elif case == "nan_last":
        grads[-1][-1] = NAN
    base = float(ref.norm_ref(ref.inputs([1, 3, 5, 257, 1153, ref.CHUNK + 7]), norm_type)[1])
    max_norm = 2.0 * base if case == "does_not_clip" else 0.5 * base
    total, coef, per, clipped = ref.clip_ref(grads, max_norm, norm_type)
    t_total, t_grads = torch_clip(grads, max_norm, norm_type)
    torch.testing.assert_close(total, t_total, rtol=1e-12, atol=0, equal_nan=True)
    for a, b in zip(clipped, t_grads):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=0, equal_nan=True)
    for g, n in zip(grads, per):
        torch.testing.assert_close(n, torch.linalg.vector_norm(g.double(), norm_type), rtol=1e-12, atol=0, equal_nan=True)
    if case == "does_not_clip":
        assert float(coef) == 1.0 and all(torch.equal(a, g.double()) for a, g in zip(clipped, grads))
    elif case == "zeros":
        assert float(total) == 0.0 and float(coef) == 1.0
    elif case == "one_inf":
        assert float(total) == INF and float(coef) == 0.0
        assert int(torch.isnan(clipped[3]).sum()) == 1 and bool(torch.isnan(clipped[3][100]))          # inf * 0
        assert all(bool((c[torch.isfinite(g)] == 0).all()) for c, g in zip(clipped, grads))
    elif case == "nan_last":
        assert math.isnan(float(total)) and math.isnan(float(coef)) and all(bool(torch.isnan(c).all()) for c in clipped)
    else:
        assert 0.0 < float(coef) < 1.0


def test_the_gate_passes_the_row_split_and_catches_a_dropped_head_tail_or_second_group():
    """Every tensor of the GPU test's size matrix at every phase (floats behind a 16-byte boundary).  The restatement must pass the per-tensor
    gate everywhere; each mutation must fail it wherever it drops an element at all, the largest tensor included."""
    cs = counts()
    grads = ref.inputs(cs)
    exact = ref.norm_ref(grads)[0]
    worst = 0.0
    caught = {m: 0 for m in ref.MUTATIONS}
    for phase in range(4):
        for i, g in enumerate(grads):
            got, _ = ref.tensor_norm_f32(g, phase)
            e = ref.rel_ratio(torch.tensor(got), exact[i], ref.NORM_RTOL)
            worst = max(worst, e)
            assert e <= 1.0, (phase, cs[i], e)
            for m in ref.MUTATIONS:
                bad, dropped = ref.tensor_norm_f32(g, phase, m)
                if not dropped:
                    assert bad == got
                    continue
                e = ref.rel_ratio(torch.tensor(bad), exact[i], ref.NORM_RTOL)
                assert e > 1.0, (m, phase, cs[i], e)
                caught[m] += 1
                if i == len(cs) - 1:
                    assert e > 3.0, (m, phase, e)                  # 1 / (2 * 49,157) = 1e-5 against a gate of 1.4e-6
    # the largest tensor loses something to every mutation (skip_head: at the phases that have a head)
    assert all(ref.tensor_norm_f32(grads[-1], 1, m)[1] for m in ref.MUTATIONS)
    assert min(caught.values()) >= 20, caught
    assert worst > 0.0            # (the restatement does round: it is not the float64 value)


def test_public_functions_exist_and_refuse_what_they_cannot_do():
    from mfvit import optim
    assert callable(optim.clip_grad_norm_) and callable(optim.grad_norm) and callable(optim._TableOptimizer.clip_grad_norm_)
    ps = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(TypeError, match="optimizer"):
        optim.clip_grad_norm_(ps, 1.0)                                     # a parameter iterable: the tables live on the optimizer
    with pytest.raises(TypeError, match="optimizer"):
        optim.grad_norm(iter(ps))
    opt = optim.Adam(ps)
    with pytest.raises(NotImplementedError, match="torch.nn.utils.clip_grad_norm_"):
        optim.clip_grad_norm_(opt, 1.0, norm_type=3)
    with pytest.raises(NotImplementedError, match="torch.nn.utils.clip_grad_norm_"):
        opt.clip_grad_norm_(1.0, norm_type=1)
    with pytest.raises(NotImplementedError):
        optim.grad_norm(opt, norm_type=0.5)


def test_entry_points_are_declared_and_bound():
    from mfvit import _lib
    text = open(os.path.join(ROOT, "include", "mfvit.h")).read()
    for name in ("mfvit_grad_norm_partials", "mfvit_grad_clip_coef", "mfvit_grad_scale"):
        assert f"int {name}(" in text and name in _lib.SIGNATURES
    assert "torch.nn.utils.clip_grad_norm_" in text
    assert _lib.lib().mfvit_abi_version() == 5
