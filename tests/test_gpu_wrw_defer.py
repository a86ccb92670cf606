"""DRL_WRW_DEFER end to end: one grouped fold of the conv weight gradients
at the end of the Ape-X backward instead of one fold behind every layer's
wrw. It keeps the arithmetic, so a learner must reach the same bits with it
on as off, eager and captured; and the deferral must not leak out of its
context."""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GATES = ("DRL_WRW_DEFER",)


class _Gates:
    """Set the gate for a block; the earlier environment comes back."""

    def __init__(self, values):
        self.values = dict(zip(GATES, values))

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in GATES}
        os.environ.update(self.values)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run_learner(graphed, steps=3):
    """Shape of tests/test_gpu_apex_fusions.py::_run_learner, at batch 32."""
    from distributed_rl_amd.algos.ape_x import ApexLearner
    from distributed_rl_amd.config import load_config

    torch.manual_seed(123)
    learner = ApexLearner(load_config("ape_x"), device=DEV, enable_tb=False,
                          batch_size=32, replay_capacity=256)
    g = torch.Generator(device=DEV)
    g.manual_seed(77)
    B = 256
    cols = {
        "state": torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8,
                               device=DEV, generator=g),
        "action": torch.randint(0, 6, (B,), dtype=torch.int32, device=DEV,
                                generator=g),
        "reward": torch.rand(B, device=DEV, generator=g),
        "next_state": torch.randint(0, 256, (B, 4, 84, 84),
                                    dtype=torch.uint8, device=DEV,
                                    generator=g),
        "done": (torch.rand(B, device=DEV, generator=g) < 0.1).float(),
    }
    learner.push_experience(cols, torch.rand(B, device=DEV, generator=g) + 0.1)
    stepper = learner.make_graphed_step() if graphed else learner.step
    for _ in range(steps):
        stepper()
    torch.cuda.synchronize()
    return (learner.mp.flat_mparam.clone(), learner.mp.flat_cparam.clone(),
            [t.clone() for t in learner.optim.sq + learner.optim.ga])


def _same(a, b):
    assert torch.equal(a[0], b[0])  # master params
    assert torch.equal(a[1], b[1])  # compute params
    assert len(a[2]) == len(b[2])
    for x, y in zip(a[2], b[2]):    # optimizer state
        assert torch.equal(x, y)


@pytest.fixture(scope="module")
def eager_ref():
    with _Gates("0"):
        ref = _run_learner(graphed=False)
    # the steps did train: the second-moment state left its zero init
    assert float(ref[2][0].abs().sum()) > 0
    return ref


def test_learner_eager_bit_identical(eager_ref):
    with _Gates("1"):
        got = _run_learner(graphed=False)
    _same(got, eager_ref)


def test_learner_captured_bit_identical():
    with _Gates("0"):
        ref = _run_learner(graphed=True)
    with _Gates("1"):
        got = _run_learner(graphed=True)
    _same(got, ref)
    assert float(ref[2][0].abs().sum()) > 0


def _cnn_and_frames():
    from distributed_rl_amd.config import load_config
    from distributed_rl_amd.models.base_agent import CNN2D

    cfg = load_config("ape_x")
    torch.manual_seed(2)
    info = next(c for c in cfg.model_info.values()
                if str(c.get("netCat", "")).upper() == "CNN2D")
    cnn = CNN2D(info).to(DEV).to(torch.bfloat16).to(
        memory_format=torch.channels_last)
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    s = torch.randint(0, 256, (5, 4, 84, 84), dtype=torch.uint8, device=DEV,
                      generator=g).to(memory_format=torch.channels_last)
    assert cnn._fused_ok(s)
    return cnn, s


def _backward_grads(cnn, s):
    for p in cnn.parameters():
        p.grad = None
    out = cnn(s)
    g = torch.Generator(device=DEV)
    g.manual_seed(8)
    w = torch.randn(out.shape, device=DEV, generator=g).to(out.dtype)
    (out * w).float().sum().backward()
    torch.cuda.synchronize()
    return [p.grad.clone() for p in cnn.parameters()]


def test_plain_backward_folds_at_once():
    """loss.backward() is outside any deferral context: the gate at 1 folds
    every layer where it is produced and gives the gate-at-0 gradients."""
    from distributed_rl_amd import ops

    cnn, s = _cnn_and_frames()
    with _Gates("0"):
        ref = _backward_grads(cnn, s)
    with _Gates("1"):
        got = _backward_grads(cnn, s)
        assert ops._pending_wrw_folds is None
    assert len(ref) == 6  # three convs, weight and bias
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
        assert float(a.float().abs().sum()) > 0


def test_deferred_context_folds_on_exit():
    """Inside the context the three folds are owed; leaving it fills the
    gradients with the bits of the immediate fold."""
    from distributed_rl_amd import ops

    cnn, s = _cnn_and_frames()
    params = list(cnn.parameters())
    with _Gates("0"):
        ref = _backward_grads(cnn, s)
    with _Gates("1"):
        out = cnn(s)
        g = torch.Generator(device=DEV)
        g.manual_seed(8)
        w = torch.randn(out.shape, device=DEV, generator=g).to(out.dtype)
        loss = (out * w).float().sum()
        with ops.deferred_wrw_folds():
            grads = torch.autograd.grad(loss, params)
            assert len(ops._pending_wrw_folds) == 3
        assert ops._pending_wrw_folds is None
        torch.cuda.synchronize()
    for a, b in zip(grads, ref):
        assert torch.equal(a, b)
    # gate off: the context is a no-op and the folds are immediate
    with _Gates("0"):
        out = cnn(s)
        loss = (out * w).float().sum()
        with ops.deferred_wrw_folds():
            grads = torch.autograd.grad(loss, params)
            assert ops._pending_wrw_folds is None
        torch.cuda.synchronize()
    for a, b in zip(grads, ref):
        assert torch.equal(a, b)


def test_deferred_context_error_launches_no_fold(monkeypatch):
    from distributed_rl_amd import ops

    cnn, s = _cnn_and_frames()
    params = list(cnn.parameters())
    launched = []
    monkeypatch.setattr(ops, "_launch_pending_folds",
                        lambda pending: launched.append(len(pending)))
    seen = {}
    with _Gates("1"):
        out = cnn(s)
        loss = out.float().sum()
        with pytest.raises(ZeroDivisionError):
            with ops.deferred_wrw_folds():
                torch.autograd.grad(loss, params)
                seen["list"] = ops._pending_wrw_folds
                seen["owed"] = len(seen["list"])
                raise ZeroDivisionError
    torch.cuda.synchronize()
    assert seen["owed"] == 3
    assert seen["list"] == [] and launched == []
    assert ops._pending_wrw_folds is None
    # and the next backward is whole again
    monkeypatch.undo()
    with _Gates("1"):
        got = _backward_grads(cnn, s)
    with _Gates("0"):
        ref = _backward_grads(cnn, s)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
