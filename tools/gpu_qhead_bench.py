"""Microbench of the fused q-head loss op (forward + backward) at B = 512.

  A = 18: the any-A kernels against what the learner ran for A = 18 before
          them: three pairs of F.linear heads, ops.dueling_nstep_dqn_loss
          and its autograd backward, on the same hidden rows.
  A = 6:  DRL_QHEAD_ANY=1 against the compile-time (512, 6) kernels.

The arms alternate inside one process; every round times ITERS calls of
each arm between device events; reported: the median of the rounds and the
spread (max - min), in microseconds per call. One JSON line per comparison.
"""

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from distributed_rl_amd import ops

DEV = "cuda:0"
B, HH = 512, 512
ROUNDS, ITERS, WARM = 3, 200, 20


def make(A):
    g = torch.Generator(device=DEV)
    g.manual_seed(A)

    def bf(*shape, scale=1.0):
        return (torch.randn(*shape, device=DEV, generator=g) * scale).to(
            torch.bfloat16)

    def heads():
        return [bf(A, HH, scale=0.05), bf(A, scale=0.1),
                bf(1, HH, scale=0.05), bf(1, scale=0.1)]

    leaves = [t.requires_grad_(True) for t in [bf(B, 2 * HH)] + heads()]
    consts = [bf(B, 2 * HH), bf(B, 2 * HH)] + heads()
    rows = [torch.randint(0, A, (B,), device=DEV, generator=g),
            torch.randn(B, device=DEV, generator=g),
            (torch.rand(B, device=DEV, generator=g) < 0.1).float(),
            torch.rand(B, device=DEV, generator=g) + 0.5]
    return leaves, consts, rows


def fused(leaves, consts, rows):
    def call():
        loss, _, _ = ops.dueling_q_head_loss(
            *leaves, *consts, *rows, 0.99, 3, 0.6, pre_act=True)
        torch.autograd.grad(loss, leaves)
    return call


def composed(leaves, consts, rows):
    """The learner's _fast_heads branch from the hidden rows on (the ReLU of
    the hidden layer is part of its w1 epilogue there, a clamp here)."""
    h_s, wa, ba, wv, bv = leaves
    h_on, h_tg, wat, bat, wvt, bvt = consts

    def heads(h, w_a, b_a, w_v, b_v):
        h = F.relu(h)
        return F.linear(h[:, :HH], w_a, b_a), F.linear(h[:, HH:], w_v, b_v)

    def call():
        adv_s, val_s = heads(h_s, wa, ba, wv, bv)
        with torch.no_grad():
            adv_on, val_on = heads(h_on, wa, ba, wv, bv)
            adv_tg, val_tg = heads(h_tg, wat, bat, wvt, bvt)
        loss, _, _ = ops.dueling_nstep_dqn_loss(
            adv_s.float(), val_s.float(), adv_on.float(), val_on.float(),
            adv_tg.float(), val_tg.float(), *rows, 0.99, 3, 0.6)
        torch.autograd.grad(loss, leaves)
    return call


def with_gate(value, call):
    def gated():
        os.environ["DRL_QHEAD_ANY"] = value
        call()
    return gated


def time_us(call):
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(ITERS):
        call()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / ITERS


def compare(name, arms):
    for call in arms.values():
        for _ in range(WARM):
            call()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, call in arms.items():
            times[k].append(time_us(call))
    out = {"case": name, "B": B, "rounds": ROUNDS, "iters": ITERS}
    for k, ts in times.items():
        ts = sorted(ts)
        out[k] = {"median_us": round(ts[len(ts) // 2], 2),
                  "spread_us": round(ts[-1] - ts[0], 2)}
    print(json.dumps(out), flush=True)


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    ops.hip_ext(required=True)
    t18, t6 = make(18), make(6)
    compare("A=18 any-A kernels vs linear heads + dueling loss",
            {"any": fused(*t18), "composed": composed(*t18)})
    compare("A=6 DRL_QHEAD_ANY=1 vs unset",
            {"any": with_gate("1", fused(*t6)),
             "fixed": with_gate("0", fused(*t6))})
    os.environ.pop("DRL_QHEAD_ANY", None)


if __name__ == "__main__":
    main()
