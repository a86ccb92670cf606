#!/usr/bin/env python
"""Measurements behind profiles/r10_resconv_any_hw.md.

  kernels  cost of run-time H, W: event-timed binding calls at --images on
           the five table geometries and the stem, table kernel and
           run-time kernel (any_hw / the _hw bindings) alternating.
  torso    what a user gets: forward+backward of the bf16 channels_last
           torso at 64x64 and 72x96, own path (gates default, and with
           DRL_OWN_STEM=1) against DRL_OWN_RESCONV=0 DRL_OWN_POOL=1. The
           gates are read per call, so the arms alternate in one process.

Per arm: --rounds rounds of --iters timed calls after --warmup; one median
per round; reported as the median of the round medians and their spread
(max - min). r06's rule: a difference counts only if it exceeds three times
the larger spread. One JSON line per comparison.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
BF16 = torch.bfloat16


def _cl(*shape):
    return torch.randn(*shape, device=DEV).to(BF16).contiguous(
        memory_format=torch.channels_last)


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)  # us
    return statistics.median(times)


def _compare(name, arms, args):
    """arms: {label: fn}; alternates them round by round."""
    meds = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            meds[k].append(_time(fn, args.warmup, args.iters))
    res = {"case": name}
    for k, v in meds.items():
        res[k] = {"median_us": round(statistics.median(v), 2),
                  "spread_us": round(max(v) - min(v), 2),
                  "rounds_us": [round(t, 2) for t in v]}
    print(json.dumps(res), flush=True)
    return res


def kernels(args):
    from distributed_rl_amd.ops import hip_ext

    ext = hip_ext(required=True)
    n = args.images
    e = torch.empty(0, device=DEV, dtype=BF16)
    geoms = [(42, 42, 16, 16), (42, 42, 16, 32), (21, 21, 32, 32),
             (11, 11, 32, 32), (42, 42, 32, 16)]
    for H, W, C, COUT in geoms:
        x, w = _cl(n, C, H, W), _cl(COUT, C, 3, 3)
        b = torch.randn(COUT, device=DEV).to(BF16)
        out, g = _cl(n, COUT, H, W), _cl(n, COUT, H, W)
        tag = f"{H}x{W}x{C}->{COUT}"
        _compare(f"fwd {tag}", {
            "table": lambda: ext.conv3x3p1_fwd(x, w, b, e, out, True, True),
            "runtime": lambda: ext.conv3x3p1_fwd(x, w, b, e, out, True, True,
                                                 any_hw=True)}, args)
        # masked input gradient of the (COUT -> C) conv this mirrors
        wd, gx = _cl(C, COUT, 3, 3), _cl(n, COUT, H, W)
        ws = torch.empty(wd.numel(), device=DEV, dtype=BF16)
        _compare(f"dgrad(masked) {tag}", {
            "table": lambda: ext.conv3x3p1_dgrad(x, wd, ws, gx, out),
            "runtime": lambda: ext.conv3x3p1_dgrad(x, wd, ws, gx, out,
                                                   any_hw=True)}, args)
        if ext.conv3x3p1_wrw_supported(H, W, C, COUT):
            gw = torch.empty(COUT, 9 * C, device=DEV, dtype=BF16)
            gb = torch.empty(COUT, device=DEV, dtype=BF16)
            _compare(f"wrw {tag}", {
                "table": lambda: ext.conv3x3p1_wrw(x, g, gw, gb, True),
                "runtime": lambda: ext.conv3x3p1_wrw(x, g, gw, gb, True,
                                                     any_hw=True)}, args)
    x, w = _cl(n, 4, 84, 84), _cl(16, 4, 3, 3)
    b = torch.randn(16, device=DEV).to(BF16)
    out, g = _cl(n, 16, 84, 84), _cl(n, 16, 84, 84)
    gw = torch.empty(16, 36, device=DEV, dtype=BF16)
    gb = torch.empty(16, device=DEV, dtype=BF16)
    _compare("stem fwd 84x84x4->16", {
        "table": lambda: ext.conv3x3c4_fwd(x, w, b, out),
        "runtime": lambda: ext.conv3x3c4_fwd_hw(x, w, b, out)}, args)
    _compare("stem wrw 84x84x4->16", {
        "table": lambda: ext.conv3x3c4_wrw(x, g, gw, gb),
        "runtime": lambda: ext.conv3x3c4_wrw_hw(x, g, gw, gb)}, args)


GATES = ("DRL_OWN_RESCONV", "DRL_OWN_RESCONV_WRW", "DRL_OWN_RESCONV_DGRAD",
         "DRL_OWN_STEM", "DRL_OWN_STEM_WRW", "DRL_OWN_POOL")


def torso(args):
    from distributed_rl_amd.models.base_agent import ImpalaResNet

    torch.manual_seed(0)
    net = ImpalaResNet(dict(iSize=4, channels=[16, 32, 32], nBlocks=2)).to(
        DEV).to(memory_format=torch.channels_last).to(BF16)
    params = list(net.parameters())

    def arm(env):
        def run():
            for gate in GATES:
                os.environ.pop(gate, None)
            os.environ.update(env)
            y = net(x)
            torch.autograd.grad(y.float().square().sum(), params)
        return run

    for H, W in [(64, 64), (72, 96)]:
        x = _cl(args.images, 4, H, W)
        _compare(f"torso fwd+bwd {H}x{W} n={args.images}", {
            "own": arm({}),
            "own+stem": arm({"DRL_OWN_STEM": "1"}),
            "library_convs": arm({"DRL_OWN_RESCONV": "0",
                                  "DRL_OWN_POOL": "1"})}, args)
    for gate in GATES:
        os.environ.pop(gate, None)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("what", choices=["kernels", "torso", "all"])
    ap.add_argument("--images", type=int, default=1344)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.what in ("kernels", "all"):
        kernels(a)
    if a.what in ("torso", "all"):
        torso(a)
