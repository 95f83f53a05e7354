"""Cost of the weight average: the minibatch step with and without it, and cadre_ema_update alone against the stream-copy rate.

The minibatch step at B = 64 and B = 256 (84x84 agent, 4 command nets): the update's hipGraph followed by the optimiser step's
hipGraph on one packed minibatch, replayed --steps times between two HIP events; the two forms — no average set (the launches
of the step as it is without the module) and an average set (cadre_ema_update's three launches in the optimiser graph) —
alternate round by round in ONE process on ONE agent, the median round of each is reported.

cadre_ema_update alone on the shipped arena (12 bytes per element: read p, read e, write e) between two HIP events over
--reps calls, next to cadre_hbm_stream's copy (peaks.hip; 8 bytes per element) on 1 GiB buffers and on buffers of the arena's
size, measured in the same process.  Reported, not gated.

    python tools/average_bench.py [--steps 200] [--rounds 7] [--reps 200] [--out profiles/average_latency.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                      # ms per call


def step_times(agent, avg, B, steps, rounds):
    from tests.test_ppo_stats_gpu import dev, samples
    lrn = agent.learner
    smp = samples(B, 4, 1)
    w = lrn.workspace(B)
    agent._pack(w, 0, dev(smp[0]))
    agent._pack(w, 1, dev(smp[1]))

    def step():
        lrn.update(B, 1.0 / B)
        lrn.clip_adam(lr=1e-5, max_grad_norm=250.0)
    for mode in (False, True):
        lrn.set_weight_average(avg if mode else None)
        for _ in range(4):                              # eager run, capture, replays
            step()
    torch.cuda.synchronize()
    res = {False: [], True: []}
    for r in range(rounds):
        for mode in ((False, True) if r % 2 == 0 else (True, False)):
            lrn.set_weight_average(avg if mode else None)
            res[mode].append(_events(step, steps))
    lrn.set_weight_average(None)
    return res


def kernel_times(agent, avg, reps):
    from cadre_amd import hip
    L = hip.lib()
    n = int(agent.arena.total)
    out = {}
    avg.update()
    torch.cuda.synchronize()
    out["ema"] = min(_events(avg.update, reps) for _ in range(3))
    sink = torch.zeros(4, device="cuda")
    for name, m in (("copy_arena", n), ("copy_1GiB", 1 << 28)):
        a = torch.empty(m, device="cuda").normal_()
        b = torch.empty_like(a)
        fn = lambda: hip.check(L.cadre_hbm_stream(1, hip.ptr(a), hip.ptr(b), 4 * m, hip.ptr(sink), hip.stream()), "cadre_hbm_stream")
        fn()
        torch.cuda.synchronize()
        out[name] = (min(_events(fn, max(5, reps // (1 + m // n))) for _ in range(3)), m)
        del a, b
    return out, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("average_bench: no HIP device; the numbers of this tool are GPU times")
    from cadre_amd.average import WeightAverage
    from tests.test_learner_gpu import make_agent
    agent = make_agent(84, 84)
    avg = WeightAverage(agent, decay=0.999)
    lines = ["Weight average (%s), arena of %d floats" % (torch.cuda.get_device_name(0), agent.arena.total)]
    for B in (64, 256):
        res = step_times(agent, avg, B, args.steps, args.rounds)
        med = {m: float(np.median(v)) for m, v in res.items()}
        lines.append("PPO minibatch step (update graph + optimiser graph), B = %d, median of %d alternating rounds x %d replayed steps, HIP events"
                     % (B, args.rounds, args.steps))
        for mode, name in ((False, "no average"), (True, "average set")):
            lines.append("  %-12s %.4f ms/step   rounds: %s" % (name, med[mode], " ".join("%.4f" % x for x in res[mode])))
        lines.append("  difference: %+.1f us/step (%+.2f %%); round-to-round spread without the average: %.2f %%"
                     % (1e3 * (med[True] - med[False]), 100.0 * (med[True] / med[False] - 1.0),
                        100.0 * (max(res[False]) - min(res[False])) / med[False]))
    kt, n = kernel_times(agent, avg, args.reps)
    ema_rate = 12.0 * n / (kt["ema"] * 1e-3)
    lines.append("cadre_ema_update alone (3 launches, %d bytes), best of 3 x %d calls: %.1f us, %.0f GB/s" % (12 * n, args.reps, 1e3 * kt["ema"], ema_rate / 1e9))
    for name in ("copy_arena", "copy_1GiB"):
        t, m = kt[name]
        rate = 8.0 * m / (t * 1e-3)
        lines.append("  cadre_hbm_stream copy of %d floats (%d bytes moved): %.1f us, %.0f GB/s; the average runs at %.2f of it"
                     % (m, 8 * m, 1e3 * t, rate / 1e9, ema_rate / rate))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
