"""Cost of the rollout-finishing stage of a learner section: 32 environments (64 storages), T = 128.

Three forms on the same storages, bootstrap values already in place (every form would copy them alike):
  gae x64   64 cadre_gae launches, one per storage (compute_returns per storage)
  multi     one cadre_gae_multi launch (finish_rollouts, options off)
  scaled    one cadre_return_stats launch + one cadre_gae_multi launch with reward scaling
Each form is timed with HIP events over --iters repetitions after --warmup; the forms are interleaved over --rounds rounds
and the median per-stage time of each form is reported with the spread of its rounds.

    python tools/rollout_finish_overhead.py [--iters 200] [--rounds 7] [--out profiles/rollout_finish_overhead.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cadre_amd import hip
    from ppo_agent.storage import ReturnScaler, RolloutStorage

    N, T = args.envs, args.steps
    g = torch.Generator().manual_seed(1)
    st = []
    for _ in range(2 * N):
        s = RolloutStorage(T, 2, 32, 1, 32, True, 0.99, 0.95)
        s.rewards.copy_(torch.rand(T + 1, 1, generator=g))
        s.value_preds.copy_(torch.randn(T + 1, 1, generator=g) * 0.3)
        s.masks.copy_((torch.rand(T + 1, 1, generator=g) >= 0.05).float())
        s.to("cuda:0")
        s._next.fill_(0.1)
        st.append(s)
    rs = ReturnScaler(N, 0.99, device="cuda:0")
    RolloutStorage.finish_rollouts(st, [0.1] * (2 * N), reward_scaler=rs)          # builds the pointer table
    (table,) = [t for t in RolloutStorage._finish_tables.values()]
    L = hip.lib()
    g32, gt32 = float(np.float32(0.99)), float(np.float32(0.99 * 0.95))
    stream = hip.stream()

    def run(form, n):
        for _ in range(n):
            if form == "gae x64":
                for s in st:
                    hip.check(L.cadre_gae(hip.ptr(s.rewards), hip.ptr(s.value_preds), hip.ptr(s.masks), hip.ptr(s._next),
                                          hip.ptr(s.returns), hip.ptr(s.advantages), 1, T, g32, gt32, 1, stream), "cadre_gae")
                continue
            state = rs.state if form == "scaled" else None
            if state is not None:
                hip.check(L.cadre_return_stats(hip.ptr(table), 2 * N, T, rs.gamma, rs.epsilon, 1, hip.ptr(state),
                                               hip.ptr(rs._scratch), stream), "cadre_return_stats")
            hip.check(L.cadre_gae_multi(hip.ptr(table), 2 * N, T, g32, gt32, 1, hip.ptr(state), rs.clip, stream),
                      "cadre_gae_multi")

    forms = ("gae x64", "multi", "scaled")
    for f in forms:
        run(f, args.warmup)
    torch.cuda.synchronize()
    res = {f: [] for f in forms}
    for _ in range(args.rounds):
        for f in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(f, args.iters)
            e1.record()
            torch.cuda.synchronize()
            res[f].append(1e3 * e0.elapsed_time(e1) / args.iters)
    lines = ["rollout finishing stage, %d environments (%d storages), T = %d (%s, median of %d rounds x %d stages, us per stage)"
             % (N, 2 * N, T, torch.cuda.get_device_name(0), args.rounds, args.iters)]
    base = float(np.median(res["gae x64"]))
    for f in forms:
        v = res[f]
        med = float(np.median(v))
        lines.append("%-8s %9.2f us  (%.3f x gae x64)   min %.2f  max %.2f   rounds: %s"
                     % (f, med, med / base, min(v), max(v), " ".join("%.2f" % x for x in v)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
