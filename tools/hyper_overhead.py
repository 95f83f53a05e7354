"""Cost of the device-resident hyper-parameter block on the minibatch step, and of a learning rate that changes.

One step = update_policy_from_storages (gather + the update's hipGraph) + add_gradient + chief_step (clip + Adam graph),
as learner_section runs it, at B = 64 and B = 256 (one worker, 4 command nets, 84x84 agent).  Modes on the same agent and
storages:
  off          today's by-value step
  hp           the `_hp` entry points, block at constant values
  stats        by-value, cadre_ppo_loss_stats + the row copy + cadre_grad_norms (what hp+adaptive contains)
  hp+adaptive  block + stats loss kernel + the KL-adaptive lr controller (desired_kl = 1e-2, lr between 1e-5 and 1e-3)
Each mode is timed with HIP events over --iters steps after --warmup steps (graphs captured during the warm-up); the
modes are interleaved over --rounds rounds and the median per-step time of each mode is reported.  `hp` is meant to cost
nothing: it is compared with the round-to-round spread of `off` in the same run.
Then "lr changes every step" (a new value for each of --lr-iters steps), reported, not gated:
  by value     today's path: every new lr is a new graph key — an eager step, and one more entry kept in the learner
  block        set_hyper (one asynchronous 8-byte copy) + the captured graphs

    python tools/hyper_overhead.py [--iters 200] [--rounds 5] [--out profiles/hyper_overhead.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = ("off", "hp", "stats", "hp+adaptive")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lr-iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ppo_agent.chief import chief_step
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.storage import RolloutStorage
    from tests.helpers import fill_storages
    from tests.test_learner_gpu import make_agent

    lines = ["PPO update step: device-resident hyper-parameters (%s, median of %d rounds x %d steps)"
             % (torch.cuda.get_device_name(0), args.rounds, args.iters)]
    for B in (64, 256):
        agent = make_agent(84, 84)
        shared = Shared_grad_buffers(agent.model_dict, agent.device)
        T = 2 * B
        data = fill_storages(T, 3)
        pair = []
        for hd in ("steer", "throttle"):
            s = RolloutStorage(T, 2, 530, 8, 530, True, 0.99, 0.95)
            for k, v in data[hd].items():
                getattr(s, k).copy_(torch.from_numpy(v))
            s.to("cuda:0")
            s.compute_returns(torch.tensor([0.1]))
            pair.append(s)
        lrn = agent.learner
        rows = torch.zeros(max(args.warmup, args.iters, args.lr_iters), 2, lrn.stats_fields(), device="cuda:0")
        idx = [torch.randperm(T)[:B] for _ in range(8)]

        def step(i, row, lr):
            agent.update_policy_from_storages(
                [(pair[0], idx[i % 8], pair[0].advantages, pair[1], idx[(i + 4) % 8], pair[1].advantages)],
                sync=False, stats_row=row)
            shared.add_gradient(agent.model_dict)
            chief_step(shared, None, 250.0, lr=lr, zero_grads=False)

        def run(mode, n):
            lrn.set_device_hyper(mode.startswith("hp"))
            if mode == "hp+adaptive":
                lrn.set_adaptive_lr(1e-2, lr_min=1e-5, lr_max=1e-3, lr=3e-4)
            stats = mode in ("stats", "hp+adaptive")
            lrn.set_update_modes(stats=stats)
            for i in range(n):
                step(i, rows[i] if stats else None, 3e-4)
            lrn.set_update_modes()
            if mode == "hp+adaptive":
                lrn.set_adaptive_lr(None)

        for mode in MODES:
            run(mode, args.warmup)
        torch.cuda.synchronize()
        res = {m: [] for m in MODES}
        for _ in range(args.rounds):
            for mode in res:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(mode, args.iters)
                e1.record()
                torch.cuda.synchronize()
                res[mode].append(e0.elapsed_time(e1) / args.iters)
        med = {m: float(np.median(v)) for m, v in res.items()}
        spread = 100.0 * (max(res["off"]) - min(res["off"])) / med["off"]
        for mode, v in res.items():
            base = "stats" if mode == "hp+adaptive" else "off"
            lines.append("B=%-4d %-11s  %.4f ms/step  (%+.2f %% vs %s)   rounds: %s"
                         % (B, mode, med[mode], 100.0 * (med[mode] / med[base] - 1.0), base, " ".join("%.4f" % x for x in v)))
        d_hp = 100.0 * (med["hp"] / med["off"] - 1.0)
        lines.append("B=%-4d round-to-round spread of off: %.2f %% (max - min over median); hp vs off: %+.2f %% -> %s"
                     % (B, spread, d_hp, "inside the spread" if d_hp <= spread else "OUTSIDE the spread"))
        # ---- lr changes every step: host time matters here (eager steps), so the window ends in a synchronise
        n = args.lr_iters
        for name, hp in (("by value", False), ("block", True)):
            lrn.set_device_hyper(hp)
            lrn.set_update_modes()
            g0 = len(lrn._graphs)
            lrs = [3e-4 * (1.0 - 0.5 * (i + 1) / n) for i in range(n)]
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(n):
                step(i, None, lrs[i])
            e1.record()
            torch.cuda.synchronize()
            lines.append("B=%-4d lr changes every step, %-8s  %.4f ms/step over %d steps, %d entries added to the learner's graph table"
                         % (B, name, e0.elapsed_time(e1) / n, n, len(lrn._graphs) - g0))
        lrn.set_device_hyper(False)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
