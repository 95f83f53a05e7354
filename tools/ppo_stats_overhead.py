"""Cost of the PPO update diagnostics and of the armed KL gate on the minibatch step.

One step = update_policy_from_storages (gather + the update's hipGraph) + add_gradient + chief_step (clip + Adam graph),
as learner_section runs it, at B = 64 and B = 256 (one worker, 4 command nets, 84x84 agent: the step does not depend on
the frame size).  Three modes on the same agent and storages:
  off    today's launches
  stats  cadre_ppo_loss_stats + the row copy + cadre_grad_norms
  gate   stats + target_kl = 1e9 (armed, never fires: the gated optimiser entry point)
Each mode is timed with HIP events over --iters steps after --warmup steps (graphs captured during the warm-up); the
modes are interleaved over --rounds rounds and the median per-step time of each mode is reported.

    python tools/ppo_stats_overhead.py [--iters 200] [--rounds 5] [--out profiles/ppo_stats_overhead.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ppo_agent.chief import chief_step
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.storage import RolloutStorage
    from tests.helpers import fill_storages
    from tests.test_learner_gpu import make_agent

    lines = ["PPO update step: diagnostics / KL gate overhead (%s, median of %d rounds x %d steps)"
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
        F = lrn.stats_fields()
        rows = torch.zeros(args.warmup + args.iters, 2, F, device="cuda:0")
        idx = [torch.randperm(T)[:B] for _ in range(8)]

        def run(mode, n):
            if mode == "off":
                lrn.set_update_modes()
            else:
                lrn.set_update_modes(stats=True, target_kl=1e9 if mode == "gate" else None)
            for i in range(n):
                row = None if mode == "off" else rows[i]
                agent.update_policy_from_storages(
                    [(pair[0], idx[i % 8], pair[0].advantages, pair[1], idx[(i + 4) % 8], pair[1].advantages)],
                    sync=False, stats_row=row)
                shared.add_gradient(agent.model_dict)
                chief_step(shared, None, 250.0, zero_grads=False)
            lrn.set_update_modes()

        for mode in ("off", "stats", "gate"):
            run(mode, args.warmup)
        torch.cuda.synchronize()
        res = {m: [] for m in ("off", "stats", "gate")}
        for _ in range(args.rounds):
            for mode in res:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(mode, args.iters)
                e1.record()
                torch.cuda.synchronize()
                res[mode].append(e0.elapsed_time(e1) / args.iters)
        base = float(np.median(res["off"]))
        for mode, v in res.items():
            med = float(np.median(v))
            lines.append("B=%-4d %-5s  %.4f ms/step  (%+.2f %% vs off)   rounds: %s"
                         % (B, mode, med, 100.0 * (med / base - 1.0), " ".join("%.4f" % x for x in v)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
