"""Time of one imitation step next to the PPO step of the same process and shapes.

One step = the minibatch gather + the update's hipGraph + the clip + Adam graph, at B = 64 and B = 256 (one worker, 4
command nets, 84x84 agent; the encoder does not run):
  ppo   update_policy_from_storages + learner.clip_adam        (cadre_ppo_loss in the update)
  bc    imitate_from_storages       + learner.clip_adam        (cadre_bc_loss in its place; label smoothing 0.1, row weights)
on the same agent, the same storages and the same row indices — the two steps differ by one kernel of the same grid.  Timed
with HIP events over --iters steps after --warmup steps (graphs captured during the warm-up), the modes interleaved over
--rounds rounds; the median per mode, the round-to-round spread of `ppo` and the launch counts (learner.launches) are
reported.  Reads nothing outside the tree.

    python tools/bc_step_bench.py [--iters 200] [--rounds 5] [--out profiles/bc_step.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_agent():
    from cadre_amd import synth
    from ppo_agent.agent import CadreAgent
    fh, fw = synth.feat_hw(84, 84)
    cfg = dict(use_lstm=True, vae_device=0, device_num=0, vae_params="CoPM", measurement_dim=18,
               num_output=dict(steer=33, throttle=3), command_num=4, obs_hw=(84, 84), weights_init="none",
               vae_state_dict=synth.encoder_state(fh, fw, 7))
    steer = {i: (i - 16) / 16.0 for i in range(33)}
    agent = CadreAgent(rank=0, model_cfg=cfg, frame=8, STEER_CONTROL=steer, THROTTLE_CONTROL={0: [0, 0], 1: [0, 1], 2: [0.6, 0]},
                       ent_coeff=0.01, value_coeff=0.1, clip_coeff=1.0, clip=0.1)
    agent.arena.load_numpy_state(synth.ppo_state(11, command_num=4))
    return agent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bc_step_bench needs an MI355X: a time taken elsewhere says nothing")
    from ppo_agent.storage import RolloutStorage
    from tests.helpers import fill_storages

    agent = make_agent()
    lrn = agent.learner
    lines = ["Imitation step next to the PPO step (%s, median of %d rounds x %d steps, same process, same storages)"
             % (torch.cuda.get_device_name(0), args.rounds, args.iters)]
    for B in (64, 256):
        T = 2 * B
        data = fill_storages(T, 3, with_hidden=False)
        pair = []
        for hd in ("steer", "throttle"):
            s = RolloutStorage(T, 2, 530, 8, 530, True, 0.99, 0.95)
            for k, v in data[hd].items():
                getattr(s, k).copy_(torch.from_numpy(v))
            s.to("cuda:0")
            s.compute_returns(torch.tensor([0.1]))
            pair.append(s)
        weights = (torch.rand(T, 1) * 3.75 + 0.25).cuda()
        idx = [torch.randperm(T)[:B] for _ in range(8)]
        launches = {}

        def run(mode, n):
            for i in range(n):
                a, b = idx[i % 8], idx[(i + 4) % 8]
                if mode == "ppo":
                    agent.update_policy_from_storages([(pair[0], a, pair[0].advantages, pair[1], b, pair[1].advantages)], sync=False)
                else:
                    agent.imitate_from_storages([(pair[0], a, weights, pair[1], b, weights)], sync=False, label_smoothing=0.1)
                lrn.clip_adam(lr=3e-4, max_grad_norm=250.0)

        for mode in ("ppo", "bc"):
            run(mode, 1)                                   # (the eager first call of the mode counts its launches)
            launches[mode] = lrn.launches[("all", B)]
            run(mode, args.warmup)
        torch.cuda.synchronize()
        res = {"ppo": [], "bc": []}
        for _ in range(args.rounds):
            for mode in ("ppo", "bc"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(mode, args.iters)
                e1.record()
                torch.cuda.synchronize()
                res[mode].append(e0.elapsed_time(e1) / args.iters)
        med = {m: float(np.median(v)) for m, v in res.items()}
        spread = 100.0 * (max(res["ppo"]) - min(res["ppo"])) / med["ppo"]
        for m in ("ppo", "bc"):
            lines.append("B=%-4d %-3s  %.4f ms/step  (%+.2f %% vs ppo)  launches in the update: %d   rounds: %s"
                         % (B, m, med[m], 100.0 * (med[m] / med["ppo"] - 1.0), launches[m], " ".join("%.4f" % x for x in res[m])))
        d = abs(100.0 * (med["bc"] / med["ppo"] - 1.0))
        lines.append("B=%-4d round-to-round spread of ppo: %.2f %% (max - min over median) -> bc is %s the spread"
                     % (B, spread, "inside" if d <= spread else "OUTSIDE"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
