"""Cost of the ordinal policy heads (model_cfg["ordinal_policy"]) on the minibatch step and on act().

One step = update_policy_from_storages (gather + the update's hipGraph) + add_gradient + chief_step (clip + Adam graph), as
learner_section runs it, at B = 64 and B = 256 (one worker, 4 command nets, 84x84 agent), and one act() (eager launch
chain, including its host-side copies and its one host sync).  Two agents in the same process, same weights and storages:
  off   built without the key: today's launch chain (cadre_ppo_loss, cadre_sample)
  on    ordinal_policy=True: cadre_ppo_loss_ord / cadre_sample_ord with the rank tables of the control tables
The step is timed with HIP events over --iters steps after --warmup steps (graphs captured during the warm-up), act() with
the host clock around --act-iters synchronised calls; the modes are interleaved over --rounds rounds, the median per mode
is reported and the round-to-round spread of `off` is printed beside it.

--off-only: time `off` alone (runs on a tree that does not have the key: the parent commit).  --parent FILE: the output
of such a run on the parent commit; its numbers are added to the report and compared with this tree's `off` against the
spread.

    python tools/ordinal_head_overhead.py [--iters 200] [--rounds 5] [--parent FILE] [--out profiles/ordinal_head_overhead.txt]
"""
import argparse
import os
import re
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_agent(ordinal):
    from cadre_amd import synth
    from ppo_agent.agent import CadreAgent
    fh, fw = synth.feat_hw(84, 84)
    cfg = dict(use_lstm=True, vae_device=0, device_num=0, vae_params="CoPM", measurement_dim=18,
               num_output=dict(steer=33, throttle=3), command_num=4, obs_hw=(84, 84), weights_init="none",
               vae_state_dict=synth.encoder_state(fh, fw, 7))
    if ordinal:
        cfg["ordinal_policy"] = True
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
    ap.add_argument("--act-iters", type=int, default=50)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cadre_amd import synth
    from ppo_agent.chief import chief_step
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.storage import RolloutStorage
    from tests.helpers import fill_storages

    modes = ("off",) if args.off_only else ("off", "on")
    parent = {}
    if args.parent:
        for m in re.finditer(r"^(B=\d+|act\(\))\s+off\s+([\d.]+) ms", open(args.parent).read(), re.M):
            parent[m.group(1)] = float(m.group(2))
    lines = ["Ordinal policy heads: PPO update step and act() (%s, median of %d rounds x %d steps / %d act calls)"
             % (torch.cuda.get_device_name(0), args.rounds, args.iters, args.act_iters)]
    agents = {m: make_agent(m == "on") for m in modes}
    shared = {m: Shared_grad_buffers(a.model_dict, a.device) for m, a in agents.items()}

    def report(tag, res, unit):
        med = {m: float(np.median(v)) for m, v in res.items()}
        spread = 100.0 * (max(res["off"]) - min(res["off"])) / med["off"]
        for m, v in res.items():
            lines.append("%-6s %-3s  %.4f ms/%s  (%+.2f %% vs off)   rounds: %s"
                         % (tag, m, med[m], unit, 100.0 * (med[m] / med["off"] - 1.0), " ".join("%.4f" % x for x in v)))
        lines.append("%-6s round-to-round spread of off: %.2f %% (max - min over median)" % (tag, spread))
        if tag in parent:
            d = 100.0 * (med["off"] / parent[tag] - 1.0)
            lines.append("%-6s parent commit, same tool, same box: off %.4f ms/%s; this tree's off: %+.2f %% -> %s"
                         % (tag, parent[tag], unit, d, "inside the spread" if abs(d) <= spread else "OUTSIDE the spread"))

    for B in (64, 256):
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
        idx = [torch.randperm(T)[:B] for _ in range(8)]

        def run(mode, n):
            agent = agents[mode]
            for i in range(n):
                agent.update_policy_from_storages(
                    [(pair[0], idx[i % 8], pair[0].advantages, pair[1], idx[(i + 4) % 8], pair[1].advantages)], sync=False)
                shared[mode].add_gradient(agent.model_dict)
                chief_step(shared[mode], None, 250.0, lr=3e-4, zero_grads=False)

        for mode in modes:
            run(mode, args.warmup)
        torch.cuda.synchronize()
        res = {m: [] for m in modes}
        for _ in range(args.rounds):
            for mode in modes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(mode, args.iters)
                e1.record()
                torch.cuda.synchronize()
                res[mode].append(e0.elapsed_time(e1) / args.iters)
        report("B=%d" % B, res, "step")

    steps = synth.synth_rollout(args.act_iters + args.warmup, 84, 84, seed=5)

    def act_round(mode, lo, hi):
        agent = agents[mode]
        ts = []
        for td in steps[lo:hi]:
            obs = dict(rgb=td["rgb"], route_fig=td["route_fig"].copy(), measurements=td["measurements"], command=td["command"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agent.act(obs)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ts))

    for mode in modes:
        act_round(mode, 0, args.warmup)
    res = {m: [] for m in modes}
    for _ in range(args.rounds):
        for mode in modes:
            res[mode].append(act_round(mode, args.warmup, args.warmup + args.act_iters))
    report("act()", res, "call")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
