"""Time of one step of the PPG auxiliary phase next to the PPO step of the same process and shapes.

One step = the minibatch gather + the update's hipGraph + the clip + Adam graph, at B = 64 (one entry, 4 command nets, 84x84
agent, the row-sorted form; the encoder does not run):
  ppo   update_policy_from_storages + learner.clip_adam        (cadre_ppo_loss in the update)
  aux   aux_from_storages           + learner.clip_adam        (cadre_aux_loss in its place + the copy of the step's row ids
                                                                into the static workspace tensor the captured graph reads)
on the same agent, the same storages and the same row indices.  Timed with HIP events over --iters steps after --warmup
steps (graphs captured during the warm-up), the modes interleaved over --rounds rounds; the median per mode, the
round-to-round spread of `ppo` and the launch counts (learner.launches) are reported.  Reads nothing outside the tree.

    python tools/aux_step_bench.py [--iters 200] [--rounds 7] [--out profiles/aux_phase_latency.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bc_step_bench import make_agent          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aux_step_bench needs an MI355X: a time taken elsewhere says nothing")
    from cadre_amd.phasic import AuxBuffer
    from ppo_agent.storage import RolloutStorage
    from tests.helpers import fill_storages

    agent = make_agent()
    lrn = agent.learner
    lines = ["Auxiliary step next to the PPO step (%s, median of %d rounds x %d steps, same process, same storages)"
             % (torch.cuda.get_device_name(0), args.rounds, args.iters)]
    for B in (64,):
        T = 4 * B
        data = fill_storages(T, 3, with_hidden=False)
        pair = []
        for hd in ("steer", "throttle"):
            s = RolloutStorage(T, 2, 530, 8, 530, True, 0.99, 0.95)
            for k, v in data[hd].items():
                getattr(s, k).copy_(torch.from_numpy(v))
            s.to("cuda:0")
            s.compute_returns(torch.tensor([0.1]))
            pair.append(s)
        buf = AuxBuffer(agent, 1, T)
        buf.append([tuple(pair)])                          # the phase's rows ARE the PPO step's rows
        order = torch.arange(T)
        for lo in range(0, T, B):
            agent.aux_record_from_storages(buf.entry(order[lo:lo + B]), buf.table)
        idx = [torch.randperm(T)[:B] for _ in range(8)]
        launches = {}

        def run(mode, n):
            for i in range(n):
                a = idx[i % 8]
                if mode == "ppo":
                    agent.update_policy_from_storages([(pair[0], a, pair[0].advantages, pair[1], a, pair[1].advantages)], sync=False)
                else:
                    agent.aux_from_storages(buf.entry(a), buf.table, sync=False)
                lrn.clip_adam(lr=3e-4, max_grad_norm=250.0)

        lrn.clip_adam(lr=3e-4, max_grad_norm=250.0)        # (the record pass packed W_hh: a step makes the census count the packing launch)
        for mode in ("ppo", "aux"):
            run(mode, 1)                                   # (the eager first call of the mode counts its launches)
            launches[mode] = lrn.launches[("all", B)]
            run(mode, args.warmup)
        torch.cuda.synchronize()
        res = {"ppo": [], "aux": []}
        for _ in range(args.rounds):
            for mode in ("ppo", "aux"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(mode, args.iters)
                e1.record()
                torch.cuda.synchronize()
                res[mode].append(e0.elapsed_time(e1) / args.iters)
        med = {m: float(np.median(v)) for m, v in res.items()}
        spread = 100.0 * (max(res["ppo"]) - min(res["ppo"])) / med["ppo"]
        for m in ("ppo", "aux"):
            lines.append("B=%-4d %-3s  %.4f ms/step  (%+.2f %% vs ppo)  launches in the update: %d   rounds: %s"
                         % (B, m, med[m], 100.0 * (med[m] / med["ppo"] - 1.0), launches[m], " ".join("%.4f" % x for x in res[m])))
        d = abs(100.0 * (med["aux"] / med["ppo"] - 1.0))
        lines.append("B=%-4d round-to-round spread of ppo: %.2f %% (max - min over median) -> aux is %s the spread"
                     % (B, spread, "inside" if d <= spread else "OUTSIDE"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
