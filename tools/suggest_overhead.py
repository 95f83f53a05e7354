"""Cost of exploration suggestions on the minibatch step.

learner_section(..., step_events=) at B = 64 (one environment, T = 128, two minibatches per epoch, 4 command nets, 84x84 agent),
with and without `suggest=` on the same agent and storages: the step-to-step HIP event intervals of a section (gather, the rows
launch, the update's hipGraph, add_gradient, chief_step), the modes interleaved over --rounds rounds, the median per-step time
of each mode reported.  With suggestions about a third of the rows of each head are marked.  Reported, not gated.

    python tools/suggest_overhead.py [--epochs 50] [--rounds 5] [--out profiles/suggest_step.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cadre_amd.suggest import Suggestions, peaked_prior, uniform_prior
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.storage import RolloutStorage
    from ppo_agent.train import learner_section
    from tests.helpers import fill_storages
    from tests.test_learner_gpu import make_agent

    B, T = 64, 128
    agent = make_agent(84, 84)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    sug = Suggestions(dict(coeff=0.05, events=dict(blocked=dict(head="throttle", prior=peaked_prior(3, 1, 0.8), horizon=6),
                                                   route_deviation=dict(head="steer", prior=uniform_prior(33), horizon=6))),
                      agent.arena.n_out, agent.device)
    data = fill_storages(T, 3)
    pair = []
    for h, hd in enumerate(("steer", "throttle")):
        s = RolloutStorage(T, T // B, 530, 8, 530, True, 0.99, 0.95)
        for k, v in data[hd].items():
            getattr(s, k).copy_(torch.from_numpy(v))
        s.to("cuda:0")
        ev = s._event_tensors()
        ev[torch.arange(9 + h, T, 18, device="cuda:0")] = sug.code["route_deviation" if h == 0 else "blocked"]
        pair.append(s)
    agent.learner.set_loss("ppo+suggest", suggest_coeff=0.05)
    agent.learner.set_loss("ppo")

    def run(with_sug, epochs):
        evs = []
        cfg = dict(use_adv_norm=True, ppo_epoch=epochs, max_grad_norm=250.0, lr=3e-4)
        learner_section(agent, pair[0], pair[1], False, cfg, shared, losses_on_device=True, step_events=evs,
                        **(dict(suggest=sug) if with_sug else {}))
        torch.cuda.synchronize()
        return [evs[i].elapsed_time(evs[i + 1]) for i in range(len(evs) - 1)]

    for mode in (False, True):
        run(mode, 3)                                    # eager run, warm-up, capture
    res = {False: [], True: []}
    for _ in range(args.rounds):
        for mode in (False, True):
            res[mode].append(float(np.median(run(mode, args.epochs))))
    marked = [int((s.suggest != 0).sum()) for s in pair]
    med = {m: float(np.median(v)) for m, v in res.items()}
    lines = ["PPO minibatch step with exploration suggestions (%s, B = %d, median step of %d rounds x %d steps; marked rows of %d: %d steer, %d throttle)"
             % (torch.cuda.get_device_name(0), B, args.rounds, 2 * args.epochs, T, marked[0], marked[1])]
    for mode, name in ((False, "without the key"), (True, "with suggestions")):
        lines.append("%-17s %.4f ms/step   rounds: %s" % (name, med[mode], " ".join("%.4f" % x for x in res[mode])))
    lines.append("difference: %+.4f ms/step (%+.2f %%); round-to-round spread without the key: %.2f %%"
                 % (med[True] - med[False], 100.0 * (med[True] / med[False] - 1.0),
                    100.0 * (max(res[False]) - min(res[False])) / med[False]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
