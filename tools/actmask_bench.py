"""Cost of action masks: act_batch with and without `allowed=`, and the minibatch step in modes "ppo" and "ppo+mask".

act_batch at N = 8 (84x84 agent, 4 command nets): two agents with the same weights step the same observation streams, one with
`allowed=` (random steer words, the throttle head without its last bin), one without; a call is timed with the host clock around the
call and a device synchronise, the two forms alternating step by step, the median over the steps reported.

The minibatch step at B = 64 and B = 256 (one environment, T = 2 B, two minibatches per epoch): learner_section(..., step_events=) with
and without `actmask=` on the same agent and the same rows (a storage pair per mode) — the step-to-step HIP event intervals of a section (gather, the words launch, the
update's hipGraph, add_gradient, chief_step), the modes interleaved over --rounds rounds, the median per-step time of each mode
reported.  With masks every row carries a proper word on both heads.  Reported, not gated.

    python tools/actmask_bench.py [--epochs 50] [--rounds 5] [--steps 120] [--out profiles/actmask_latency.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def act_batch_times(steps, N=8):
    from tests.test_act_batch_gpu import build_agent, env_streams, obs_of
    streams, _ = env_streams(N, 84, 84, 4, steps)
    agents = {False: build_agent(84, 84), True: build_agent(84, 84)}
    r = np.random.RandomState(0)
    res = {False: [], True: []}
    for t in range(steps):
        words = [(int(r.randint(1, 2 ** 33 - 1)) | 1 << 16, 0b011) for _ in range(N)]
        for mode in ((False, True) if t % 2 == 0 else (True, False)):
            obs = [obs_of(streams[e][t]) for e in range(N)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            agents[mode].act_batch(obs, **(dict(allowed=words) if mode else {}))
            torch.cuda.synchronize()
            res[mode].append(1e3 * (time.perf_counter() - t0))
    return {m: np.asarray(v[steps // 6:]) for m, v in res.items()}       # (the first calls build workspaces and caches)


def step_times(B, epochs, rounds):
    from cadre_amd.actmask import ActionMasks
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.storage import RolloutStorage
    from ppo_agent.train import learner_section
    from tests.helpers import fill_storages
    from tests.test_learner_gpu import make_agent
    T = 2 * B
    agent = make_agent(84, 84)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    am = ActionMasks(lambda obs, info: (1, 1), agent.arena.n_out, agent.device)
    data = fill_storages(T, 3)
    r = np.random.RandomState(1)
    pairs = {False: [], True: []}                                    # the same rows twice: a pair with words is refused without actmask=
    for h, (hd, K) in enumerate((("steer", 33), ("throttle", 3))):
        for masked in (False, True):
            s = RolloutStorage(T, 2, 530, 8, 530, True, 0.99, 0.95)
            for k, v in data[hd].items():
                getattr(s, k).copy_(torch.from_numpy(v))
            s.to("cuda:0")
            pairs[masked].append(s)
        acts = pairs[True][h].action[:, 0].cpu().numpy()
        words = np.array([(int(r.randint(1, 2 ** K - 1)) | (1 << int(a))) & ~(1 << ((int(a) + 1) % K)) for a in acts], np.int64)
        pairs[True][h]._allowed_tensor().copy_(torch.from_numpy(words))   # a proper word on every row; the stored action stays allowed

    def run(masked, n_epochs):
        evs = []
        cfg = dict(use_adv_norm=True, ppo_epoch=n_epochs, max_grad_norm=250.0, lr=3e-4)
        learner_section(agent, pairs[masked][0], pairs[masked][1], False, cfg, shared, losses_on_device=True, step_events=evs,
                        **(dict(actmask=am) if masked else {}))
        torch.cuda.synchronize()
        return [evs[i].elapsed_time(evs[i + 1]) for i in range(len(evs) - 1)]

    for mode in (False, True):
        run(mode, 3)                                    # eager run, warm-up, capture
    res = {False: [], True: []}
    for _ in range(rounds):
        for mode in (False, True):
            res[mode].append(float(np.median(run(mode, epochs))))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("actmask_bench: no HIP device; the numbers of this tool are GPU times")
    lines = ["Action masks (%s)" % torch.cuda.get_device_name(0)]
    a = act_batch_times(args.steps)
    lines.append("act_batch, N = 8, 84x84, host clock around the call + synchronise, median of %d alternating calls per form" % len(a[False]))
    for mode, name in ((False, "allowed=None"), (True, "allowed=words")):
        lines.append("  %-14s %.4f ms/call   (p10 %.4f, p90 %.4f)" % (name, np.median(a[mode]), np.percentile(a[mode], 10), np.percentile(a[mode], 90)))
    lines.append("  difference: %+.4f ms/call (%+.2f %%)" % (np.median(a[True]) - np.median(a[False]),
                                                           100.0 * (np.median(a[True]) / np.median(a[False]) - 1.0)))
    for B in (64, 256):
        res = step_times(B, args.epochs, args.rounds)
        med = {m: float(np.median(v)) for m, v in res.items()}
        lines.append("PPO minibatch step, B = %d, median step of %d rounds x %d steps, HIP events" % (B, args.rounds, 2 * args.epochs))
        for mode, name in ((False, '"ppo"'), (True, '"ppo+mask"')):
            lines.append("  %-11s %.4f ms/step   rounds: %s" % (name, med[mode], " ".join("%.4f" % x for x in res[mode])))
        lines.append("  difference: %+.4f ms/step (%+.2f %%); round-to-round spread of \"ppo\": %.2f %%"
                     % (med[True] - med[False], 100.0 * (med[True] / med[False] - 1.0),
                        100.0 * (max(res[False]) - min(res[False])) / med[False]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
