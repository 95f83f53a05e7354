"""What sample reuse costs on the GPU at the C2 update shape (1 worker x 128 steps, 2 minibatches of 64 rows, 4 command nets,
84x84 agent; the encoder does not run):

  refresh   ReuseWindow.refresh with all M slots filled: the record pass over M (T + 1) rows (gather + the update's forward +
            cadre_reuse_record per minibatch of 128 rows, eager) + ONE cadre_vtrace_multi launch over the 2 M stale storages
  step N    update_policy_from_storages with the live entry (B = 64) + learner.clip_adam
  step (1+M)N   the same with the M stale entries behind it (B = 64 (1 + M))
in one process on the same agent and storages.  Timed with HIP events over --iters calls after --warmup calls (graphs captured
during the warm-up), the modes interleaved over --rounds rounds; medians, the round-to-round spread of the N-entry step and
the launch counts are reported.  No bar is set on these numbers.  Reads nothing outside the tree.

    python tools/reuse_overhead.py [--rollouts 3] [--iters 100] [--rounds 5] [--out profiles/reuse_overhead.txt]
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
    ap.add_argument("--rollouts", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reuse_overhead needs an MI355X: a time taken elsewhere says nothing")
    from cadre_amd import hip
    from cadre_amd.reuse import ReuseWindow
    from ppo_agent.storage import RolloutStorage
    from tests.helpers import fill_storages

    T, MBN, M = 128, 2, args.rollouts
    Bw = T // MBN
    agent = make_agent()
    lrn = agent.learner

    def rollout(seed):
        data = fill_storages(T, seed, with_hidden=False)
        pair = []
        for hd in ("steer", "throttle"):
            s = RolloutStorage(T, MBN, 530, 8, 530, True, 0.99, 0.95)
            for k, v in data[hd].items():
                getattr(s, k).copy_(torch.from_numpy(v))
            s.to("cuda:0")
            pair.append(s)
        return tuple(pair)

    win = ReuseWindow(agent, M, 1, T)
    for m in range(M):
        win.append([rollout(10 + m)], [False])
    live = rollout(3)
    RolloutStorage.finish_rollouts(list(live), [torch.tensor([0.1]), torch.tensor([0.1])])
    idx = [torch.randperm(T)[:Bw] for _ in range(8)]

    def step(stale, n):
        for i in range(n):
            a = idx[i % 8]
            batches = [(live[0], a, live[0].advantages, live[1], a, live[1].advantages)]
            if stale:
                batches += win.entries(0, i // MBN, i % MBN, Bw)
            agent.update_policy_from_storages(batches, sync=False)
            lrn.clip_adam(lr=3e-4, max_grad_norm=250.0)

    def refresh(_stale, n):
        for _ in range(n):
            win.refresh(True)

    modes = (("refresh", refresh, None), ("step_N", step, False), ("step_(1+M)N", step, True))
    n0 = hip.N_CALLS
    win.refresh(True)
    launches = {"refresh": hip.N_CALLS - n0}
    lrn.clip_adam(lr=3e-4, max_grad_norm=250.0)
    for name, fn, arg in modes:
        fn(arg, args.warmup)
    launches["step_N"], launches["step_(1+M)N"] = lrn.launches[("all", Bw)], lrn.launches[("all", Bw * (1 + M))]
    torch.cuda.synchronize()
    res = {name: [] for name, _f, _a in modes}
    for _ in range(args.rounds):
        for name, fn, arg in modes:
            n = max(1, args.iters // 10) if name == "refresh" else args.iters
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(arg, n)
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / n)
    med = {k: float(np.median(v)) for k, v in res.items()}
    spread = 100.0 * (max(res["step_N"]) - min(res["step_N"])) / med["step_N"]
    lines = ["Sample reuse at the C2 update shape (%s; T = %d, minibatch %d, M = %d stale rollouts; median of %d rounds, same process)"
             % (torch.cuda.get_device_name(0), T, Bw, M, args.rounds)]
    for name, _f, _a in modes:
        what = "launches in the call" if name == "refresh" else "launches in the update"
        lines.append("%-12s %.4f ms/call   %s: %d   rounds: %s" % (name, med[name], what, launches[name],
                                                                    " ".join("%.4f" % x for x in res[name])))
    lines.append("step (1+M)N / step N: %.2fx at %dx the rows; round-to-round spread of step N: %.2f %% (max - min over median)"
                 % (med["step_(1+M)N"] / med["step_N"], 1 + M, spread))
    lines.append("per learner section (%d steps at ppo_epoch 4): refresh %.3f ms + steps %.3f ms against %.3f ms without reuse"
                 % (4 * MBN, med["refresh"], 4 * MBN * med["step_(1+M)N"], 4 * MBN * med["step_N"]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
