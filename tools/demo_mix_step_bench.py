"""Time of one mixed step (PPO rows + demonstration rows, DAPG-style) next to the plain PPO step of the same row count.

One step = the minibatch gather + the update's hipGraph + the clip + Adam graph (4 command nets, 84x84 agent; the encoder
does not run), at Bw = 64 and Bw = 256 rows per worker minibatch:
  ppo   update_policy_from_storages of TWO worker entries       + learner.clip_adam   (2 Bw rows, cadre_ppo_loss)
  mix   update_policy_from_storages of one worker entry and
        one demonstration entry (demo=, blocks = 1)             + learner.clip_adam   (2 Bw rows, cadre_mix_row_kinds +
                                                                                       cadre_ppo_demo_loss in its place)
on the same agent and the same storages — the two steps differ by the loss launch and the row-kind launch in front of it.
Timed with HIP events over --iters steps after --warmup steps (graphs captured during the warm-up), the modes interleaved
over --rounds rounds; the median per mode, the round-to-round spread of `ppo` and the launch counts (learner.launches) are
reported.  Then the loss launches alone, back to back on the update's workspace: cadre_ppo_loss_ord against
cadre_mix_row_kinds + cadre_ppo_demo_loss at the same B.  Reads nothing outside the tree.

    python tools/demo_mix_step_bench.py [--iters 200] [--rounds 5] [--out profiles/demo_mix_step.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bc_step_bench import make_agent  # noqa: E402


def storages(T, seed):
    from ppo_agent.storage import RolloutStorage
    from tests.helpers import fill_storages
    data = fill_storages(T, seed, with_hidden=False)
    pair = []
    for hd in ("steer", "throttle"):
        s = RolloutStorage(T, 2, 530, 8, 530, True, 0.99, 0.95)
        for k, v in data[hd].items():
            getattr(s, k).copy_(torch.from_numpy(v))
        s.to("cuda:0")
        s.compute_returns(torch.tensor([0.1]))
        pair.append(s)
    return pair


def loss_launch_us(agent, B, n=500):
    """Microseconds per loss launch, back to back on workspace(B) as the last step left it: (cadre_ppo_loss_ord,
    cadre_mix_row_kinds + cadre_ppo_demo_loss)."""
    from cadre_amd import hip
    lrn, a = agent.learner, agent.arena
    w = lrn.workspace(B)
    L, st = hip.lib(), hip.stream()
    O3, dO3, NP = w["O3"], w["dO3"], a.NP
    table = torch.zeros(2, 64, dtype=torch.int32, device=a.device)
    table[:, 0] = -1
    head = (hip.ptr(O3), NP, 2 * B * NP, hip.ptr(O3[1]), NP, 2 * B * NP, hip.ptr(w["actions"]), hip.ptr(w["commands"]),
            hip.ptr(w["old_values"]), hip.ptr(w["returns"]), hip.ptr(w["old_logp"]), hip.ptr(w["adv"]))
    poison = hip.ptr(w["sync"][a.Z * lrn.S:])

    def ppo():
        hip.check(L.cadre_ppo_loss_ord(*head, B, a.C, a.n_out[0], a.n_out[1], None, 0.1, 0.1, 1.0, 0.01, 2.0 / B,
                                       hip.ptr(w["losses"]), hip.ptr(dO3), hip.ptr(dO3[1]), hip.ptr(w["loss_scratch"]), poison,
                                       None, 0, None, 0.0, None, hip.ptr(table), st), "cadre_ppo_loss_ord")

    def mix():
        hip.check(L.cadre_mix_row_kinds(None, B, B // 2, hip.ptr(w["row_kind"]), st), "cadre_mix_row_kinds")
        hip.check(L.cadre_ppo_demo_loss(*head, hip.ptr(w["row_kind"]), B, a.C, a.n_out[0], a.n_out[1], None, 0.1, 0.1, 1.0, 0.01,
                                        2.0 / B, 0.1, 1.0, 0.0, 2.0 / B, hip.ptr(w["losses"]), hip.ptr(w["demo_losses"]),
                                        hip.ptr(dO3), hip.ptr(dO3[1]), hip.ptr(w["loss_scratch"]), hip.ptr(w["demo_scratch"]),
                                        poison, None, 0, None, 0.0, None, hip.ptr(w["demo_stats"]), hip.BC_STATS_FIELDS,
                                        hip.ptr(table), st), "cadre_ppo_demo_loss")
    out = []
    for fn in (ppo, mix):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(1000.0 * e0.elapsed_time(e1) / n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("demo_mix_step_bench needs an MI355X: a time taken elsewhere says nothing")
    agent = make_agent()
    lrn = agent.learner
    lines = ["Mixed step (PPO rows + demonstration rows) next to the PPO step of the same row count (%s, median of %d rounds x "
             "%d steps, same process, same storages)" % (torch.cuda.get_device_name(0), args.rounds, args.iters)]
    for Bw in (64, 256):
        B, T = 2 * Bw, 4 * Bw
        pair, dpair = storages(T, 3), storages(T, 5)
        weights = (torch.rand(T, 1) * 3.75 + 0.25).cuda()
        idx = [torch.randperm(T)[:Bw] for _ in range(8)]
        launches = {}

        def run(mode, n):
            for i in range(n):
                a, b, c, d = (idx[(i + j) % 8] for j in (0, 4, 2, 6))
                first = (pair[0], a, pair[0].advantages, pair[1], b, pair[1].advantages)
                if mode == "ppo":
                    agent.update_policy_from_storages([first, (pair[0], c, pair[0].advantages, pair[1], d, pair[1].advantages)],
                                                      sync=False)
                else:
                    agent.update_policy_from_storages([first], sync=False, demo=[(dpair[0], c, weights, dpair[1], d, weights)],
                                                      demo_label_smoothing=0.1, demo_coeff=1.0, demo_value_coeff=0.0)
                lrn.clip_adam(lr=3e-4, max_grad_norm=250.0)

        for mode in ("ppo", "mix"):
            run(mode, 1)                                   # (the eager first call of the mode counts its launches)
            launches[mode] = lrn.launches[("all", B)]
            run(mode, args.warmup)
        torch.cuda.synchronize()
        res = {"ppo": [], "mix": []}
        for _ in range(args.rounds):
            for mode in ("ppo", "mix"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(mode, args.iters)
                e1.record()
                torch.cuda.synchronize()
                res[mode].append(e0.elapsed_time(e1) / args.iters)
        med = {m: float(np.median(v)) for m, v in res.items()}
        spread = 100.0 * (max(res["ppo"]) - min(res["ppo"])) / med["ppo"]
        for m in ("ppo", "mix"):
            lines.append("Bw=%-4d B=%-4d %-3s  %.4f ms/step  (%+.2f %% vs ppo)  launches in the update: %d   rounds: %s"
                         % (Bw, B, m, med[m], 100.0 * (med[m] / med["ppo"] - 1.0), launches[m], " ".join("%.4f" % x for x in res[m])))
        d = abs(100.0 * (med["mix"] / med["ppo"] - 1.0))
        lines.append("Bw=%-4d round-to-round spread of ppo: %.2f %% (max - min over median) -> mix is %s the spread"
                     % (Bw, spread, "inside" if d <= spread else "OUTSIDE"))
        us = loss_launch_us(agent, B)
        lines.append("Bw=%-4d loss launches alone, back to back at B=%d: cadre_ppo_loss_ord %.2f us, cadre_mix_row_kinds + "
                     "cadre_ppo_demo_loss %.2f us (%+.2f us)" % (Bw, B, us[0], us[1], us[1] - us[0]))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
