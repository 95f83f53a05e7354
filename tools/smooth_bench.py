"""Cost of the temporal smoothness term in the PPO step: one "ppo+smooth" step of 128 PPO rows + 128 successor rows next to the plain
PPO step of 256 rows, and the two small launches on their own.

Timed with HIP events, the modes interleaved over --rounds rounds, medians reported with the round-to-round spread:
  ppo      update_policy_from_storages of TWO worker entries of 128 rows                  + learner.clip_adam   (256 rows)
  smooth   Smoothness.step (the successor indices, on the host) + one worker entry + one successor entry (smooth=; the
           cadre_smooth_mates launch rides outside the update's graph)                    + learner.clip_adam   (256 rows)
  mates    cadre_smooth_mates for that step, back to back
  jitter   cadre_action_jitter on 8 storages of T = 512, back to back
on the same agent (4 command nets, 84x84; the encoder does not run).  Reads nothing outside the tree.

    python tools/smooth_bench.py [--iters 200] [--rounds 5] [--out profiles/smooth_step.txt]
    python tools/smooth_bench.py --ppo-only --tree PATH     # the plain PPO step of another checkout (the parent commit's), same tool
"""
import argparse
import os
import sys

import numpy as np
import torch

T, BW = 512, 128


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ppo-only", action="store_true", help="time the plain PPO step only (needs nothing of the smoothness term)")
    ap.add_argument("--tree", default=None, help="the checkout whose code runs (default: this one)")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, tree)
    if not torch.cuda.is_available():
        raise SystemExit("smooth_bench needs an MI355X: a time taken elsewhere says nothing")
    from cadre_amd import hip
    from tools.bc_step_bench import make_agent
    from tools.demo_mix_step_bench import storages
    agent = make_agent()
    lrn = agent.learner
    pair = storages(T, 3)
    idx = [torch.randperm(T - 1)[:BW] for _ in range(8)]
    B = 2 * BW
    modes = ("ppo",) if args.ppo_only else ("ppo", "smooth")
    sm = None
    if not args.ppo_only:
        from cadre_amd.smooth import Smoothness
        sm = Smoothness(agent, 0.1)
        lrn.set_loss("ppo+smooth", smooth_coeff=0.1)
        lrn.set_loss("ppo")

    def step(mode, i):
        a, b, c, d = (idx[(i + j) % 8] for j in (0, 4, 2, 6))
        first = (pair[0], a, pair[0].advantages, pair[1], b, pair[1].advantages)
        if mode == "ppo":
            agent.update_policy_from_storages([first, (pair[0], c, pair[0].advantages, pair[1], d, pair[1].advantages)], sync=False)
        else:
            agent.update_policy_from_storages([first], sync=False, smooth=sm.step([first]))
        lrn.clip_adam(lr=3e-4, max_grad_norm=250.0)

    launches = {}
    for mode in modes:
        step(mode, 0)                                          # (the eager first call of the mode counts its launches)
        launches[mode] = lrn.launches[("all", B)]
        for i in range(args.warmup):
            step(mode, i)
    torch.cuda.synchronize()
    small = {}
    if sm is not None:
        L, st = hip.lib(), hip.stream()
        w = lrn.workspace(B)
        stable, idx_d, _bw, _t = agent._smooth_src
        srt = lrn.sorted_rows(B)

        def mates(_i):
            hip.check(L.cadre_smooth_mates(hip.ptr(stable), hip.ptr(idx_d), 1, 1, BW, T, agent.arena.C, 0, hip.ptr(w["pos"]) if srt else None,
                                           B, hip.ptr(w["row_kind"]), hip.ptr(w["mate"]), st), "cadre_smooth_mates")
        many = [s for k in range(4) for s in storages(T, 30 + k)]
        small = dict(mates=mates, jitter=lambda _i: sm.jitter(many))
        for fn in small.values():
            timed(fn, 20)
    res = {k: [] for k in list(modes) + list(small)}
    for _ in range(args.rounds):
        for mode in modes:
            res[mode].append(timed(lambda i, m=mode: step(m, i), args.iters))
        for k, fn in small.items():
            res[k].append(1000.0 * timed(fn, args.iters))
    med = {k: float(np.median(v)) for k, v in res.items()}
    spread = lambda k: 100.0 * (max(res[k]) - min(res[k])) / med[k]
    lines = ["Temporal smoothness in the PPO step (%s, median of %d interleaved rounds x %d, same process, same storages; tree %s)"
             % (torch.cuda.get_device_name(0), args.rounds, args.iters, "this one" if not args.tree else "another checkout")]
    for k, what in (("mates", "cadre_smooth_mates, 128 + 128 rows"), ("jitter", "cadre_action_jitter, 8 storages of T = %d (with the output allocation)" % T)):
        if k in small:
            lines.append("%-7s %8.2f us  spread %.2f %%  (%s)  rounds: %s" % (k, med[k], spread(k), what, " ".join("%.2f" % x for x in res[k])))
    for m in modes:
        lines.append("B=%-4d %-6s  %.4f ms/step  (%+.2f %% vs ppo)  launches in the update: %d   spread %.2f %%   rounds: %s"
                     % (B, m, med[m], 100.0 * (med[m] / med["ppo"] - 1.0), launches[m], spread(m), " ".join("%.4f" % x for x in res[m])))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
