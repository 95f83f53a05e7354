"""Cost of self-imitation learning in the PPO step: the prioritised draw and the priority write-back on their own, and one mixed
step next to the PPO step and the "ppo+demo" step of the same row count.

The buffer has the reference's rollout size, T = 200, M = 8 rollouts of N = 4 environments (6432 rows per head), every row
eligible (tail = "bootstrap").  Timed with HIP events, the modes interleaved over --rounds rounds, medians reported with the
round-to-round spread:
  draw     cadre_sil_draw (three launches) of 64 rows per head, back to back; also at Rcap = 2^20
  scatter  cadre_sil_scatter of 64 rows per head, back to back
  ppo      update_policy_from_storages of TWO worker entries of 64 rows          + learner.clip_adam   (128 rows)
  demo     one worker entry + one demonstration entry (demo=)                    + learner.clip_adam   (128 rows)
  sil      SelfImitationBuffer.entries (the draw) + one worker entry + one SIL entry (sil=) + after_step (the write-back)
                                                                                 + learner.clip_adam   (128 rows)
on the same agent (4 command nets, 84x84; the encoder does not run).  Reads nothing outside the tree.

    python tools/sil_bench.py [--iters 200] [--rounds 5] [--out profiles/selfimit_step.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bc_step_bench import make_agent  # noqa: E402
from tools.demo_mix_step_bench import storages  # noqa: E402

T, M, N, BW = 200, 8, 4, 64


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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sil_bench needs an MI355X: a time taken elsewhere says nothing")
    from cadre_amd import hip
    from cadre_amd.selfimit import SelfImitationBuffer
    agent = make_agent()
    lrn = agent.learner
    L, st = hip.lib(), hip.stream()
    buf = SelfImitationBuffer(agent, M, N, T, tail="bootstrap", seed=1)
    rollouts = [storages(T, 20 + i) for i in range(N)]
    for m in range(M):
        buf.append(rollouts, [False] * N)
    assert buf.ready and buf.rows_filled() == M * N * (T + 1)
    pair, dpair = storages(4 * BW, 3), storages(4 * BW, 5)
    weights = (torch.rand(4 * BW, 1) * 3.75 + 0.25).cuda()
    idx = [torch.randperm(4 * BW)[:BW] for _ in range(8)]
    B = 2 * BW
    lrn.set_loss("ppo+sil", sil_coeff=0.1, sil_value_coeff=0.01)
    lrn.set_loss("ppo")

    def step(mode, i):
        a, b, c, d = (idx[(i + j) % 8] for j in (0, 4, 2, 6))
        first = (pair[0], a, pair[0].advantages, pair[1], b, pair[1].advantages)
        if mode == "ppo":
            agent.update_policy_from_storages([first, (pair[0], c, pair[0].advantages, pair[1], d, pair[1].advantages)], sync=False)
        elif mode == "demo":
            agent.update_policy_from_storages([first], sync=False, demo=[(dpair[0], c, weights, dpair[1], d, weights)],
                                              demo_label_smoothing=0.1, demo_coeff=1.0, demo_value_coeff=0.0)
        else:
            agent.update_policy_from_storages([first], sync=False, sil=buf.entries(BW, 0, 0, i))
            buf.after_step(BW)
        lrn.clip_adam(lr=3e-4, max_grad_norm=250.0)

    modes = ("ppo", "demo", "sil")
    launches = {}
    for mode in modes:
        step(mode, 0)                                          # (the eager first call of the mode counts its launches)
        launches[mode] = lrn.launches[("all", B)]
        for i in range(args.warmup):
            step(mode, i)
    torch.cuda.synchronize()
    # the two small launches on their own
    n = BW
    u = torch.randint(0, 1 << 62, (2, n), dtype=torch.int64).cuda()
    out_idx = torch.zeros(2, n, dtype=torch.int64, device="cuda")
    w = lrn.workspace(B)
    big = 1 << 20
    q_big = torch.randint(0, 1 << 16, (2, big), dtype=torch.int32).cuda()
    s_big = torch.zeros(4 * (big // 1024) + 2, dtype=torch.int64, device="cuda")

    def draw(_i):
        hip.check(L.cadre_sil_draw(hip.ptr(buf.q), buf.R, buf.rows_filled(), hip.ptr(u), n, hip.ptr(out_idx), hip.ptr(buf._scratch), st),
                  "cadre_sil_draw")

    def draw_big(_i):
        hip.check(L.cadre_sil_draw(hip.ptr(q_big), big, big, hip.ptr(u), n, hip.ptr(out_idx), hip.ptr(s_big), st), "cadre_sil_draw")

    def scatter(_i):
        hip.check(L.cadre_sil_scatter(hip.ptr(buf.q), buf.R, hip.ptr(out_idx), n, hip.ptr(w["sil_w"]), None, B, BW, buf.alpha,
                                      buf.prio_eps, st), "cadre_sil_scatter")
    small = dict(draw=draw, draw_2_20=draw_big, scatter=scatter)
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
    lines = ["Self-imitation in the PPO step (%s, median of %d interleaved rounds x %d, same process, same storages; buffer T=%d M=%d "
             "N=%d, %d rows per head)" % (torch.cuda.get_device_name(0), args.rounds, args.iters, T, M, N, buf.R)]
    for k, what in (("draw", "cadre_sil_draw, 64 rows per head, Rcap=%d" % buf.R), ("draw_2_20", "cadre_sil_draw, 64 rows per head, Rcap=2^20"),
                    ("scatter", "cadre_sil_scatter, 64 rows per head")):
        lines.append("%-10s %8.2f us  spread %.2f %%  (%s)  rounds: %s" % (k, med[k], spread(k), what, " ".join("%.2f" % x for x in res[k])))
    for m in modes:
        lines.append("B=%-4d %-4s  %.4f ms/step  (%+.2f %% vs ppo, %+.2f %% vs demo)  launches in the update: %d   spread %.2f %%   rounds: %s"
                     % (B, m, med[m], 100.0 * (med[m] / med["ppo"] - 1.0), 100.0 * (med[m] / med["demo"] - 1.0), launches[m], spread(m),
                        " ".join("%.4f" % x for x in res[m])))
    lines.append("the sil step carries the draw (3 launches) and the write-back (1 launch) outside the update's graph; the draw at "
                 "Rcap=2^20 is %.1f %% of one ppo step" % (100.0 * med["draw_2_20"] / (1000.0 * med["ppo"])))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
