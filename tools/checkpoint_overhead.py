"""Cost of a training checkpoint's device side at the full-size arena (parameters + both Adam moments, 3 x ~80 MB).

Three measurements:
  (a) capture   one cadre_state_capture launch over the three ranges (copy + one digest each from the same read)
  (b) copy_ x3  the same bytes as three Tensor.copy_ calls into the same staging buffer: what a torch-only capture would
                cost, the yardstick (it forms no digest)
  (c) section   a learner_section_multi (2 environments, T = 64, 2 epochs x 2 minibatches) without and with a capture
                enqueued behind it (capture(): the launch plus the side-stream copy to pinned host memory)
(a) and (b) are timed with HIP events over --iters repetitions after --warmup, interleaved over --rounds rounds; (c) with
HIP events around each section, interleaved likewise.  Medians are reported with the spread of the rounds.

    python tools/checkpoint_overhead.py [--iters 50] [--rounds 7] [--out profiles/checkpoint_overhead.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sections", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cadre_amd import checkpoint, hip
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section_multi
    from tests.test_act_batch_gpu import build_agent
    from tests.test_ppo_stats_gpu import storages

    agent = build_agent(84, 84)
    a = agent.arena
    a.ensure_adam()
    g = torch.Generator().manual_seed(1)
    a.exp_avg.copy_(torch.randn(a.total, generator=g) * 1e-3)
    a.exp_avg_sq.copy_(torch.rand(a.total, generator=g) * 1e-6)
    srcs = [a.params, a.exp_avg, a.exp_avg_sq]
    nbytes = [t.numel() * 4 for t in srcs]
    offs = [sum(nbytes[:k]) for k in range(3)]
    staging = torch.empty(sum(nbytes), dtype=torch.uint8, device=a.device)
    views = [staging[o:o + n].view(torch.float32) for o, n in zip(offs, nbytes)]
    table = hip.capture_table([(t.data_ptr(), o, n) for t, o, n in zip(srcs, offs, nbytes)], a.device)
    digests = torch.zeros(3, dtype=torch.int64, device=a.device)

    def run(form, n):
        for _ in range(n):
            if form == "capture":
                hip.state_capture(table, 3, staging, digests)
            else:
                for v, t in zip(views, srcs):
                    v.copy_(t)

    forms = ("capture", "copy_ x3")
    for f in forms:
        run(f, args.warmup)
    torch.cuda.synchronize()
    for v, t in zip(views, srcs):                           # (the launch copied what copy_ copies)
        assert torch.equal(v.view(torch.int32), t.view(torch.int32))
    want = [checkpoint.reference_digest(t.cpu().numpy()) for t in srcs]
    assert [int(d) & (2 ** 64 - 1) for d in digests.tolist()] == want
    res = {f: [] for f in forms}
    for _ in range(args.rounds):
        for f in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(f, args.iters)
            e1.record()
            torch.cuda.synchronize()
            res[f].append(1e3 * e0.elapsed_time(e1) / args.iters)
    total = sum(nbytes)
    lines = ["checkpoint device side, arena of %d floats: %d ranges, %.1f MB read + %.1f MB written (%s, median of %d rounds x "
             "%d repetitions, us)" % (a.total, 3, total / 1e6, total / 1e6, torch.cuda.get_device_name(0), args.rounds, args.iters)]
    base = float(np.median(res["copy_ x3"]))
    for f in forms:
        v = res[f]
        med = float(np.median(v))
        lines.append("%-9s %9.2f us  (%.3f x copy_ x3, %.2f TB/s read + written)   min %.2f  max %.2f   rounds: %s"
                     % (f, med, med / base, 2 * total / med / 1e6, min(v), max(v), " ".join("%.2f" % x for x in v)))

    # (c) a learner section with and without a capture behind it
    N, T = 2, 64
    rollouts = [tuple(storages(T, 2, 21 + e)) for e in range(N)]
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    cfg = dict(use_adv_norm=True, ppo_epoch=2, max_grad_norm=250.0, lr=3e-4)

    def section(with_capture):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        learner_section_multi(agent, rollouts, [False] * N, cfg, shared, losses_on_device=True)
        if with_capture:
            checkpoint.capture(agent, rollouts, None)
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    for _ in range(3):
        section(False); section(True)
    sec = {False: [], True: []}
    for _ in range(args.rounds):
        for wc in (False, True):
            sec[wc].append(float(np.median([section(wc) for _ in range(args.sections)])))
    m0, m1 = float(np.median(sec[False])), float(np.median(sec[True]))
    lines.append("learner_section_multi (%d environments, T = %d, 2 epochs x 2 minibatches), compute stream, us:" % (N, T))
    lines.append("section            %9.2f us   min %.2f  max %.2f" % (m0, min(sec[False]), max(sec[False])))
    lines.append("section + capture  %9.2f us   min %.2f  max %.2f   (+%.2f us, %.3f x)"
                 % (m1, min(sec[True]), max(sec[True]), m1 - m0, m1 / m0))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
