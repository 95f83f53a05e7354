"""Time of the minibatch gather launch of a behaviour-cloning step from a materialised DemoSet and from a frame-table
DemoSet of the same episodes.

Two synthetic episodes (84x84 frames, --rows transitions in all) are recorded with RolloutRecorder into a temporary
directory and loaded twice: DemoSet.from_episodes(frame_table=False / True).  The launch timed is the one the step issues at
B = 256 (row-sorted layout, one worker): cadre_gather_sorted_multi against cadre_gather_sorted_multi_ft on the same learner
workspace, the same row indices, tables built as CadreAgent builds them.  Both move the same bytes into the workspace; the
frame-table form reads them from 8x fewer distinct source rows.  HIP events around --reps back-to-back launches per run,
--runs runs per form after a warm-up, the forms alternating; medians, the materialised runs' own (max - min) / median
spread, the outputs compared bit for bit, and the two sets' device bytes for the window rows.

    python tools/frame_table_gather_bench.py [--runs 30] [--reps 50] [--out profiles/frame_table_gather.txt]
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def record(directory, lengths, seed=40):
    from cadre_amd import replay, synth
    rec = replay.RolloutRecorder(directory)
    paths = []
    for e, n in enumerate(lengths):
        for i, td in enumerate(synth.synth_rollout(n, 84, 84, seed=seed + e)):
            rec.step(dict(rgb=td["rgb"], route_fig=td["route_fig"], measurements=td["measurements"], command=td["command"]),
                     ((7 * i + e) % 33, (i + e) % 3), (-0.5, -0.1), (0.0, 0.0), td["reward"], [False, False])
        paths.append(rec.end_episode())
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_table_gather_bench needs an MI355X: a time taken elsewhere says nothing")
    if args.runs < 20:
        raise SystemExit("at least 20 runs per form")
    from cadre_amd import hip
    from ppo_agent.imitation import DemoSet
    from tools.bc_step_bench import make_agent

    B = 256
    agent = make_agent()
    with tempfile.TemporaryDirectory() as d:
        paths = record(d, (args.rows // 2, args.rows - args.rows // 2))
        sets = {"materialised": DemoSet.from_episodes(agent, paths, gamma=0.99),
                "frame table": DemoSet.from_episodes(agent, paths, gamma=0.99, frame_table=True)}
    a, L, st = agent.arena, hip.lib(), hip.stream()
    w = agent.learner.workspace(B)
    idx = torch.stack([torch.randperm(sets["materialised"].T)[:B] for _ in range(2)]).cuda()
    calls, nbytes = {}, {}
    for name, demo in sets.items():
        ft = demo.frame_table
        rows = []
        for stor in (demo.steer, demo.throttle):
            src = agent._ft_source(stor)
            row = [src[0], hip.ptr(stor._hn), hip.ptr(stor._cn), hip.ptr(stor.action), hip.ptr(stor.value_preds),
                   hip.ptr(stor.returns), hip.ptr(stor.action_log_probs), hip.ptr(stor.command), hip.ptr(demo.weights)]
            rows.append(row + [src[1], src[2]] if ft else row)
        table = torch.tensor(rows, dtype=torch.int64).cuda()
        s0 = demo.steer
        fn = L.cadre_gather_sorted_multi_ft if ft else L.cadre_gather_sorted_multi
        argv = (hip.ptr(table), 2, s0._ldo, s0.seq_length, s0._ldh, hip.ptr(idx), B, a.D, a.D, B, a.C,
                hip.ptr(w["X"]), w["X"].stride(0), a.DP, hip.ptr(w["h0"]), hip.ptr(w["c0"]), w["h0"].stride(0), a.DP,
                hip.ptr(w["actions"]), hip.ptr(w["commands"]), hip.ptr(w["old_values"]), hip.ptr(w["returns"]),
                hip.ptr(w["old_logp"]), hip.ptr(w["adv"]), hip.ptr(w["pos"]), hip.ptr(w["seg"]), st)
        calls[name] = (fn, argv, table)
        nbytes[name] = s0.frame_bytes() if ft else s0._obs.numel() * 4

    def run(name, n):
        fn, argv, _t = calls[name]
        for _ in range(n):
            hip.check(fn(*argv), name)

    outs = {}
    for name in calls:                                       # the same bits in the workspace, whichever form filled it
        w["X"].fill_(-1.0)
        run(name, 1)
        outs[name] = (w["X"].clone(), w["pos"].clone(), w["seg"].clone())
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(*outs.values()))
    for name in calls:
        run(name, args.warmup * args.reps)
    torch.cuda.synchronize()
    res = {name: [] for name in calls}
    for _ in range(args.runs):
        for name in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name, args.reps)
            e1.record()
            torch.cuda.synchronize()
            res[name].append(1000.0 * e0.elapsed_time(e1) / args.reps)
    med = {n_: float(np.median(v)) for n_, v in res.items()}
    ref_ = res["materialised"]
    spread = (max(ref_) - min(ref_)) / med["materialised"]
    slower = med["frame table"] / med["materialised"] - 1.0
    T, F = sets["materialised"].T, sets["frame table"].steer.n_frames
    lines = ["Minibatch gather of a behaviour-cloning step, B = %d, row-sorted, one worker (%s; median of %d runs x %d back-to-back "
             "launches per form, forms alternating, HIP events; launch-to-launch time, launch overhead included)"
             % (B, torch.cuda.get_device_name(0), args.runs, args.reps),
             "set: 2 episodes, %d transitions, %d frames, window of %d; outputs bit-identical: %s" % (T, F, sets["materialised"].steer.seq_length, same)]
    for name in calls:
        lines.append("%-13s %8.2f us/launch   min %.2f  max %.2f   window rows on the device: %d bytes (%.1f KB per transition)"
                     % (name, med[name], min(res[name]), max(res[name]), nbytes[name], nbytes[name] / 1024.0 / T))
    lines.append("materialised runs' own spread (max - min) / median: %.2f %%; frame table against materialised: %+.2f %% -> %s"
                 % (100.0 * spread, 100.0 * slower, "no slower than the spread allows" if slower <= spread else "SLOWER than the spread allows"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
