#!/usr/bin/env python3
"""Env-step latency of an evaluation ensemble at 144x256: EnsembleEvaluator.act over N environments and M snapshots against
the existing API's loop on the same box — N x (CadreAgent.ensemble_act + avg_action), each environment with its own
sliding-window cache — sampled and greedy (the loop's greedy form: get_latent_feature + act_from_feature(deterministic)).

One process per (N, M) line pair (a fresh child each: no workspace, cache or allocator state carries over).  Inside a
child the two forms run on the same observations, alternating which goes first, and each timed step is the whole step:
from the observations on the host to the [steer, throttle, brake] controls of all N environments on the host (a host
clock around work that ends with the controls read back).  Reported: median and the 10th .. 90th percentile over the
timed steps after warm-up, and the ratio of the medians.  Exit status 1 when at N = 8, M = 6 the evaluator is slower
than the loop.  `--out FILE` also writes the lines there."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, S, C = 144, 256, 8, 4


def make_group(M):
    import torch  # noqa: F401
    from cadre_amd import synth
    from ppo_agent.agent import CadreAgent
    fh, fw = synth.feat_hw(H, W)
    enc = synth.encoder_state(fh, fw, 7)
    group = []
    for m in range(M):
        cfg = dict(use_lstm=True, vae_device=0, device_num=0, vae_params="CoPM", measurement_dim=18,
                   num_output=dict(steer=33, throttle=3), command_num=C, obs_hw=(H, W), weights_init="none", vae_state_dict=enc)
        ag = CadreAgent(rank=0, model_cfg=cfg, frame=S, STEER_CONTROL={i: (i - 16) / 16.0 for i in range(33)},
                        THROTTLE_CONTROL={0: [0, 0], 1: [0, 1], 2: [0.6, 0]}, ent_coeff=0.01, value_coeff=0.1,
                        clip_coeff=1.0, clip=0.1)
        ag.arena.load_numpy_state(synth.ppo_state(11 + m))
        group.append(ag)
    return group


class Streams:
    """N sliding-window observation streams (env_wrapper.py:899-904): a pool of frames per environment, window t =
    frames t .. t + S - 1."""

    def __init__(self, N, steps, seed=0):
        r = np.random.RandomState(seed)
        n = steps + S
        self.rgb = [r.randint(0, 256, (n, H, W, 3), dtype=np.uint8) for _ in range(N)]
        self.route = [((r.rand(n, W, H) < 0.15) * 255).astype(np.uint8) for _ in range(N)]
        self.meas = [r.rand(n, 3) for _ in range(N)]
        self.cmd = r.randint(0, C, (steps, N))

    def obs(self, e, t):
        return dict(rgb=self.rgb[e][t:t + S], route_fig=self.route[e][t:t + S].copy(), measurements=self.meas[e][t:t + S],
                    command=int(self.cmd[t, e]))


def child(N, M, warm, steps):
    import torch
    from ppo_agent.agent import CadreAgent
    from ppo_agent.evaluate import EnsembleEvaluator
    assert torch.cuda.is_available(), "the latency tool needs an MI355X"
    group = make_group(M)
    lead = group[0]
    ev = EnsembleEvaluator(group, max_envs=N)
    for greedy in (False, True):
        streams = Streams(N, warm + steps, seed=int(greedy))
        caches = [None] * N
        ev._vec = None
        times = {"loop": [], "evaluator": []}

        def loop(obs):
            out = []
            for e, o in enumerate(obs):
                lead._cache = caches[e]
                if greedy:
                    feat = lead.get_latent_feature(o)
                    acts = [a.act_from_feature(feat, o["command"], deterministic=True)[1] for a in group]
                else:
                    acts = [t[1] for t in CadreAgent.ensemble_act(group, o)]
                caches[e] = lead._cache
                out.append(lead.avg_action(acts))
            return out

        def evaluator(obs):
            return ev.act(obs, deterministic=greedy).controls
        torch.manual_seed(1)
        for t in range(warm + steps):
            order = (("loop", loop), ("evaluator", evaluator)) if t % 2 == 0 else (("evaluator", evaluator), ("loop", loop))
            for name, fn in order:
                obs = [streams.obs(e, t) for e in range(N)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctl = fn(obs)
                dt = time.perf_counter() - t0              # (the controls are Python floats here: the device work is done)
                assert len(ctl) == N
                if t >= warm:
                    times[name].append(dt)
        row = dict(N=N, M=M, mode="greedy" if greedy else "sampled", steps=steps)
        for name, ts in times.items():
            ts = np.asarray(ts) * 1e3
            row[name] = dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)))
        row["ratio"] = row["loop"]["median_ms"] / row["evaluator"]["median_ms"]
        print("ROW " + json.dumps(row), flush=True)


def fmt(row):
    l, e = row["loop"], row["evaluator"]
    return ("N=%2d M=%d %-7s loop %8.2f ms (%.2f .. %.2f)   evaluator %7.2f ms (%.2f .. %.2f)   loop / evaluator x%.2f   [%d steps]"
            % (row["N"], row["M"], row["mode"], l["median_ms"], l["p10_ms"], l["p90_ms"], e["median_ms"], e["p10_ms"], e["p90_ms"],
               row["ratio"], row["steps"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="1,8,32")
    ap.add_argument("--agents", default="1,3,6")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--child", nargs=2, type=int, default=None, metavar=("N", "M"))
    ap.add_argument("--child-timeout", type=int, default=600)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.warmup, a.steps)
    lines, rows = [], []
    for N in (int(x) for x in a.envs.split(",")):
        for M in (int(x) for x in a.agents.split(",")):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(N), str(M), "--warmup", str(a.warmup),
                                "--steps", str(a.steps)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                               timeout=a.child_timeout)
            if p.returncode != 0:                          # a failed child ends the run: nothing more is started on the device
                print(p.stdout)
                print("child N=%d M=%d failed with status %d" % (N, M, p.returncode))
                return 2
            for ln in p.stdout.splitlines():
                if ln.startswith("ROW "):
                    rows.append(json.loads(ln[4:]))
                    lines.append(fmt(rows[-1]))
                    print(lines[-1], flush=True)
    import torch
    head = ["ensemble evaluation, env-step latency at %dx%d on %s" % (H, W, torch.cuda.get_device_name(0)),
            "whole step, observations on the host -> controls on the host; median (10th .. 90th percentile); one process per (N, M)"]
    bad = [r for r in rows if r["N"] == 8 and r["M"] == 6 and r["ratio"] < 1.0]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(head + lines) + "\n")
    if bad:
        print("FAIL: at N = 8, M = 6 the evaluator is slower than the loop")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
