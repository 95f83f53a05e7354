#!/usr/bin/env python3
"""Env-step latency of N environments: N act() calls (one per environment, each with its own sliding-window cache) against
one CadreAgent.act_batch over the N, with and without the `shifted` hint, at 144x256 and 288x288.

Per env step of all N environments: the wall time on a synchronised host clock (what a rollout loop waits for, incl.
the host work and the copies) and the device time between two events around the step; medians over the timed steps
after warm-up.  `--out FILE` also writes the rows as JSON."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cadre_amd import synth  # noqa: E402
from ppo_agent.agent import CadreAgent  # noqa: E402


def make_agent(H, W):
    fh, fw = synth.feat_hw(H, W)
    cfg = dict(use_lstm=True, vae_device=0, device_num=0, vae_params="CoPM", measurement_dim=18,
               num_output=dict(steer=33, throttle=3), command_num=4, obs_hw=(H, W), weights_init="none",
               vae_state_dict=synth.encoder_state(fh, fw, 7))
    agent = CadreAgent(rank=0, model_cfg=cfg, frame=8, STEER_CONTROL={i: (i - 16) / 16.0 for i in range(33)},
                       THROTTLE_CONTROL={0: [0, 0], 1: [0, 1], 2: [0.6, 0]}, ent_coeff=0.01, value_coeff=0.1,
                       clip_coeff=1.0, clip=0.1)
    agent.arena.load_numpy_state(synth.ppo_state(11))
    return agent


class Streams:
    """N sliding-window observation streams (env_wrapper.py:899-904): a pool of frames per environment, window t =
    frames t .. t + S - 1."""

    def __init__(self, N, H, W, steps, S=8, seed=0):
        r = np.random.RandomState(seed)
        n = steps + S
        self.rgb = [r.randint(0, 256, (n, H, W, 3)).astype(np.uint8) for _ in range(N)]
        self.route = [((r.rand(n, W, H) < 0.15) * 255).astype(np.uint8) for _ in range(N)]
        self.meas = [r.rand(n, 3) for _ in range(N)]
        self.cmd = r.randint(0, 4, (steps, N))
        self.S = S

    def obs(self, e, t):
        S = self.S
        return dict(rgb=self.rgb[e][t:t + S], route_fig=self.route[e][t:t + S].copy(), measurements=self.meas[e][t:t + S],
                    command=int(self.cmd[t, e]))


def run(agent, streams, N, mode, warm, steps):
    wall, dev = [], []
    caches = [None] * N
    agent._vec = None
    for t in range(warm + steps):
        obs = [streams.obs(e, t) for e in range(N)]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        if mode == "act":
            outs = []
            for e in range(N):
                agent._cache = caches[e]
                outs.append(agent.act(obs[e]))
                caches[e] = agent._cache
        else:
            outs = agent.act_batch(obs, shifted=[t > 0] * N if mode == "act_batch+hint" else None)
        e1.record()
        for o in outs:
            agent.convert_action(o[1])               # .item(): the rollout loop reads every action
        torch.cuda.synchronize()
        if t >= warm:
            wall.append(time.perf_counter() - t0)
            dev.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(wall)), float(np.median(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="144x256,288x288")
    ap.add_argument("--envs", default="1,2,4,8,16,32")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for size in a.sizes.split(","):
        H, W = (int(x) for x in size.split("x"))
        agent = make_agent(H, W)
        Ns = [int(x) for x in a.envs.split(",")]
        streams = Streams(max(Ns), H, W, a.warmup + a.steps)
        for N in Ns:
            res = {m: run(agent, streams, N, m, a.warmup, a.steps) for m in ("act", "act_batch", "act_batch+hint")}
            base = res["act"][0]
            for m, (wall, dev) in res.items():
                row = dict(H=H, W=W, N=N, mode=m, wall_ms=wall * 1e3, device_ms=dev * 1e3, env_steps_per_s=N / wall,
                           speedup_vs_act=base / wall)
                rows.append(row)
                print("%dx%d N=%2d %-15s wall %7.2f ms  device %7.2f ms  %8.0f env steps/s  x%.2f vs N act()"
                      % (H, W, N, m, row["wall_ms"], row["device_ms"], row["env_steps_per_s"], row["speedup_vs_act"]),
                      flush=True)
        del agent
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
