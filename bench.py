#!/usr/bin/env python3
"""bench.py — PPO-update throughput of the MI355X-native Cadre learner (BASELINE.json metric).

One "step" = one learner ROUND over one batch of synthetic rollouts:
  encode every window of W*T transitions (8 frames each, reference convention — the
  reference re-encodes all 8 frames of the sliding window at every env step) -> fill the
  rollout storages -> get_value -> GAE + advantage normalisation -> ppo_epoch(4) x
  mini_batch_num(2) x (update_policy + gradient all-reduce(SUM) + per-model clip + Adam).
value = (n_gpus * W * T) / t_round  [samples/s], inputs resident in HBM before timing.

    python bench.py                       # N=1, config C2: 1 worker x 128 steps, 288x288, fp32
    python bench.py --full                # + nested C3 section, latent-cache / direct-conv / stem rounds, rooflines, peaks, CPU baseline
    python bench.py --dump-outputs DIR    # + what the last timed round computed, as DIR/<name>.npy
    python bench.py --gpus N              # N ranks: the parent (no GPU call) starts one child per GPU and relays the line
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

T_START = time.perf_counter()
CONFIGS = {
    "C1": dict(workers=1, T=32, H=84, W=84),
    "C2": dict(workers=1, T=128, H=288, W=288),
    "C3": dict(workers=4, T=128, H=288, W=288, encoder_dtype="bf16"),   # "bf16 encoder / fp32 losses"
}
PEAK_F32_MFMA_TFLOPS = 157.3        # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 2500.0      # MI355X_MICROARCH.md: dense bf16 MFMA peak (no sparsity)
PEAK_HBM_GBPS = 8000.0              # MI355X_MICROARCH.md: HBM3E peak (6.3 TB/s achievable)
PPO_EPOCH, MINI_BATCH_NUM, SEQ = 4, 2, 8
# reference config/train_config.py values the learner section reads
TRAIN_CFG = dict(use_adv_norm=True, ppo_epoch=PPO_EPOCH, max_grad_norm=250.0, lr=3e-4)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


class Worker:
    """One logical CARLA worker: sliding-window observations resident in HBM + its two storages.
    Synthetic by default, or one recorded episode (cadre_amd/replay.py, config C5)."""

    def __init__(self, cfg, seed, device, episode=None):
        from ppo_agent.storage import RolloutStorage
        T, H, W = cfg["T"], cfg["H"], cfg["W"]
        rng = np.random.RandomState(seed)
        if episode is None:
            nf = T + SEQ - 1
            rgb = rng.randint(0, 256, (nf, H, W, 3)).astype(np.uint8)
            route = ((rng.rand(nf, W, H) < 0.15) * 255).astype(np.uint8)
            meas = rng.rand(nf, 3)
            win = (np.arange(T).reshape(T, 1) + np.arange(SEQ).reshape(1, SEQ)).reshape(-1)
            rec = None
        else:
            rgb, route, meas = episode["rgb"], episode["route"], episode["measurements"]
            win = episode["window"][:T].reshape(-1).astype(np.int64)
            rec = episode
        self.rgb = torch.from_numpy(rgb).to(device)
        self.route = torch.from_numpy(route).to(device)
        self.win = torch.from_numpy(win).to(device)                                                     # frame ids
        self.meas = torch.from_numpy(meas).to(device)[self.win].contiguous()                            # [T*S,3] f64
        self.stor = []
        for j, K in enumerate((33, 3)):
            s = RolloutStorage(T, MINI_BATCH_NUM, 530, SEQ, 530, True, 0.99, 0.95)
            if rec is None:
                s.action.copy_(torch.from_numpy(rng.randint(0, K, (T + 1, 1))))
                s.action_log_probs.copy_(torch.from_numpy((-np.log(K) + 0.1 * rng.standard_normal((T + 1, 1))).astype(np.float32)))
                s.value_preds.copy_(torch.from_numpy((0.3 * rng.standard_normal((T + 1, 1))).astype(np.float32)))
                s.rewards.copy_(torch.from_numpy(rng.rand(T + 1, 1).astype(np.float32)))
                s.masks.copy_(torch.from_numpy((rng.rand(T + 1, 1) >= 0.02).astype(np.float32)))
                s.command.copy_(torch.from_numpy(rng.randint(0, 4, (T + 1, 1)).astype(np.int32)))
            else:
                s.action[:T, 0] = torch.from_numpy(rec["action"][:T, j])
                s.action_log_probs[:T, 0] = torch.from_numpy(rec["action_log_prob"][:T, j])
                s.value_preds[:T, 0] = torch.from_numpy(rec["value"][:T, j])
                s.rewards[:T, 0] = torch.from_numpy(rec["reward"][:T, j])
                s.masks[:T, 0] = torch.from_numpy(1.0 - rec["done"][:T, j].astype(np.float32))
                s.command[:T, 0] = torch.from_numpy(rec["command"][:T])
            s.to(device)
            self.stor.append(s)


def encode_worker(agent, wk, cfg, chunk_windows):
    """a2/a3: all T windows x 8 frames through the HIP encoder, latent rows written straight into
    the steer storage's 544-pitch feature buffer, measurements appended, copied to throttle."""
    from cadre_amd import hip
    T = cfg["T"]
    enc = agent.vae_model
    obs_rows = wk.stor[0]._obs.view(-1, wk.stor[0]._ldo)          # [(T+1)*S, 544]
    L = hip.lib()
    if cfg.get("dedup"):
        # sliding-window latent cache: each of the T+S-1 distinct frames is encoded
        # once (bit-identical per-frame results), windows are assembled by a row gather
        nf = wk.rgb.shape[0]
        if getattr(wk, "lat", None) is None:
            wk.lat = torch.zeros(nf, 512, device=wk.rgb.device)
        step = chunk_windows * SEQ
        for f0 in range(0, nf, step):
            f1 = min(nf, f0 + step)
            enc.forward_nhwc(enc.preprocess(wk.rgb[f0:f1], wk.route[f0:f1]), wk.lat[f0:f1])
        obs_rows[:T * SEQ, :512].copy_(wk.lat.index_select(0, wk.win))
        hip.check(L.cadre_append_measurements(hip.ptr(wk.meas), hip.ptr(obs_rows), obs_rows.stride(0), T * SEQ,
                                              hip.stream()), "cadre_append_measurements")
        chunk_windows = T + 1                                     # skip the per-window loop below
    for t0 in range(0, T if not cfg.get("dedup") else 0, chunk_windows):
        t1 = min(T, t0 + chunk_windows)
        ids = wk.win[t0 * SEQ:t1 * SEQ]
        x = enc.preprocess(wk.rgb, wk.route, frame_idx=ids)      # window gather rides on the packing pass
        rows = obs_rows[t0 * SEQ:t1 * SEQ]
        enc.forward_nhwc(x, rows)
        hip.check(L.cadre_append_measurements(hip.ptr(wk.meas[t0 * SEQ:t1 * SEQ]), hip.ptr(rows), rows.stride(0),
                                              (t1 - t0) * SEQ, hip.stream()), "cadre_append_measurements")
    obs_rows[T * SEQ:].copy_(obs_rows[(T - 1) * SEQ:T * SEQ])      # row T (bootstrap obs) = last window
    wk.stor[1]._obs.copy_(wk.stor[0]._obs)


class JointFrames:
    """The W workers of one GPU encoded as ONE stream of windows (configs with several workers per GPU): their frames
    in one tensor, window ids offset per worker, chunks of `chunk_windows` windows cut across workers — twice the work
    items per launch of a per-worker chunk, so the persistent conv kernels lose less to the last partial round of items
    (layer4 at 1024 frames: 5.06 items per CU -> 6 rounds).  Same per-frame results: frames are independent."""

    def __init__(self, workers):
        self.rgb = torch.cat([w.rgb for w in workers])
        self.route = torch.cat([w.route for w in workers])
        base = np.cumsum([0] + [int(w.rgb.shape[0]) for w in workers[:-1]])
        self.win = torch.cat([w.win + int(b) for w, b in zip(workers, base)])
        self.meas = torch.cat([w.meas for w in workers])
        self.lat = None


def encode_joint(agent, workers, joint, cfg, chunk_windows):
    from cadre_amd import hip
    T = cfg["T"]
    enc = agent.vae_model
    L = hip.lib()
    nwin = T * len(workers)
    ldo = workers[0].stor[0]._ldo
    if joint.lat is None:
        joint.lat = torch.zeros(nwin * SEQ, ldo, device=joint.rgb.device)
    for t0 in range(0, nwin, chunk_windows):
        t1 = min(nwin, t0 + chunk_windows)
        x = enc.preprocess(joint.rgb, joint.route, frame_idx=joint.win[t0 * SEQ:t1 * SEQ])
        rows = joint.lat[t0 * SEQ:t1 * SEQ]
        enc.forward_nhwc(x, rows)
        hip.check(L.cadre_append_measurements(hip.ptr(joint.meas[t0 * SEQ:t1 * SEQ]), hip.ptr(rows), rows.stride(0),
                                              (t1 - t0) * SEQ, hip.stream()), "cadre_append_measurements")
    for w, wk in enumerate(workers):
        obs_rows = wk.stor[0]._obs.view(-1, ldo)
        obs_rows[:T * SEQ].copy_(joint.lat[w * T * SEQ:(w + 1) * T * SEQ])
        obs_rows[T * SEQ:].copy_(obs_rows[(T - 1) * SEQ:T * SEQ])
        wk.stor[1]._obs.copy_(wk.stor[0]._obs)


def learner_round(agent, workers, cfg, shared, timers=None, joint=None, losses_to_host=True):
    """One learner round.  timers (list, untimed split pass only): receives (t_encode, t_update, step_ms) with step_ms the
    HIP-event time of each of the 8 minibatch steps (gather + update_policy + gradient exchange + clip + Adam)."""
    from ppo_agent.chief import chief_step
    from ppo_agent.train import learner_section
    t0 = time.perf_counter()
    host = [] if os.environ.get("CADRE_BENCH_HOST_TRACE") else None      # host-side enqueue times of the round's phases (no syncs added)
    if joint is not None:
        encode_joint(agent, workers, joint, cfg, cfg["chunk_windows"])
    else:
        for wk in workers:
            encode_worker(agent, wk, cfg, cfg["chunk_windows"])
    if host is not None:
        host.append(("encode enqueued", time.perf_counter() - t0))
    if timers is not None:
        torch.cuda.synchronize(); t1 = time.perf_counter()
    if len(workers) == 1:
        # ONE worker per GPU (C1 / C2): the learner section is the function train() itself runs
        # (cadre_amd/ppo_agent/train.py:learner_section = reference train.py:76-110) — bootstrap values, GAE,
        # 4 epochs x 2 minibatches of update_policy + hand-off + in-process chief_step; nothing bench-specific
        evs = [] if timers is not None else None
        dev_l = learner_section(agent, workers[0].stor[0], workers[0].stor[1], False, TRAIN_CFG, shared,
                                in_process_chief=True, losses_on_device=True, step_events=evs)
        if host is not None:
            host.append(("updates enqueued", time.perf_counter() - t0))
        if not losses_to_host:
            return dev_l
        losses = dev_l.tolist()
        if host is not None:
            host.append(("losses on the host", time.perf_counter() - t0))
            log("[bench] host timeline (ms since round start): " + ", ".join("%s %.2f" % (k, 1e3 * v) for k, v in host))
        if timers is not None:
            torch.cuda.synchronize(); t2 = time.perf_counter()
            timers.append((t1 - t0, t2 - t1, [evs[i].elapsed_time(evs[i + 1]) for i in range(len(evs) - 1)]))
        return losses
    advs = []
    # (commands stay on the device: .item() in get_last would wait for the encoder pass and expose ~1 ms of host work)
    if len(workers) > 1:      # bootstrap values of all workers in one LSTM + critic pass
        vals = agent.get_values([(wk.stor[0].get_last(as_tensor=True), wk.stor[1].get_last(as_tensor=True)) for wk in workers])
    else:
        vals = [agent.get_value(False, wk.stor[0].get_last(as_tensor=True), wk.stor[1].get_last(as_tensor=True)) for wk in workers]
    if host is not None:
        host.append(("bootstrap values enqueued", time.perf_counter() - t0))
    for wk, (nv_s, nv_t) in zip(workers, vals):
        advs.append((wk.stor[0].compute_returns(nv_s), wk.stor[1].compute_returns(nv_t)))
    if host is not None:
        host.append(("GAE enqueued", time.perf_counter() - t0))
    nW = len(workers)
    dev_losses = []
    hook = shared.overlap_hook(agent.arena)  # several ranks + --grad-buckets: MLP and steer-LSTM gradient buckets out beside the rest of the backward
    evs = []
    for _ in range(PPO_EPOCH):
        idx = [(wk.stor[0].sample_indices(), wk.stor[1].sample_indices()) for wk in workers]
        for b in range(len(idx[0][0])):
            batches = [(wk.stor[0], idx[i][0][b], advs[i][0], wk.stor[1], idx[i][1][b], advs[i][1])
                       for i, wk in enumerate(workers)]
            if timers is not None:
                evs.append(torch.cuda.Event(enable_timing=True)); evs[-1].record()
            dev_losses.append(agent.update_policy_from_storages(batches, sync=False, mlp_grads_ready=hook))
            shared.add_gradient(agent.model_dict)                 # hand-off; chief_step runs the cross-rank exchange (SUM)
            chief_step(shared, None, 250.0, zero_grads=False)     # next writer: the fused update (overwrites)
    if timers is not None:
        evs.append(torch.cuda.Event(enable_timing=True)); evs[-1].record()
    if host is not None:
        host.append(("updates enqueued", time.perf_counter() - t0))
    if not losses_to_host:                                        # the caller reads them later: the host never waits inside a round
        return torch.stack(dev_losses)
    losses = torch.stack(dev_losses).tolist()                     # the round's single host sync
    if host is not None:
        host.append(("losses on the host", time.perf_counter() - t0))
        log("[bench] host timeline (ms since round start): " + ", ".join("%s %.2f" % (k, 1e3 * v) for k, v in host))
    if timers is not None:
        torch.cuda.synchronize(); t2 = time.perf_counter()
        timers.append((t1 - t0, t2 - t1, [evs[i].elapsed_time(evs[i + 1]) for i in range(len(evs) - 1)]))
    return losses


def host_cores():
    """CPU threads this process may really use: affinity mask capped by the cgroup CPU quota
    (os.cpu_count() reports the whole machine inside a container and oversubscribes OpenMP)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q = open("/sys/fs/cgroup/cpu.max").read().split()
        if q[0] != "max":
            n = min(n, max(1, int(int(q[0]) / int(q[1]))))
    except (OSError, ValueError, IndexError):
        try:
            quota = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            period = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if quota > 0:
                n = min(n, max(1, quota // period))
        except (OSError, ValueError):
            pass
    return max(1, min(n, 64))


def cpu_baseline(cfg, enc_state, ppo_state):
    """Oracle (kind 'port') on the host cores, bounded sample, extrapolated to one round."""
    from oracle import encoder_ref, ppo_ref
    from cadre_amd import synth
    ncores = host_cores()
    torch.set_num_threads(ncores)
    log("[bench] cpu_baseline on %d host threads (os.cpu_count()=%s)" % (ncores, os.cpu_count()))
    T, H, W, nW = cfg["T"], cfg["H"], cfg["W"], cfg["workers"]
    td = synth.synth_rollout(2, H, W, seed=1)
    t0 = time.perf_counter()
    nwin = 0
    while nwin < 1 or (time.perf_counter() - t0 < 8.0 and nwin < 128):      # ~8 s of encoder windows
        encoder_ref.latent_feature(td[nwin % 2]["rgb"], td[nwin % 2]["route_fig"], td[nwin % 2]["measurements"], enc_state)
        nwin += 1
    t_win = (time.perf_counter() - t0) / nwin
    params = ppo_ref.to_torch_params(ppo_state, requires_grad=True)
    adam = {m: {k: (torch.zeros_like(p), torch.zeros_like(p)) for k, p in d.items()} for m, d in params.items()}
    r = np.random.RandomState(0)
    B = T // MINI_BATCH_NUM
    samp = []
    for K in (33, 3):
        samp.append((torch.from_numpy((r.standard_normal((SEQ * B, 530)) * 0.5).astype(np.float32)),
                     torch.from_numpy(r.randint(0, K, (B, 1)).astype(np.int64)),
                     torch.from_numpy((0.3 * r.standard_normal((B, 1))).astype(np.float32)),
                     torch.from_numpy(r.standard_normal((B, 1)).astype(np.float32)), torch.ones(B, 1),
                     torch.from_numpy((-np.log(K) + 0.1 * r.standard_normal((B, 1))).astype(np.float32)),
                     torch.from_numpy(r.standard_normal((B, 1)).astype(np.float32)),
                     [torch.zeros(B, 530), torch.zeros(B, 530)], torch.from_numpy(r.randint(0, 4, (B, 1)).astype(np.int32))))
    t0 = time.perf_counter()
    nup = 0
    while nup < 1 or (time.perf_counter() - t0 < 8.0 and nup < 128):          # ~8 s of update steps
        ppo_ref.update_policy(params, samp[0], samp[1])
        grads = {m: {k: p.grad for k, p in d.items()} for m, d in params.items()}
        ppo_ref.chief_step(params, grads, adam, nup + 1)
        nup += 1
    t_up = (time.perf_counter() - t0) / nup
    t_round = nW * T * t_win + nW * PPO_EPOCH * MINI_BATCH_NUM * t_up
    return dict(value=nW * T / t_round, unit="samples/s", cores=ncores, kind="port",
                sample="oracle (torch-CPU restatement, %d threads): %d encoder windows of 8 frames at %dx%d (%.3f s each) + "
                       "%d update_policy+clip+Adam steps at minibatch %d (%.3f s each), extrapolated to one round of "
                       "%d windows + %d updates" % (ncores, nwin, H, W, t_win, nup, B, t_up, nW * T,
                                                   nW * PPO_EPOCH * MINI_BATCH_NUM))


# tile id -> (WM, WN, WVN, WVM) template arguments of gemm_f32_kernel<WM, WN, AMODE, BMODE, WVN, NS, WVM>
TPL_F32 = {1: (2, 2, 2, 2), 2: (2, 1, 2, 2), 3: (1, 1, 2, 2), 4: (4, 2, 2, 2), 5: (2, 4, 2, 2), 6: (4, 1, 2, 2), 8: (2, 1, 4, 2),
           9: (1, 1, 4, 1), 10: (1, 1, 2, 4)}
# tile id -> (WM, WN, WVN, NS, WVM) of gemm_bf16_kernel<WM, WN, AMODE, WVN, NS, WVM>
TPL_BF16 = {1: (2, 2, 2, 2, 2), 2: (2, 1, 2, 2, 2), 3: (1, 1, 2, 2, 2), 4: (4, 2, 2, 1, 2), 7: (4, 2, 4, 1, 2),
            10: (1, 1, 2, 2, 4), 11: (2, 1, 2, 2, 4)}
TILE = {1: "128x128", 2: "128x64", 3: "64x64", 4: "256x128", 5: "128x256", 6: "256x64", 7: "256x256 (8 waves)",
        8: "128x128 (8 waves)", 9: "32x128", 10: "128x64 (8 waves)", 11: "256x64 (8 waves)",
        12: "64x64, 8 M-tiles per workgroup", 64: "128 positions x 64, weights resident in LDS, pixel ring",
        65: "128/256 positions x 64/128, pixel window resident in LDS",
        66: "256x256 on four waves (128x128 each), B streamed to registers in fragment order"}
AM = {0: "dense A[M][K]", 1: "dense A[K][M]", 2: "NHWC implicit-GEMM conv", 3: "Cin=4 stem conv",
      4: "Cin=4 stem conv on the zero-padded image"}


def kname(k):
    """Exact kernel symbol as rocprofv3 prints it, from a hip.PROFILE key."""
    if k[0] == "wino_c64":
        return "wino2_c64_kernel<%s>" % ("true" if k[1] else "false")
    if k[0] == "wgo":
        return "wino_gemm_out_kernel<%d, %d>" % (k[1], k[2])
    if k[0] == "gw128":
        return "gemm_bf16_w128_kernel"
    if k[0] == "s2":
        return "conv3x3_s2_kernel<%d>" % k[1]
    if k[0] == "s1x":
        return "conv3x3_s1x_kernel<%d, %d>" % (k[1], k[2])
    if k[0] == "ring":
        tf = ("true" if k[1] else "false", k[2], k[3], "true" if k[4] else "false")
        if len(k) > 7 and k[7] == 8:             # one wave per SIMD, streamed weights (128-channel tile)
            return "conv3x3_ring1w_kernel<%d, %s>" % (k[3], tf[3])
        if len(k) > 7 and k[7] == 9:             # the weight-stationary 64 -> 64 stage
            return "conv3x3_c64s_kernel<%d, %s>" % (k[3], tf[3])
        if len(k) > 7 and k[7]:                  # G k-tiles per ping-pong slot (bf16)
            return "conv3x3_ring_pp2_kernel<%d, %d, %s, %d>" % (k[2], k[3], tf[3], k[7])
        return "conv3x3_ring_pp_kernel<%s, %d, %d, %s, false>" % tf if k[6] else ("conv3x3_ring_kernel<%s, %d, %d, %s, %%d>" % tf) % k[5]
    if k[0] == "bf16":
        _, tile, am = k
        if tile == 12:
            return "conv_stream_bf16_kernel<%d>" % am
        if tile == 64:
            return "conv3x3_c64_bf16_v2_kernel"

        wm_, wn_, wvn_, ns_, wvm_ = TPL_BF16[tile]
        return "gemm_bf16_kernel<%d, %d, %d, %d, %d, %d>" % (wm_, wn_, am, wvn_, ns_, wvm_)
    if k[0] == 12:
        return "conv_stream_f32_kernel<%d>" % k[1]

    wm_, wn_, wvn_, wvm_ = TPL_F32[k[0]]
    return "gemm_f32_kernel<%d, %d, %d, %d, %d, 2, %d>" % (wm_, wn_, k[1], k[2], wvn_, wvm_)


def roofline_of(prof, steps):
    """Dominant (most time) GEMM/conv kernel of the timed region, priced against BOTH roofs:
    t_mfma = algorithmic FLOPs / MFMA peak of its dtype, t_hbm = algorithmic bytes / HBM peak; the larger
    one is the bound, frac = that time / measured time."""
    by = {}
    for key, flops, e0, e1, _shape, nbytes in prof:
        d = by.setdefault(key, [0.0, 0.0, 0, 0.0])
        d[0] += flops; d[1] += e0.elapsed_time(e1) * 1e-3; d[2] += 1; d[3] += nbytes
    if not by:
        return None, {}
    dom = max(by, key=lambda k: by[k][1])
    fl, t, n, nb = by[dom]
    bf16 = dom[0] in ("bf16", "s2", "s1x", "gw128") or (dom[0] == "ring" and dom[1])
    peak_tf = PEAK_BF16_MFMA_TFLOPS if bf16 else PEAK_F32_MFMA_TFLOPS
    t_mfma, t_hbm = fl / (peak_tf * 1e12), nb / (PEAK_HBM_GBPS * 1e9)
    tile, am = (65, 2) if dom[0] in ("ring", "s2", "s1x") else ((66, 0) if dom[0] == "gw128" else ((dom[1], dom[2]) if bf16 else (dom[0], dom[1])))
    desc = "%s tile, %s%s" % (TILE.get(tile, tile), AM.get(am, am), ", bf16" if bf16 else "")
    if dom[0] == "wino_c64":
        desc = "fused Winograd F(2x2,3x3) of the fp32 64 -> 64 stage (executed FLOPs)"
    if dom[0] == "wgo":
        desc = "Winograd F(%dx%d,3x3) plane products + inverse transform in one kernel (executed FLOPs)" % (dom[1], dom[1])
    r = {"kernel": kname(dom), "kernel_desc": desc,
         "flops_per_launch": round(fl / n, 1), "bytes_per_launch": round(nb / n, 1), "launches": n,
         "avg_launch_us": round(t / n * 1e6, 2),
         "mfma_frac": round(t_mfma / t, 4), "hbm_frac": round(t_hbm / t, 4),
         "achieved_tflops": round(fl / t / 1e12, 2), "achieved_GBps": round(nb / t / 1e9, 1)}
    if t_mfma >= t_hbm:
        r.update(bound="mfma", achieved=round(fl / t / 1e12, 2), peak=peak_tf, unit="TFLOP/s", frac=round(t_mfma / t, 4))
    else:
        r.update(bound="hbm", achieved=round(nb / t / 1e9, 1), peak=PEAK_HBM_GBPS, unit="GB/s", frac=round(t_hbm / t, 4))
    r["per_kernel"] = {kname(k): {"tflops": round(v[0] / v[1] / 1e12, 2), "GBps": round(v[3] / v[1] / 1e9, 1),
                                  "time_ms_per_step": round(v[1] / steps * 1e3, 3), "launches_per_step": v[2] // steps}
                       for k, v in sorted(by.items(), key=lambda kv: -kv[1][1])}
    return dom, r


DUMP_PARAMS_SAMPLE = 1 << 22       # parameter entries written by --dump-outputs (16 MB; the arena holds ~20 M)
DUMP_SEED = 20240607


def dump_outputs(dump_dir, agent, workers, dev_l):
    """--dump-outputs: what the last timed round handed its caller — the per-minibatch losses, the parameters after the
    round's last Adam step (a fixed, seeded sample of the arena), the encoder features written into the rollout storages and
    the returns / advantages of both heads — as DIR/<name>.npy in float32 (< 64 MB in all)."""
    os.makedirs(dump_dir, exist_ok=True)
    params = agent.arena.params
    n = params.numel()
    if n > DUMP_PARAMS_SAMPLE:
        idx = np.sort(np.random.RandomState(DUMP_SEED).choice(n, DUMP_PARAMS_SAMPLE, replace=False))
        params = params[torch.from_numpy(idx).to(params.device)]
    arrays = {
        "losses": torch.as_tensor(dev_l, dtype=torch.float32),
        "params_sample": params,
        "features": torch.stack([wk.stor[0].obs for wk in workers]),
        "returns": torch.stack([torch.stack([s.returns for s in wk.stor]) for wk in workers]),
        "advantages": torch.stack([torch.stack([s.advantages for s in wk.stor]) for wk in workers]),
    }
    total = 0
    for k, v in arrays.items():
        a = v.detach().float().cpu().numpy()
        total += a.nbytes
        np.save(os.path.join(dump_dir, k + ".npy"), a)
    assert total <= 64 << 20, total
    log("[bench] outputs of the last timed round written to %s (%s; %.1f MB)" % (dump_dir, ", ".join(arrays), total / 2**20))


def run_config(name, args, rank, local_rank, world, use_dist, steps, warmup, episodes_dir=None, dedup=None, section=None,
               dump_dir=None):
    """Build the agent + workers of BASELINE config `name`, warm up, time `steps` learner rounds (barrier +
    synchronize on both sides, MAX over ranks) and return the result dict (rank 0) plus what cpu_baseline needs.
    Without --full that is all; --full adds the per-kernel launch profile of the timed region, three untimed split rounds
    (t_encode / t_update, update roofline) and, at N > 1, the exchange timing and parameter checksums."""
    import torch.distributed as dist
    from cadre_amd import hip, synth
    from ppo_agent.agent import CadreAgent
    from ppo_agent.models import Shared_grad_buffers
    dedup = args.dedup if dedup is None else dedup
    cfg = dict(CONFIGS[name]); cfg["dedup"] = dedup
    # windows per encoder launch chain: 128 (1024 frames) per worker; with several workers per GPU their windows form
    # one stream cut into chunks of 256 (2048 frames: every activation tensor stays below the 2 GiB buffer window)
    joint_ok = cfg["workers"] > 1 and not dedup and not episodes_dir and not args.no_joint_encode
    cw = args.chunk_windows if args.chunk_windows else (256 if joint_ok else 128)
    cfg["chunk_windows"] = cw
    episodes = None
    if episodes_dir:
        from cadre_amd import replay
        paths = replay.list_episodes(episodes_dir)
        if len(paths) < cfg["workers"] * world:
            raise SystemExit("--replay needs >= %d episodes, found %d" % (cfg["workers"] * world, len(paths)))
        episodes = [replay.load_episode(p) for p in paths[rank * cfg["workers"]:(rank + 1) * cfg["workers"]]]
        cfg["T"] = min(len(e["command"]) for e in episodes)
        cfg["H"], cfg["W"] = episodes[0]["rgb"].shape[1:3]
    H, W, T, nW = cfg["H"], cfg["W"], cfg["T"], cfg["workers"]
    fh, fw = synth.feat_hw(H, W)
    enc_state = synth.encoder_state(fh, fw, 7)
    ppo_state = synth.ppo_state(11)
    enc_dtype = args.encoder_dtype or cfg.get("encoder_dtype", "f32")
    mcfg = dict(use_lstm=True, vae_device=local_rank, device_num=local_rank, vae_params="CoPM", measurement_dim=18,
                num_output=dict(steer=33, throttle=3), command_num=4, obs_hw=(H, W), weights_init="none", vae_state_dict=enc_state,
                encoder_max_frames=cw * SEQ, encoder_dtype=enc_dtype)
    agent = CadreAgent(rank=rank, model_cfg=mcfg, frame=SEQ, STEER_CONTROL={i: (i - 16) / 16.0 for i in range(33)},
                       THROTTLE_CONTROL={0: [0, 0], 1: [0, 1], 2: [0.6, 0]}, ent_coeff=0.01, value_coeff=0.1,
                       clip_coeff=1.0, clip=0.1)
    agent.arena.load_numpy_state(ppo_state)                      # identical start on every rank (startup broadcast)
    if use_dist:
        dist.broadcast(agent.arena.params, 0)
    dev = agent.device
    workers = [Worker(cfg, 1234 + 1000 * rank + w, dev, None if episodes is None else episodes[w]) for w in range(nW)]
    joint = JointFrames(workers) if joint_ok else None
    shared = Shared_grad_buffers(agent.model_dict, dev)
    torch.manual_seed(100 + rank)

    def sync():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize()

    log("[bench] %s setup done, %d worker(s), %.1f s since start" % (name, nW, time.perf_counter() - T_START))
    for _ in range(warmup):
        learner_round(agent, workers, cfg, shared, joint=joint)
    sync()
    log("[bench] %s warmup done %.1f s" % (name, time.perf_counter() - T_START))
    n_ex0 = shared.n_allreduce
    hip.PROFILE = prof = [] if args.full else None
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    for i in range(steps):
        marks[i].record()
        # losses stay on the device until the region's closing sync (a per-round .tolist() leaves the GPU idle for the
        # ~0.2 ms the host needs to get the next round's first launches out)
        dev_l = learner_round(agent, workers, cfg, shared, joint=joint, losses_to_host=bool(os.environ.get("CADRE_BENCH_SYNC_LOSSES")))
    marks[steps].record()
    sync()
    elapsed = time.perf_counter() - t0
    losses = dev_l if isinstance(dev_l, list) else dev_l.tolist()
    hip.PROFILE = None
    n_ex = shared.n_allreduce - n_ex0
    per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    log("[bench] %s timed region %.3f s for %d steps" % (name, elapsed, steps))
    if dump_dir and rank == 0:
        dump_outputs(dump_dir, agent, workers, dev_l)
    if use_dist:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    ms = elapsed / steps * 1e3
    frames = nW * (T + SEQ - 1 if dedup else T * SEQ)
    n_wino = agent.vae_model.winograd_convs()
    out = {
        "value": round(world * nW * T / (elapsed / steps), 2), "ms_per_step": round(ms, 3), "steps": steps, "warmup": warmup,
        "dtype": "f32" if enc_dtype == "f32" else "bf16 encoder (fp32 accumulate) / f32 PPO update",
        "data": "synthetic" if episodes is None else "replayed records from %s" % episodes_dir,
        "config": {"workload": "%s: %d worker(s) x %d-step rollout, %dx%dx3 synthetic obs (+route), DANet encoder "
                               "(%s) + PPO update (4 epochs x 2 minibatches), %s"
                               % (name, nW, T, H, W,
                                  "latent cache: each distinct frame encoded once" if dedup
                                  else "8 frames/transition, reference convention",
                                  "fp32" if enc_dtype == "f32" else "bf16 encoder / fp32 losses"),
                   "workers_per_gpu": nW, "num_steps": T, "obs": [H, W], "minibatch_per_gpu": nW * T // MINI_BATCH_NUM,
                   "parallelism": "dp%d" % world, "frames_per_round_per_gpu": frames,
                   "conv_algorithm": ("Winograd in fp32 on %d stride-1 3x3 convs: F(4x4,3x3) on the 36x36 maps (layer2: plane products and inverse "
                                      "transform in one kernel), F(6x6,3x3) on the 18x18 maps (layer3), F(3x3,3x3) on the 9x9 maps (layer4, head) — exact "
                                      "tilings —, the fused F(2x2,3x3) kernel on the 64-channel stage (layer1); direct convolution elsewhere; "
                                      "CADRE_WINOGRAD=0 = direct everywhere (c2_direct_conv)" % n_wino) if n_wino else "direct"},
        "ms_per_step_min_median_max": [round(per_step[0], 3), round(per_step[len(per_step) // 2], 3), round(per_step[-1], 3)],
        "last_losses": [round(x, 6) for x in losses[-1]],
    }
    if args.full:
        out.update(full_figures(agent, workers, cfg, shared, joint, prof, steps, section, dedup, enc_dtype, frames))
    if use_dist and args.full:
        out.update(exchange_figures(agent, shared, world, n_ex, sync))
    del workers, shared, agent
    torch.cuda.empty_cache()
    return out, cfg, enc_state, ppo_state


def full_figures(agent, workers, cfg, shared, joint, prof, steps, section, dedup, enc_dtype, frames):
    """--full: rooflines of the timed region's launch profile and the t_encode / t_update split of three untimed rounds."""
    T, nW, cw = cfg["T"], cfg["workers"], cfg["chunk_windows"]
    # ---- per-kernel roofline from the HIP events recorded (on the launch stream) inside the timed region
    dom, roof = roofline_of(prof, steps)
    if roof is not None:
        # HBM bytes per launch of the dominant kernel from the rocprofv3 PMC passes of `bench.py --section <section>` (tools/
        # prof_bench.sh): ONE section per profiled command, so the counter averages and the HIP-event averages above describe
        # the same launches (until round 5 the file was keyed by kernel name over a six-section command: VERDICT r5 "weak" 2)
        traffic, tl, tr = None, None, None
        tpath = os.path.join(ROOT, "profiles", "hbm_traffic.json")
        if section and os.path.exists(tpath):
            try:
                sec_t = json.load(open(tpath)).get(section, {})
                ent = sec_t.get("kernels", {}).get(roof["kernel"], {})
                traffic, tl, tr = ent.get("hbm_bytes_per_launch"), ent.get("launches"), sec_t.get("rounds")
            except (ValueError, OSError):
                traffic = None
        roof["traffic"] = traffic
        roof["traffic_unit"] = "HBM bytes per launch (rocprofv3 PMC passes of `bench.py --section %s`, profiles/hbm_traffic.json)" % section
        roof["traffic_launches_per_round"] = (tl / tr) if (tl and tr) else None
        roof["launches_per_round"] = roof["launches"] / steps
        if traffic:
            roof["traffic_over_algorithmic"] = round(traffic / roof["bytes_per_launch"], 3)
    # untimed split pass for t_encode / t_update
    # (three passes, the median round by update time: one pass alone caught a 1.5 ms outlier step now and then)
    timers = []
    for _ in range(3):
        learner_round(agent, workers, cfg, shared, timers, joint=joint)
    t_enc, t_upd, step_ms = sorted(timers, key=lambda t: t[1])[1]
    # ---- update step against its HBM roof: parameters P read by forward and backward (8P bytes),
    # gradients written (4P), [all-reduce buffer 4P,] clip read (4P), Adam p/g/m/v in + p/m/v out (28P) = 48P bytes,
    # plus the activations of the 8 nets x 8 steps
    P = sum(p.numel() for m in agent.model_dict.values() for p in m.parameters())      # 19 382 808 (arena padding not counted)
    B_gpu = nW * T // MINI_BATCH_NUM
    act_bytes = B_gpu * 8 * SEQ * (530 * 2 + 2120 * 2) * 4
    upd_bytes = 48 * P + act_bytes
    step_ms_s = sorted(step_ms)
    med = step_ms_s[len(step_ms_s) // 2]
    lrn = agent.learner
    n_launch = sum(v for (part, b), v in lrn.launches.items() if b == B_gpu and part == "all") or \
        sum(v for (part, b), v in lrn.launches.items() if b == B_gpu)
    # FLOPs: the reference evaluates all 4 command nets of a head on every row and masks (agent.py:170-182): 3 x 2 x 0.144 G
    # per row (forward + backward).  Rows are sorted by command here and each net runs ITS run of rows only: a quarter of
    # that is executed.  Both roofs are priced on what is executed / moved; the larger time names the bound.
    flops_ref = 3 * 2 * 0.144e9 * B_gpu
    flops_exec = flops_ref / 4
    t_hbm_s, t_mfma_s = upd_bytes / (PEAK_HBM_GBPS * 1e9), flops_exec / (PEAK_F32_MFMA_TFLOPS * 1e12)
    hbm_frac = t_hbm_s / (med * 1e-3)
    mfma_frac = t_mfma_s / (med * 1e-3)
    update_roofline = {
        "bound": "hbm" if t_hbm_s >= t_mfma_s else "mfma",
        "frac": round(max(hbm_frac, mfma_frac), 4),
        "bytes_per_step": upd_bytes, "ms_per_step": round(med, 4), "ms_per_step_min": round(step_ms_s[0], 4),
        "ms_per_step_max": round(step_ms_s[-1], 4), "achieved": round(upd_bytes / (med * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBPS,
        "unit": "GB/s", "hbm_frac": round(hbm_frac, 4),
        "achieved_tflops_executed": round(flops_exec / (med * 1e-3) / 1e12, 2), "peak_tflops": PEAK_F32_MFMA_TFLOPS,
        "mfma_frac": round(mfma_frac, 4), "minibatch_rows": B_gpu,
        "kernels_per_update": n_launch, "kernels_note": "C-ABI launches of update_policy (forward, loss, backward) per "
        "minibatch step; + 3-4 for gather/sort/permute and 3 for clip + Adam; one hipGraph replay each",
        "flops_per_step": round(flops_ref, 1), "flops_per_step_executed": round(flops_exec, 1),
        "note": "one minibatch step = gather + update_policy + gradient exchange + per-model clip + Adam, HIP events in an "
                "untimed pass; bytes = 48 x %d parameters + %d activation bytes (SURVEY.md 8d); flops_per_step = the "
                "reference's command-masked work (every net on every row), flops_per_step_executed = a quarter of it (rows "
                "sorted by command, each net on its own run); hbm_frac = bytes / 8 TB/s, mfma_frac = executed FLOPs / "
                "157.3 TFLOP/s (fp32 matrix pipe), bound = the larger time" % (P, act_bytes)}
    flops_frame = agent.vae_model.flops_per_frame()
    flops_exec = agent.vae_model.flops_per_frame(executed=True)
    nwin = nW * T if joint is not None else T
    enc_bytes = sum(agent.vae_model.algorithmic_bytes(min(cw, nwin - t0) * SEQ) for t0 in range(0, nwin, cw)) * (1 if joint is not None else nW)
    return {
        "t_encode_ms": round(t_enc * 1e3, 3), "t_update_ms": round(t_upd * 1e3, 3),
        "encoder_frames_per_sec": round(frames / t_enc, 1),
        "encoder_tflops": round(frames * flops_frame / t_enc / 1e12, 2),
        "encoder_tflops_executed": round(frames * flops_exec / t_enc / 1e12, 2),
        "encoder_flops_per_round": {"algorithmic_direct_conv": float(frames * flops_frame), "executed": float(frames * flops_exec)},
        "encoder_tflops_note": "encoder_tflops counts DIRECT-convolution FLOPs (the algorithmic work of the layer stack) over "
                               "t_encode; with Winograd convs fewer are executed (encoder_tflops_executed) — the roofline "
                               "object and per_kernel count executed FLOPs only",
        "update_only_samples_per_sec": round(nW * T * PPO_EPOCH / t_upd, 1),
        "encoder_fwd_GBps": round(enc_bytes / t_enc / 1e9, 1) if not dedup else None,
        "encoder_fwd_hbm_frac": round(enc_bytes / t_enc / 1e9 / PEAK_HBM_GBPS, 4) if not dedup else None,
        # north_star asks for >= 0.70 of the HBM roof on the encoder forward.  The layer stack has 149 (fp32) / 298 (bf16)
        # FLOP per algorithmic byte: fp32 is MFMA-bound 7x over (a perfect 157 TFLOP/s kernel moves 0.13 of the roof), bf16
        # sits on the ridge, where 0.70 would need 1.67 PFLOP/s sustained against a MEASURED random-operand MFMA ceiling
        # of 1.78-1.80 PFLOP/s on this chip.  The reachable figure the build tracks instead: the whole bf16
        # encoder at 1.2 PFLOP/s = 0.50 of the roof; fp32 at 0.85 of the fp32 MFMA peak on executed FLOPs = 0.23.
        "encoder_fwd_hbm_frac_target": (0.50 if enc_dtype != "f32" else 0.23) if not dedup else None,
        "encoder_fwd_GBps_note": "algorithmic bytes (SURVEY 8d layer model, weights once per chunk) / t_encode vs HBM peak "
                                 "8000 GB/s; the fp32 conv stack is MFMA-bound (see roofline)",
        "roofline": roof,
        "update_roofline": update_roofline,
    }


def exchange_figures(agent, shared, world, n_ex, sync):
    """--full at N > 1: the gradient exchange of one optimiser step timed alone, and the parameter checksums of every rank."""
    # gradient exchange alone: the collective(s) of one optimiser step on the arena, timed back to back after the run
    import torch.distributed as dist
    g = agent.arena.grads
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    mode = shared.exchange_mode()
    out = {}
    reps = 10
    sync()
    e0.record()
    for _ in range(reps):
        if mode == "sharded":                          # (the collectives chief_step issues in this mode)
            shared.counter.increment()
            shared.reduce_scatter()
            shared.all_gather_params()
        else:
            dist.all_reduce(g, op=dist.ReduceOp.SUM)
    e1.record()
    sync()
    shared.reset(zero=True)
    out["rccl_ranks"] = world
    out["grad_exchange"] = mode + (" in 3 buckets (MLP towers, steer LSTMs, throttle LSTMs), the first two beside the backward"
                                    if shared.overlap_hook(agent.arena) is not None else "")
    out["allreduce_ms_per_step"] = round(e0.elapsed_time(e1) / reps, 4)
    out["allreduce_bytes"] = int(g.numel() * 4)
    out["exchanges_in_timed_region"] = n_ex          # one per optimiser step: 8 per round
    # replicated optimiser: every rank must hold the same parameter bits after the timed rounds.  Checksum = the parameters'
    # bit patterns summed as int64, gathered from every rank (the first multi-GPU box checks C4 without a builder turn)
    cs = agent.arena.params.view(torch.int32).to(torch.int64).sum().reshape(1)
    allcs = [torch.zeros_like(cs) for _ in range(world)]
    dist.all_gather(allcs, cs)
    out["param_checksum_by_rank"] = [int(c.item()) for c in allcs]
    out["params_identical_across_ranks"] = len(set(out["param_checksum_by_rank"])) == 1
    return out


def spawn_ranks(n, timeout_s=None):
    """One process per GPU, started from a parent that never initialises HIP (a process that has touched the GPU must
    not exec or fork GPU work on this pool): children get RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* like
    torch.distributed.run would set them; rank 0's stdout (the JSON line) is relayed, every stderr goes through.
    Every child is polled: when one exits non-zero (OOM, build or ABI mismatch) the others — which would sit in a
    collective forever — are terminated (fresh children of this parent only) and that status is returned; the same
    after `timeout_s` (CADRE_BENCH_SPAWN_TIMEOUT, default 1800 s).  The rendezvous port is chosen by bind-then-close;
    a rendezvous that fails because another process took the port in between is retried once on a new port."""
    import socket
    import subprocess
    import tempfile
    timeout_s = float(os.environ.get("CADRE_BENCH_SPAWN_TIMEOUT", "1800")) if timeout_s is None else timeout_s
    for attempt in range(2):
        sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
        out0 = tempfile.TemporaryFile()
        procs = []
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                          stdout=out0 if r == 0 else subprocess.DEVNULL))
        t_end = time.monotonic() + timeout_s
        rcs = [None] * n
        failed = None
        while any(rc is None for rc in rcs):
            for r, p in enumerate(procs):
                if rcs[r] is None:
                    rcs[r] = p.poll()
                    if rcs[r] not in (None, 0) and failed is None:
                        failed = (r, rcs[r])
            if failed is not None or time.monotonic() > t_end:
                if failed is None:
                    failed = (-1, 124)
                    log("[bench] ranks did not finish within %.0f s: terminating them" % timeout_s)
                for r, p in enumerate(procs):               # the peers of a dead rank wait in a collective for ever
                    if rcs[r] is None:
                        p.terminate()
                for r, p in enumerate(procs):
                    if rcs[r] is None:
                        try:
                            rcs[r] = p.wait(timeout=20)
                        except subprocess.TimeoutExpired:
                            p.kill(); rcs[r] = p.wait()
                break
            time.sleep(0.05)
        out0.seek(0)
        text = out0.read().decode()
        out0.close()
        if failed is not None and attempt == 0 and failed[1] == RC_RENDEZVOUS:
            log("[bench] rendezvous on port %d failed, retrying on a new port" % port)
            continue
        sys.stdout.write(text)
        sys.stdout.flush()
        if failed is not None:
            log("[bench] rank %d failed with status %s (all statuses: %s)" % (failed[0], failed[1], rcs))
            return failed[1] if 0 < failed[1] < 256 else 1
        return 0
    return 1


RC_RENDEZVOUS = 75      # a child's exit status when init_process_group could not bind / connect (EX_TEMPFAIL)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default=None, choices=sorted(CONFIGS),
                    help="headline config (default: C2 PER GPU at every world size, so that value(N) / value(1) compares like "
                         "with like; C3 per GPU — BASELINE C4 at N = 8, the shape the 1 -> 8 target is defined on — rides "
                         "along as the nested \"c3\" section of every line, N = 1 included)")
    ap.add_argument("--chunk-windows", type=int, default=0,
                    help="windows (x8 frames) per encoder launch chain (default: 128, or 256 across the workers of a GPU)")
    ap.add_argument("--no-joint-encode", action="store_true", help="encode each worker's windows separately (chunks of 128)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-peaks", action="store_true", help="skip the measured-peaks microbenchmarks (HBM copy, MFMA chains; ~2 s)")
    ap.add_argument("--no-direct-conv", action="store_true", help="skip the c2_direct_conv section (C2 again with CADRE_WINOGRAD=0; N = 1, C2 headline)")
    ap.add_argument("--no-c3", "--no-nested", dest="no_c3", action="store_true",
                    help="skip the nested section of the line (C3 next to a C2 headline, C2 next to a C3 headline)")
    ap.add_argument("--encoder-dtype", default=None, choices=["f32", "bf16"],
                    help="override the config's encoder arithmetic (C2: f32, C3: bf16 storage / fp32 accumulate)")
    ap.add_argument("--replay", default=None, metavar="DIR",
                    help="replay recorded rollouts (cadre_amd/replay.py .npz episodes) instead of synthetic ones; "
                         "T/H/W come from the records (BASELINE config C5)")
    ap.add_argument("--grad-exchange", default=None, choices=["allreduce", "sharded"],
                    help="N > 1: one all-reduce(SUM) of the gradient arena + replicated clip/Adam (default), or reduce-scatter + "
                         "clip/Adam on the rank's shard + all-gather of the parameters (same wire bytes, 1/N optimiser traffic)")
    ap.add_argument("--grad-buckets", action="store_true",
                    help="N > 1, all-reduce mode: the gradient arena leaves in three buckets, two of them beside the backward "
                         "(opt-in: no multi-GPU RCCL run of this form exists yet; default = ONE blocking all-reduce of the "
                         "80 MB arena per optimiser step)")
    ap.add_argument("--no-grad-buckets", action="store_true", help=argparse.SUPPRESS)    # (round-4 flag: the default again)
    ap.add_argument("--section", default=None, choices=["headline", "c3"],
                    help="ONE section and nothing else (headline = C2, c3 = C3; no nested section, no latent-cache / direct-conv "
                         "rounds, no peaks, no CPU baseline): the command tools/prof_bench.sh runs under rocprofv3, so that "
                         "profiles/ describes exactly the launches of the section's timed region")
    ap.add_argument("--spawn-selftest", action="store_true",
                    help="launcher check (no GPU): every rank prints its RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* and exits")
    ap.add_argument("--c3-steps", type=int, default=10, help="timed rounds of the C3 section (>= 10 by default)")
    ap.add_argument("--no-latent-cache", action="store_true",
                    help="skip the c2_latent_cache / c3_latent_cache sections (the same rounds with each distinct frame encoded once)")
    ap.add_argument("--dedup", action="store_true",
                    help="encode each distinct frame once (sliding-window latent cache) instead of the "
                         "reference's 8 frames per transition; NOT the default metric convention")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: the nested section, the latent-cache / direct-conv / stem-bf16x3 rounds, "
                         "the per-kernel and update rooflines (HIP events around every encoder launch of the timed region, three "
                         "untimed split rounds), the measured peaks, the CPU baseline and, at N > 1, the exchange timing and "
                         "parameter checksums.  Without it a run sets up, warms up, times --steps rounds and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed rounds, write what the last one computed (losses, a fixed sample of the updated "
                         "parameters, encoder features, returns, advantages) as DIR/<name>.npy in float32")
    args = ap.parse_args()
    if not args.full:
        args.no_c3 = args.no_latent_cache = args.no_direct_conv = args.no_peaks = args.no_cpu_baseline = True
    if args.section:
        args.config = "C2" if args.section == "headline" else "C3"
        args.no_c3 = args.no_latent_cache = args.no_direct_conv = args.no_peaks = args.no_cpu_baseline = True

    if args.grad_exchange:
        os.environ["CADRE_GRAD_EXCHANGE"] = args.grad_exchange
    if args.grad_buckets:
        os.environ["CADRE_GRAD_BUCKETS"] = "1"
    if args.no_grad_buckets:
        os.environ["CADRE_GRAD_BUCKETS"] = "0"
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` without a launcher: this process has not touched the GPU (and never will) — it
        # starts N fresh children, one per LOCAL_RANK, relays rank 0's JSON line and exits with their status
        sys.exit(spawn_ranks(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.spawn_selftest:
        line = json.dumps({"rank": rank, "local_rank": local_rank, "world": world, "master": "%s:%s" % (
            os.environ.get("MASTER_ADDR"), os.environ.get("MASTER_PORT")), "gpus": args.gpus})
        log("[bench] selftest " + line)
        fail = os.environ.get("CADRE_BENCH_SELFTEST_FAIL_RANK")       # launcher check: one rank dies, its peers "wait in a collective"
        if fail is not None:
            if rank == int(fail):
                sys.exit(3)
            time.sleep(600)
        if rank == 0:
            print(line, flush=True)
        return
    if args.gpus != world:
        log("[bench] --gpus %d but WORLD_SIZE=%d: running with the launcher's world size" % (args.gpus, world))
    import torch.distributed as dist
    # stdout carries ONE JSON line: RCCL writes its version banner (and warnings) to the C stdout whenever a communicator
    # starts, so fd 1 is pointed at stderr for the duration of the run and restored for the line
    sys.stdout.flush()
    stdout_fd = os.dup(1)
    os.dup2(2, 1)
    # Backend and rank -> device mapping come from the environment so that the WHOLE N > 1 path below (init, startup
    # broadcast, barriers, MAX-reduce, exchange timing, the single line through the self-spawn) can run at world 2 on a
    # ONE-GPU box (tests/test_bench_world2_gpu.py): CADRE_BENCH_BACKEND=gloo (collectives on device tensors through the
    # host), CADRE_BENCH_ONE_DEVICE=1 (every rank on cuda:0).  Defaults: nccl (= RCCL), one GPU per LOCAL_RANK.
    backend = os.environ.get("CADRE_BENCH_BACKEND", "nccl")
    one_device = os.environ.get("CADRE_BENCH_ONE_DEVICE") == "1"
    dev_index = 0 if one_device else local_rank
    torch.cuda.set_device(dev_index)
    use_dist = world > 1 or os.environ.get("CADRE_BENCH_FORCE_DIST") == "1"     # force: exercise RCCL init at N=1
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        try:
            if backend == "nccl":
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev_index))
            else:
                dist.init_process_group(backend, rank=rank, world_size=world)
        except Exception as e:                               # (address in use / connection refused: the parent retries)
            log("[bench] rank %d: init_process_group(%s) failed: %r" % (rank, backend, e))
            sys.exit(RC_RENDEZVOUS)

    # headline: C2 PER GPU at every world size (BASELINE.json's single-GPU fp32 config, weak scaling: one worker x 128
    # steps per GPU) — round 4 switched the headline to C3 for N > 1, which made value(N) / value(1) compare a 4-worker
    # bf16 shape with a 1-worker fp32 one and inflated any efficiency computed from the lines ~4x.  C3 per
    # GPU (BASELINE C4 at N = 8: num_processes = 4 per GPU, bf16 encoder / fp32 losses, the shape north_star's 1 -> 8
    # target is defined on) is the nested "c3" section of EVERY line, with the same fields: its scaling is
    # c3.value(N) / (N * c3.value(1)) from the N = 1 line's c3 section.
    head = args.config or "C2"
    other = {"C2": "C3", "C3": "C2"}.get(head) if args.config is None else None
    res, cfg, enc_state, ppo_state = run_config(head, args, rank, dev_index, world, use_dist, args.steps, args.warmup,
                                                args.replay, section={"C2": "headline", "C3": "c3"}.get(head),
                                                dump_dir=args.dump_outputs)
    out = {"metric": "ppo_update_samples_per_sec", "value": res.pop("value"), "unit": "samples/s", "n_gpus": world,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": res.pop("ms_per_step"), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None}
    res.pop("steps"); res.pop("warmup")
    out.update(res)
    if args.section:
        out["section"] = args.section
    if use_dist:
        out["backend"] = backend if backend != "nccl" else "nccl (RCCL)"
        if one_device:
            out["one_device"] = True
    out["scaling_reference"] = ("value of the N = 1 line (same config, same per-GPU work): efficiency(N) = value(N) / (N x "
                                "value(1)); the nested c3 section scales against the N = 1 line's c3.value")
    # the other BASELINE shape in the same line: next to the C2 headline the C3 section (>= 10 timed rounds)
    if other and not args.no_c3 and not args.replay and not args.dedup and args.encoder_dtype is None:
        n_other = max(2, args.c3_steps) if other == "C3" else args.steps
        sec, _c, _e, _p = run_config(other, args, rank, dev_index, world, use_dist, n_other, 2, section={"C2": "headline", "C3": "c3"}.get(other))
        sec["metric"], sec["unit"], sec["n_gpus"] = "ppo_update_samples_per_sec", "samples/s", world
        out[other.lower()] = sec
    # The round a user of this learner would run: the environment re-sends 7 of the 8 frames of every
    # window (env_wrapper.py:899-904), so with the sliding-window latent cache each distinct frame is encoded ONCE — T + 7
    # frames per worker instead of 8 T, bit-identical features (tests/test_encoder_gpu.py) — and the round is ~70 % update.
    # Own keys; the headline keeps the reference's 8-frames-per-transition convention.
    if not args.no_latent_cache and not args.replay and not args.dedup and args.encoder_dtype is None and args.config is None:
        for nm in ("C2", "C3"):
            if nm != head and args.no_c3:                    # (--no-c3 keeps a run to the headline's shape: no C3 kernels in its trace)
                continue
            sec, _c, _e, _p = run_config(nm, args, rank, dev_index, world, use_dist, max(2, args.c3_steps), 2, dedup=True)
            out[nm.lower() + "_latent_cache"] = {
                "value": sec["value"], "unit": "samples/s", "ms_per_step": sec["ms_per_step"], "steps": sec["steps"], "n_gpus": world,
                "t_encode_ms": sec["t_encode_ms"], "t_update_ms": sec["t_update_ms"],
                "frames_per_round_per_gpu": sec["config"]["frames_per_round_per_gpu"],
                "update_share_of_round": round(sec["t_update_ms"] / (sec["t_encode_ms"] + sec["t_update_ms"]), 3),
                "update_roofline": sec["update_roofline"], "last_losses": sec["last_losses"],
                "ms_per_step_min_median_max": sec["ms_per_step_min_median_max"],
                "note": "%s with the sliding-window latent cache (--dedup): each distinct frame encoded once; NOT the headline "
                        "convention (the reference encodes 8 frames per transition)" % nm}
    # The fp32 model's >= 128-channel stride-1 3x3 convs run as Winograd F(3x3, 3x3) (exact fp32 arithmetic in another
    # order).  The same C2 round with direct convolution everywhere (CADRE_WINOGRAD=0), same box, same
    # process, under its own key — so that the line always states what the algorithm is worth
    if head == "C2" and world == 1 and not args.no_direct_conv and not args.replay and not args.dedup and args.encoder_dtype is None \
            and os.environ.get("CADRE_WINOGRAD", "1") not in ("", "0"):
        os.environ["CADRE_WINOGRAD"] = "0"
        try:
            sec, _c, _e, _p = run_config("C2", args, rank, dev_index, world, use_dist, args.steps, 2)
        finally:
            os.environ.pop("CADRE_WINOGRAD", None)
        out["c2_direct_conv"] = {
            "value": sec["value"], "unit": "samples/s", "ms_per_step": sec["ms_per_step"], "steps": sec["steps"],
            "t_encode_ms": sec["t_encode_ms"], "t_update_ms": sec["t_update_ms"],
            "winograd_vs_direct": round(out["value"] / sec["value"], 4),
            "encoder_tflops": sec["encoder_tflops"], "roofline": sec["roofline"], "last_losses": sec["last_losses"],
            "note": "CADRE_WINOGRAD=0: every convolution direct (implicit GEMM / window kernels)"}
    # The fused front of the fp32 model on the bf16 matrix cores with EXACT products (CADRE_STEM_EXACT_BF16=1: pixel bytes are exact in
    # bf16, every fp32 weight is the exact sum of three bf16 pieces, sums and epilogue fp32 — stem_pool.hip X3).  Its own
    # key, never the headline: VERDICT r5 item 6 keeps the dtype-f32 line on v_mfma_f32.
    if head == "C2" and world == 1 and not args.no_direct_conv and not args.replay and not args.dedup and args.encoder_dtype is None \
            and os.environ.get("CADRE_STEM_EXACT_BF16", "0") != "1" and os.environ.get("CADRE_FUSED_STEM", "1") != "0":
        os.environ["CADRE_STEM_EXACT_BF16"] = "1"
        try:
            sec, _c, _e, _p = run_config("C2", args, rank, dev_index, world, use_dist, args.steps, 2)
        finally:
            os.environ.pop("CADRE_STEM_EXACT_BF16", None)
        out["c2_stem_bf16x3"] = {
            "value": sec["value"], "unit": "samples/s", "ms_per_step": sec["ms_per_step"], "steps": sec["steps"],
            "t_encode_ms": sec["t_encode_ms"], "t_update_ms": sec["t_update_ms"],
            "vs_headline": round(sec["value"] / out["value"], 4), "last_losses": sec["last_losses"],
            "dtype": "f32 everywhere except the 7x7 stem conv: u8 pixels (exact in bf16) x fp32 weights split into 3 bf16 pieces whose "
                     "sum is the fp32 weight exactly, products exact, fp32 accumulate (39 v_mfma_f32_32x32x16_bf16 per tile instead of "
                     "100 v_mfma_f32_32x32x2_f32); rel-max-err of the front vs torch fp32 4.6e-7 - 6.2e-7 (the v_mfma_f32 front: 5.6e-7 - "
                     "8.9e-7), tests/test_kernels_gpu.py::test_fused_stem_pool_exact_bf16_pieces",
            "note": "CADRE_STEM_EXACT_BF16=1; opt-in, not the headline"}
    if rank == 0:
        if not args.no_peaks and world == 1:
            # the datasheet peaks re-measured on this box (stream copy, register-operand MFMA chains): the
            # roofline fractions above use the datasheet figures, `frac_of_measured` restates them against these
            try:
                from tools.peaks_bench import measure
                mp = measure()
                out["measured_peaks"] = mp
                for sect in (out, out.get("c3"), out.get("c2"), out.get("c2_latent_cache"), out.get("c3_latent_cache")):
                    rf = sect.get("roofline") if sect else None
                    if rf and rf.get("bound") == "mfma":
                        pk = mp["mfma_bf16_2wave_TFLOPs"] if rf["peak"] > 1000 else mp["mfma_f32_2wave_TFLOPs"]
                        rf["frac_of_measured"] = round(rf["achieved"] / pk, 4)
                    elif rf:
                        rf["frac_of_measured"] = round(rf["achieved"] / max(mp["hbm_copy_GBps"], mp["hbm_read_GBps"]), 4)
                    ur = sect.get("update_roofline") if sect else None
                    if ur:
                        ur["hbm_frac_of_measured"] = round(ur["achieved"] / max(mp["hbm_copy_GBps"], mp["hbm_read_GBps"]), 4)
                        ur["mfma_frac_of_measured"] = round(ur["achieved_tflops_executed"] / mp["mfma_f32_2wave_TFLOPs"], 4)
            except Exception as e:                           # a diagnostic: never fails the bench line
                log("[bench] measured_peaks skipped: %r" % (e,))
        if not args.no_cpu_baseline and world == 1:          # CPU baseline: rank 0 at N=1 only
            out["cpu_baseline"] = cpu_baseline(cfg, enc_state, ppo_state)
        sys.stdout.flush()
        os.dup2(stdout_fd, 1)
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
