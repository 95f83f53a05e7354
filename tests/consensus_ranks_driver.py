#!/usr/bin/env python3
"""Rank consensus (train_cfg["rank_consensus"]) with SEVERAL ranks on ONE GPU: each rank is a fresh process on cuda:0,
the process group runs over `gloo` with device tensors (timeout 120 s), and every rank plays the scenarios below and
writes OUT_DIR/rank<r>.npz.  The parent makes no GPU call, waits with a timeout and checks the exit codes:

    python -m tests.consensus_ranks_driver OUT_DIR WORLD

WORLD 1 (the collectives forced, CADRE_BENCH_FORCE_DIST=1) — one learner section (T = 64, 2 minibatches, 4 epochs) with the
KL-adaptive lr, three times: "free" (no gate: its KL sequence places the gate threshold midway before the first step whose
KL exceeds the running maximum, as test_gate_fires_at_step_k does), "kernel" (the gate, decided by the loss kernel) and
"consensus" (the same, with the key).
WORLD 2 — rank r holds ONE worker with storages(64, 2, 21 + r) and the minibatch indices OUT_DIR/config.json fixes, so that
one rank with both workers can replay them (run_multi, called by tests/test_consensus_gpu.py in the test process):
"gate" (target_kl and adaptive lr of the config, with the key), "never" (the key, target_kl 1e9), "plain" (no key, no
target_kl), and "scaling" (three rollouts of T = 16 of one environment through finish_rollouts(consensus=)).

The helpers (run_multi, run_single, scaling_run, ...) are what the test process uses for its one-rank references."""
import datetime
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

T, MBN, EPOCHS = 64, 2, 4
AD = dict(desired_kl=1e3, factor=1.5, min=1e-5, max=1e-2)      # raises lr at every applied step (the cap is out of reach)
LR0 = 3e-4
SC_T, SC_ROLLOUTS, SC_GAMMA, SC_TAU, SC_CLIP = 16, 3, 0.99, 0.95, 10.0
SPAWN_TIMEOUT = 600


def fixed_perms(seed, workers):
    """[worker][epoch][head]: one permutation of range(T) each, from one seeded generator."""
    import torch
    g = torch.Generator().manual_seed(seed)
    return [[[torch.randperm(T, generator=g).tolist() for _h in range(2)] for _e in range(EPOCHS)] for _w in range(workers)]


def pin_indices(pair, perms):
    """Replace the sampler of a (steer, throttle) storage pair by the fixed permutations perms[epoch][head]."""
    import torch
    for h, s in enumerate(pair):
        def sample(s=s, it=iter([p[h] for p in perms])):
            perm = torch.tensor(next(it), dtype=torch.int64)
            bs = s.num_steps // s.mini_batch_num
            return [perm[i:i + bs] for i in range(0, s.num_steps, bs)]
        s.sample_indices = sample


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def snapshot(agent, st, losses):
    """Everything the tests compare, small: digests of the big buffers (bit identity), per-model parameter sums, the rows."""
    import numpy as np
    import torch
    torch.cuda.synchronize()
    a, lrn = agent.arena, agent.learner
    names = a.model_names()
    rows = st["rows"]
    d = dict(params=digest(a.params), exp_avg=digest(a.exp_avg), exp_avg_sq=digest(a.exp_avg_sq),
             step_dev=int(a.step_dev.item()), step=int(a.step),
             stop=-1 if lrn._stop is None else int(lrn._stop.item()),
             lr_bits=0 if lrn._hp is None else int(lrn._hp[:1].view(torch.int64).item()),
             param_sums=np.array([float(sum(t.double().sum() for t in a.views(a.params, n).values())) for n in names]),
             losses=np.array(losses, dtype=np.float64),
             applied=np.array([r["applied"] for r in rows]), row_lr=np.array([r.get("lr", 0.0) for r in rows], dtype=np.float64),
             approx_kl=np.array([r["approx_kl"] for r in rows], dtype=np.float64),
             has_global=all("global_approx_kl" in r for r in rows),
             global_approx_kl=np.array([r.get("global_approx_kl", (np.nan, np.nan)) for r in rows], dtype=np.float64),
             stopped_at_step=-1 if st["stopped_at_step"] is None else int(st["stopped_at_step"]),
             updates_applied=int(st["updates_applied"]), consensus_world=int(st.get("consensus_world", 0)))
    return d


def _cfg(**kw):
    d = dict(use_adv_norm=True, ppo_epoch=EPOCHS, max_grad_norm=250.0, lr=LR0)
    d.update(kw)
    return d


def run_multi(seeds, perms, extra):
    """One learner_section_multi of a fresh agent over len(seeds) workers (worker i: storages(T, MBN, seeds[i]) with the
    fixed indices perms[i]); extra = train_cfg keys.  Uses the process group that is up, if any."""
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section_multi
    from tests.test_learner_gpu import make_agent
    from tests.test_ppo_stats_gpu import storages
    agent = make_agent(84, 84)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    rollouts = [storages(T, MBN, s) for s in seeds]
    for pair, p in zip(rollouts, perms):
        pin_indices(pair, p)
    st = {}
    losses = learner_section_multi(agent, rollouts, [False] * len(seeds), _cfg(**extra), shared, stats=st)
    return snapshot(agent, st, losses)


def run_single(extra, seed=9):
    """One learner_section (the construction of test_gate_fires_at_step_k: storages(64, 2, 21), global generator seeded
    with 9) of a fresh agent; also the state of the CPU generator afterwards."""
    import torch
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section
    from tests.test_learner_gpu import make_agent
    from tests.test_ppo_stats_gpu import storages
    agent = make_agent(84, 84)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    pair = storages(T, MBN, 21)
    torch.manual_seed(seed)
    st = {}
    losses = learner_section(agent, pair[0], pair[1], False, _cfg(**extra), shared, stats=st)
    d = snapshot(agent, st, losses)
    d["rng"] = digest(torch.get_rng_state())
    return d


def first_exceeding(kl):
    """(k, threshold target_kl, gap): k = the first step whose KL exceeds the running maximum (0-based, >= 1), target_kl
    such that 1.5 target_kl lies midway between that maximum and kl[k]; k = None when there is no such step."""
    k = next((j for j in range(1, len(kl)) if kl[j] > max(kl[:j])), None)
    if k is None:
        return None, None, None
    return k, (max(kl[:k]) + kl[k]) / 2 / 1.5, kl[k] - max(kl[:k])


# ----------------------------------------------------------------------------- reward scaling
def scaling_data(env, head, rollout):
    import torch
    g = torch.Generator().manual_seed(7000 + 100 * rollout + 10 * env + head)
    return dict(rewards=torch.rand(SC_T + 1, 1, generator=g) * 3.0 - 0.5, value_preds=torch.randn(SC_T + 1, 1, generator=g) * 0.3,
                masks=(torch.rand(SC_T + 1, 1, generator=g) >= 0.15).float())


def scaling_next_value(env, head):
    return 0.05 * (2 * env + head + 1)


def scaling_run(envs, shared=None):
    """SC_ROLLOUTS rollouts of the environments `envs` (two storages each) through finish_rollouts with one ReturnScaler;
    shared: the Shared_grad_buffers for consensus, or None.  Returns per rollout the scale bits and the returns."""
    import numpy as np
    import torch
    from cadre_amd import hip
    from ppo_agent.storage import ReturnScaler, RolloutStorage
    st = []
    for _ in range(2 * len(envs)):
        s = RolloutStorage(SC_T, 2, 32, 1, 32, True, SC_GAMMA, SC_TAU)
        s.to("cuda:0")
        st.append(s)
    rs = ReturnScaler(len(envs), SC_GAMMA, clip=SC_CLIP, device="cuda:0")
    scales, returns, stats = [], [], []
    for ro in range(SC_ROLLOUTS):
        for i, e in enumerate(envs):
            for h in (0, 1):
                for k, v in scaling_data(e, h, ro).items():
                    getattr(st[2 * i + h], k).copy_(v)
        nv = [scaling_next_value(e, h) for e in envs for h in (0, 1)]
        RolloutStorage.finish_rollouts(st, nv, normalise=False, reward_scaler=rs, consensus=shared)
        torch.cuda.synchronize()
        state = rs.state.cpu().numpy()
        scales.append(state[hip.RS_SCALE:hip.RS_CARRY].copy())
        stats.append(state[:6].copy())
        returns.append(np.stack([s.returns[:SC_T, 0].cpu().numpy() for s in st]))
    return dict(scales=np.array(scales), returns=np.array(returns), stats=np.array(stats))


def light_shared():
    """A Shared_grad_buffers over a small CPU arena: all that all_reduce_small needs."""
    import torch
    from cadre_amd.arena import PPOArena
    from ppo_agent.models import Model, Shared_grad_buffers, _no_orthogonal_init
    arena = PPOArena("cpu", 530, {"steer": 33, "throttle": 3}, 4)
    with _no_orthogonal_init():
        md = {"steer_ppo_0": arena.bind("steer_ppo_0", Model(530, 33))}
    return Shared_grad_buffers(md, torch.device("cpu"))


# ----------------------------------------------------------------------------- ranks
def _flat(out, name, d):
    for k, v in d.items():
        out["%s/%s" % (name, k)] = v


def rank_main(out_dir):
    import numpy as np
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    os.environ["CADRE_GRAD_EXCHANGE"] = "allreduce"
    os.environ["CADRE_GRAD_BUCKETS"] = "0"
    if world == 1:
        os.environ["CADRE_BENCH_FORCE_DIST"] = "1"           # still run the collectives
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    out = {}
    try:
        if world == 1:
            free = run_single(dict(adaptive_lr=AD))
            k, tkl, gap = first_exceeding([float(max(r)) for r in free["approx_kl"]])
            _flat(out, "free", free)
            out["k"], out["tkl"], out["gap"] = (-1 if k is None else k), (0.0 if k is None else tkl), (0.0 if k is None else gap)
            if k is not None:
                _flat(out, "kernel", run_single(dict(adaptive_lr=AD, target_kl=tkl)))
                _flat(out, "consensus", run_single(dict(adaptive_lr=AD, target_kl=tkl, rank_consensus=True)))
        else:
            with open(os.path.join(out_dir, "config.json")) as f:
                conf = json.load(f)
            seeds, perms = [21 + rank], [conf["perms"][rank]]
            _flat(out, "gate", run_multi(seeds, perms, dict(adaptive_lr=AD, target_kl=conf["target_kl"], rank_consensus=True)))
            _flat(out, "never", run_multi(seeds, perms, dict(target_kl=1e9, rank_consensus=True)))
            _flat(out, "plain", run_multi(seeds, perms, dict()))
            _flat(out, "scaling", scaling_run([rank], light_shared()))
        torch.cuda.synchronize()
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    finally:
        dist.destroy_process_group()
    return 0


def main(out_dir, world):
    if "RANK" in os.environ:
        return rank_main(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, "-m", "tests.consensus_ranks_driver", out_dir, str(world)], cwd=ROOT, env=env))
    rcs, deadline = [], time.monotonic() + SPAWN_TIMEOUT
    try:
        for p in procs:
            rcs.append(p.wait(timeout=max(1.0, deadline - time.monotonic())))
    except subprocess.TimeoutExpired:
        rcs.append("timeout")
    finally:
        for p in procs:                                          # (a rank that outlived the wait, or its failed peer)
            if p.poll() is None:
                p.kill()
                p.wait()
    print("CONSENSUS_RESULT " + json.dumps(dict(exitcodes=rcs, world=world)), flush=True)
    return 0 if rcs == [0] * world else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], int(sys.argv[2])))
