"""Cost of rank consensus (train_cfg["rank_consensus"]) on the minibatch step, over RCCL at forced world size 1.

One GPU per box: the `nccl` backend is initialised with one rank and CADRE_BENCH_FORCE_DIST=1, so every collective is
really issued (the set-up of tests/rccl_world1_driver.py).  NO run on two or more GPUs exists; what this measures is what
the extra small collective and the decision kernel cost on the host and the device, not what a network adds.

One step = update_policy_from_storages (gather + the update's hipGraph) + add_gradient + chief_step (the all-reduce of the
gradient arena, then clip + Adam), as learner_section runs it, at B = 64 and B = 256 (one worker, 4 command nets, 84x84
agent), with the KL gate armed (a target_kl it never reaches) and the KL-adaptive lr on.  Modes on the same agent and
storages, interleaved over --rounds rounds, median per-step time reported (wall clock around --iters steps, ending in a
device synchronise: the consensus path adds host work between two graph replays):
  kernel     the loss kernel decides (no key: the same commit without the feature's path)
  consensus  the key: the 16-byte all-reduce of the step's KL pair + cadre_kl_consensus between the gradient exchange and
             the optimiser step

    python tools/consensus_overhead.py [--iters 200] [--rounds 5] [--out profiles/consensus_overhead.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = ("kernel", "consensus")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch.distributed as dist
    from ppo_agent.chief import chief_step
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.storage import RolloutStorage
    from tests.helpers import fill_storages
    from tests.test_learner_gpu import make_agent

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29537")
    os.environ["CADRE_BENCH_FORCE_DIST"] = "1"          # world_size 1: still issue the RCCL collectives
    os.environ["CADRE_GRAD_EXCHANGE"] = "allreduce"
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        lines = ["PPO update step: rank consensus over RCCL %s at forced world size 1 (%s, median of %d rounds x %d steps)"
                 % (".".join(str(v) for v in torch.cuda.nccl.version()), torch.cuda.get_device_name(0), args.rounds, args.iters)]
        for B in (64, 256):
            agent = make_agent(84, 84)
            shared = Shared_grad_buffers(agent.model_dict, agent.device)
            assert shared.dist_world() == 1
            T = 2 * B
            data = fill_storages(T, 3)
            pair = []
            for hd in ("steer", "throttle"):
                s = RolloutStorage(T, 2, 530, 8, 530, True, 0.99, 0.95)
                for k, v in data[hd].items():
                    getattr(s, k).copy_(torch.from_numpy(v))
                s.to("cuda:0")
                s.compute_returns(torch.tensor([0.1]))
                pair.append(s)
            lrn = agent.learner
            rows = torch.zeros(max(args.warmup, args.iters), 2, lrn.stats_fields(), device="cuda:0")
            idx = [torch.randperm(T)[:B] for _ in range(8)]

            def run(mode, n):
                cons = mode == "consensus"
                lrn.set_adaptive_lr(1e-2, lr_min=1e-5, lr_max=1e-3, lr=3e-4, consensus=cons)
                lrn.set_update_modes(stats=True, target_kl=1e9, consensus=cons)
                for i in range(n):
                    agent.update_policy_from_storages(
                        [(pair[0], idx[i % 8], pair[0].advantages, pair[1], idx[(i + 4) % 8], pair[1].advantages)],
                        sync=False, stats_row=rows[i])
                    shared.add_gradient(agent.model_dict)
                    chief_step(shared, None, 250.0, lr=3e-4, zero_grads=False)
                lrn.set_update_modes()
                lrn.set_adaptive_lr(None)

            for mode in MODES:
                run(mode, args.warmup)
            torch.cuda.synchronize()
            res = {m: [] for m in MODES}
            for _ in range(args.rounds):
                for mode in MODES:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(mode, args.iters)
                    torch.cuda.synchronize()
                    res[mode].append(1e3 * (time.perf_counter() - t0) / args.iters)
            med = {m: float(np.median(v)) for m, v in res.items()}
            spread = 100.0 * (max(res["kernel"]) - min(res["kernel"])) / med["kernel"]
            for mode, v in res.items():
                lines.append("B=%-4d %-10s %.4f ms/step  (%+.2f %% vs kernel)   rounds: %s"
                             % (B, mode, med[mode], 100.0 * (med[mode] / med["kernel"] - 1.0), " ".join("%.4f" % x for x in v)))
            lines.append("B=%-4d consensus - kernel: %+.1f us/step; round-to-round spread of kernel: %.2f %% (max - min over median)"
                         % (B, 1e3 * (med["consensus"] - med["kernel"]), spread))
    finally:
        dist.destroy_process_group()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
