"""Latency of the cost constraint (cadre_amd/constraint.py): begin_section + mix (two critic launches, the bootstrap, the cost scan,
the multiplier, the mix) and one critic step (per head forward with the activations kept -> backward, then one Adam step over both
towers) at N T = 128, 1024 and 4096 rows of D = 530 features, beside the same chain written with torch ops on the device (in this tool
only: the product never runs it); and a whole learner_section_multi at N = 8 environments with and without the module, in the same
process.

Each form is timed with HIP events around --reps back-to-back calls, --runs runs per form after a warm-up, the forms alternating; the
median is reported with min and max.  The torch chain runs the towers with torch.addmm / relu, the scan as a Python loop over T on
[2N] vectors (what a library user would write) and the step with autograd and torch.optim.Adam.

    python tools/constraint_bench.py [--runs 20] [--reps 10] [--out profiles/constraint_latency.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((4, 32), (8, 128), (16, 256))           # (N, T): 128, 1024, 4096 rows
D, S = 530, 3


class TorchChain:
    """The module's chain as library calls on the device."""

    def __init__(self, con, storages):
        o, P = con.offsets, con.P
        self.flat = con.params.clone().requires_grad_(True)
        cut = lambda p: [p[o[0]:o[1]].view(con.D, con.H), p[o[1]:o[2]], p[o[2]:o[3]].view(con.H, con.H), p[o[3]:o[4]],
                         p[o[4]:o[5]].view(con.H, 1), p[o[5]:]]
        self.w = [cut(self.flat[h * P:(h + 1) * P]) for h in (0, 1)]
        self.opt = torch.optim.Adam([self.flat], lr=1e-3)
        self.st = storages
        self.T = storages[0][0].num_steps
        self.lam = torch.tensor([0.5, 0.5], dtype=torch.float64, device="cuda")
        self.ret = None

    def rows(self, h, upto):
        return torch.cat([p[h].obs[:upto, S - 1] for p in self.st])

    @staticmethod
    def net(x, w):
        h = torch.relu(torch.addmm(w[1], x, w[0]))
        h = torch.relu(torch.addmm(w[3], h, w[2]))
        return torch.addmm(w[5], h, w[4])[:, 0]

    def begin_section_and_mix(self):
        T, N = self.T, len(self.st)
        with torch.no_grad():
            V = torch.stack([self.net(self.rows(h, T + 1), self.w[h]).view(N, T + 1) for h in (0, 1)])       # [2][N][T + 1]
        c = torch.stack([torch.stack([p[h].costs for p in self.st]) for h in (0, 1)])
        m = torch.stack([torch.stack([p[h].masks[:, 0] for p in self.st]) for h in (0, 1)])
        gae = torch.zeros(2, N, device="cuda")
        ret = torch.zeros(2, N, T, device="cuda")
        for t in range(T - 1, -1, -1):
            delta = c[:, :, t] + 0.99 * V[:, :, t + 1] * m[:, :, t] - V[:, :, t]
            gae = delta + 0.99 * 0.95 * m[:, :, t] * gae
            ret[:, :, t] = gae + V[:, :, t]
        adv_c = ret - V[:, :, :T]
        J = c[:, :, :T].double().mean((1, 2))
        self.lam = torch.clamp(self.lam + 0.05 * (J - 0.1), 0.0, 100.0)
        lf = self.lam.float().view(2, 1, 1)
        cen = adv_c - adv_c.double().mean(2, keepdim=True).float()
        for w, p in enumerate(self.st):
            for h in (0, 1):
                p[h].advantages[:, 0] = (p[h].advantages[:, 0] - lf[h, 0, 0] * cen[h, w]) / (1.0 + lf[h, 0, 0])
        self.ret = ret
        return V

    def step(self):
        loss = 0.0
        for h in (0, 1):
            v = self.net(self.rows(h, self.T), self.w[h])
            loss = loss + 0.5 * ((v - self.ret[h].reshape(-1)) ** 2).mean()
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def fmt(name, h, t, other="torch ops"):
    return ("  %-52s HIP %8.3f ms  (min %.3f max %.3f)   %s %8.3f ms  (min %.3f max %.3f)   ratio %.2f"
            % (name, statistics.median(h), min(h), max(h), other, statistics.median(t), min(t), max(t),
               statistics.median(t) / statistics.median(h)))


def chain_sizes(args, lines):
    from cadre_amd.constraint import CostConstraint
    from cadre_amd.ppo_agent.storage import RolloutStorage
    for N, T in SIZES:
        g = torch.Generator()
        g.manual_seed(N)
        st = []
        for _w in range(N):
            pair = tuple(RolloutStorage(T, 1, D, S, 128, True, 0.99, 0.95, device="cuda") for _h in range(2))
            x = torch.randn(T + 1, S, D, generator=g).cuda()
            for s in pair:
                s.obs.copy_(x)
                s.masks.copy_((torch.rand(T + 1, 1, generator=g) >= 0.05).float())
                s.costs = torch.rand(T + 1, generator=g).cuda()
                s.advantages.copy_(torch.randn(T, 1, generator=g))
                s.step = T
            st.append(pair)
        con = CostConstraint(D, N, budget=0.1, lambda_init=0.5, epochs=1, minibatches=1, device="cuda")
        ref = TorchChain(con, st)
        R = N * T

        def section():
            con.begin_section(st, None)
            con.mix(st)
        section()
        V = ref.begin_section_and_mix()
        agree = float((con.cost_values[:, :, :T] - V[:, :, :T]).abs().max())
        calls = [("hip", "section", section), ("torch", "section", ref.begin_section_and_mix), ("hip", "step", lambda: con.step(0, R)),
                 ("torch", "step", ref.step)]
        for _ in range(args.warmup):
            for _a, _b, fn in calls:
                fn()
        torch.cuda.synchronize()
        ts = {(a, b): [] for a, b, _ in calls}
        for _ in range(args.runs):
            for a, b, fn in calls:
                ts[(a, b)].append(timed(fn, args.reps))
        lines.append("N T = %d rows (N = %d, T = %d; the cost values of the two chains differ by at most %.1e)" % (R, N, T, agree))
        lines.append(fmt("begin_section + mix (6 launches)", ts[("hip", "section")], ts[("torch", "section")]))
        lines.append(fmt("one critic step (2 x (forward + 5) + 3 kernels)", ts[("hip", "step")], ts[("torch", "step")]))


def whole_section(args, lines, N=8, T=64):
    """learner_section_multi on synthetic storages of the production geometry, with and without constraint=, alternating."""
    from cadre_amd import synth
    from cadre_amd.constraint import CostConstraint
    from cadre_amd.ppo_agent.agent import CadreAgent
    from cadre_amd.ppo_agent.models import Shared_grad_buffers
    from cadre_amd.ppo_agent.storage import RolloutStorage
    from cadre_amd.ppo_agent.train import learner_section_multi

    class AD(dict):
        __getattr__ = dict.__getitem__
        __setattr__ = dict.__setitem__
    H = W = 84
    fh, fw = synth.feat_hw(H, W)
    model_cfg = AD(use_lstm=True, vae_device=0, device_num=0, vae_params="CoPM", measurement_dim=18, num_output=AD(steer=33, throttle=3),
                   command_num=4, obs_hw=(H, W), weights_init="none", vae_state_dict=synth.encoder_state(fh, fw, 7), latent_cache=True)
    agent = CadreAgent(rank=0, model_cfg=model_cfg, frame=8, STEER_CONTROL={i: (i - 16) / 16.0 for i in range(33)},
                       THROTTLE_CONTROL={0: [0, 0], 1: [0, 1], 2: [0.6, 0]}, ent_coeff=0.01, value_coeff=0.1, clip_coeff=1.0, clip=0.1)
    agent.arena.load_numpy_state(synth.ppo_state(11))
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    g = torch.Generator()
    g.manual_seed(5)
    rollouts = []
    for _w in range(N):
        pair = []
        for K in (33, 3):
            s = RolloutStorage(T, 2, 530, 8, 530, True, 0.99, 0.95, device="cuda")
            s.obs.copy_(torch.randn(T + 1, 8, 530, generator=g))
            s.action.copy_(torch.randint(0, K, (T + 1, 1), generator=g))
            s.action_log_probs.copy_(-torch.rand(T + 1, 1, generator=g) * 2.0)
            s.value_preds.copy_(torch.randn(T + 1, 1, generator=g) * 0.3)
            s.rewards.copy_(torch.randn(T + 1, 1, generator=g))
            s.masks.copy_((torch.rand(T + 1, 1, generator=g) >= 0.05).float())
            s.command.copy_(torch.randint(0, 4, (T + 1, 1), generator=g).int())
            s.costs = torch.rand(T + 1, generator=g).cuda()
            s.step = T
            pair.append(s)
        rollouts.append(tuple(pair))
    con = CostConstraint(agent, N, budget=0.1, lambda_init=0.5)
    cfg = dict(use_adv_norm=True, ppo_epoch=4, max_grad_norm=250.0, lr=1e-6)
    dones = [False] * N

    def run(c):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        learner_section_multi(agent, rollouts, dones, cfg, shared, losses_on_device=True, **({} if c is None else dict(constraint=c)))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(args.warmup):
        run(None)
        run(con)
    ts = {"off": [], "on": []}
    for _ in range(args.runs):
        ts["off"].append(run(None))
        ts["on"].append(run(con))
    lines.append("learner_section_multi, N = %d environments, T = %d, ppo_epoch 4 x 2 minibatches; the module with its defaults (hidden 128, 4 x 4 "
                 "critic steps)" % (N, T))
    lines.append(fmt("whole section with constraint= (HIP) vs without", ts["on"], ts["off"], other="without  "))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("constraint_bench needs an MI355X: a time taken elsewhere says nothing")
    lines = ["Cost constraint latency (%s; D = %d, hidden 128; median of %d runs x %d back-to-back calls per form, forms alternating, HIP "
             "events; call-to-call time, launch overhead included)" % (torch.cuda.get_device_name(0), D, args.runs, args.reps)]
    chain_sizes(args, lines)
    whole_section(args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
