"""Latency of Curiosity.begin_section (statistics -> forward -> reward) and of one predictor step (forward with the activations kept ->
backward -> Adam) at N T = 128, 1024 and 4096 rows of D = 530 features, beside the same chain written with torch ops on the device (in
this tool only: the product never runs it).

Each form is timed with HIP events around --reps back-to-back calls, --runs runs per form after a warm-up, the forms alternating; the
median is reported with min and max.  The torch chain keeps its statistics in float64 like the module, runs the towers with
torch.addmm / relu and the step with autograd and torch.optim.Adam.

    python tools/curiosity_bench.py [--runs 20] [--reps 10] [--out profiles/curiosity_latency.txt]
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

    def __init__(self, cur, storages):
        from cadre_amd.curiosity import tower_offsets
        o, _P = tower_offsets(cur.D, cur.H, cur.E)
        cut = lambda p: [p[o[0]:o[1]].view(cur.D, cur.H), p[o[1]:o[2]], p[o[2]:o[3]].view(cur.H, cur.H), p[o[3]:o[4]],
                         p[o[4]:o[5]].view(cur.H, cur.E), p[o[5]:]]
        self.f = cut(cur.target.clone())
        self.flat = cur.predictor.clone().requires_grad_(True)
        self.g = cut(self.flat)
        self.opt = torch.optim.Adam([self.flat], lr=1e-4)
        self.st = storages
        self.T = storages[0][0].num_steps
        self.n = torch.zeros((), dtype=torch.float64, device="cuda")
        self.mu = torch.zeros(cur.D, dtype=torch.float64, device="cuda")
        self.M2 = torch.zeros(cur.D, dtype=torch.float64, device="cuda")
        self.carry = torch.zeros(len(storages), dtype=torch.float64, device="cuda")
        self.rho = [torch.zeros((), dtype=torch.float64, device="cuda") for _ in range(3)]
        self.gamma, self.E = 0.99, cur.E

    def rows(self):
        return torch.cat([p[0].obs[:self.T, S - 1] for p in self.st])

    @staticmethod
    def net(x, w):
        h = torch.relu(torch.addmm(w[1], x, w[0]))
        h = torch.relu(torch.addmm(w[3], h, w[2]))
        return torch.addmm(w[5], h, w[4])

    def normalised(self, x):
        return torch.clamp((x - self.mu.float()) / torch.sqrt(self.M2 / self.n + 1e-8).float(), -5.0, 5.0)

    def begin_section(self):
        x = self.rows()
        xd = x.double()
        nb = float(x.shape[0])
        mean = xd.mean(0)
        q = ((xd - mean) ** 2).sum(0)
        tot = self.n + nb
        delta = mean - self.mu
        self.mu, self.M2, self.n = self.mu + delta * nb / tot, self.M2 + q + delta * delta * self.n * nb / tot, tot
        with torch.no_grad():
            xh = self.normalised(x)
            err = ((self.net(xh, self.g) - self.net(xh, self.f)) ** 2).mean(1).view(-1, self.T)
        e = err.double()
        # rho_t = gamma rho_{t-1} + e_t as one cumulative sum of e_t / gamma^t (float64; T <= 256 keeps gamma^-t below 14)
        pw = self.gamma ** torch.arange(1, self.T + 1, dtype=torch.float64, device="cuda")
        rho = (self.carry.view(-1, 1) + torch.cumsum(e / pw, 1)) * pw
        self.carry = rho[:, -1]
        cnt, mu, m2 = self.rho
        nb = float(rho.numel())
        d = rho.mean() - mu
        self.rho = [cnt + nb, mu + d * nb / (cnt + nb), m2 + ((rho - rho.mean()) ** 2).sum() + d * d * cnt * nb / (cnt + nb)]
        sigma = torch.sqrt(self.rho[2] / self.rho[0] + 1e-8).float()
        ri = (err / sigma).repeat_interleave(2, 0)
        for k, s in enumerate(s for p in self.st for s in p):
            s.rewards_mixed[:self.T, 0] = s.rewards[:self.T, 0] + 0.5 * ri[k]
        return err

    def step(self):
        x = self.rows()
        xh = self.normalised(x)
        err = ((self.net(xh, self.g) - self.net(xh, self.f).detach()) ** 2).mean(1)
        m = (torch.rand(err.shape, device="cuda") < 0.25).float()
        loss = (m * err).sum() / torch.clamp(m.sum(), min=1.0)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("curiosity_bench needs an MI355X: a time taken elsewhere says nothing")
    from cadre_amd.curiosity import Curiosity
    from cadre_amd.ppo_agent.storage import RolloutStorage
    lines = ["Curiosity latency (%s; D = %d, hidden 128, embed 64; median of %d runs x %d back-to-back calls per form, forms alternating, HIP "
             "events; call-to-call time, launch overhead included)" % (torch.cuda.get_device_name(0), D, args.runs, args.reps)]
    for N, T in SIZES:
        g = torch.Generator()
        g.manual_seed(N)
        st = []
        for _w in range(N):
            pair = tuple(RolloutStorage(T, 1, D, S, 128, True, 0.99, 0.95, device="cuda") for _h in range(2))
            x = torch.randn(T + 1, S, D, generator=g).cuda()
            for s in pair:
                s.obs.copy_(x)
                s.rewards.copy_(torch.randn(T + 1, 1, generator=g))
                s.step = T
            st.append(pair)
        cur = Curiosity(D, N, coeff=0.5, epochs=1, minibatches=1, device="cuda")
        ref = TorchChain(cur, st)
        err = cur.begin_section(st)
        other = ref.begin_section()
        agree = float(((err - other).abs() / other).max())
        R = N * T

        def one_step():
            cur._forward(0, R, cur._workspace(R)["err"], save=True)
            cur.backward(R)
            cur.adam()
        calls = [("hip", "begin_section", lambda: cur.begin_section(st)), ("torch", "begin_section", ref.begin_section),
                 ("hip", "step", one_step), ("torch", "step", ref.step)]
        for _ in range(args.warmup):
            for _a, _b, fn in calls:
                fn()
        torch.cuda.synchronize()
        ts = {(a, b): [] for a, b, _ in calls}
        for _ in range(args.runs):
            for a, b, fn in calls:
                ts[(a, b)].append(timed(fn, args.reps))
        lines.append("N T = %d rows (N = %d, T = %d; err of the two chains on the first rollout differs by at most %.1e relative)" % (R, N, T, agree))
        for key, name in (("begin_section", "begin_section (3 launches: 4 kernels)"), ("step", "one predictor step (forward + 6 + 3 kernels)")):
            h, t = ts[("hip", key)], ts[("torch", key)]
            lines.append("  %-46s HIP %8.3f ms  (min %.3f max %.3f)   torch ops %8.3f ms  (min %.3f max %.3f)   ratio %.2f"
                         % (name, statistics.median(h), min(h), max(h), statistics.median(t), min(t), max(t),
                            statistics.median(t) / statistics.median(h)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
