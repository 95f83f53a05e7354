"""float64 statement of the ordinal policy head (Tang & Agrawal; the commented-out block of the reference's
ppo_agent/distributions.py:45-79) in plain torch on the CPU: forward, and autograd for the backward.  The yardstick of
tests/test_ordinal_cpu.py and tests/test_ordinal_gpu.py — written with the reference's mask matrix, not with the scans
the kernels and the module-level torch tail use.

Per head with K bins: rank[k] = position of bin k in ascending order of its control value; column j of the raw tower
output x is threshold unit j in rank space.  With eps = 1e-8:
    s = sigmoid(x)   t = sigmoid(-x)   u = log(s + eps)   w = log(t + eps)
    z_r = sum_{j <= r} u_j + sum_{j > r} w_j          (mask1: a[i, j] = 1 iff i >= j)
    logit of bin k = z[rank[k]]
then the categorical head on these logits, in bin space."""
import torch

EPS = 1e-8


def mask1(K, dtype=torch.float64):
    i = torch.arange(K)
    return (i.view(-1, 1) >= i.view(1, -1)).to(dtype)


def ordinal_logits(x, rank):
    """x [..., K] float64 raw threshold units -> unnormalised bin logits [..., K]."""
    x = x.double()
    u = torch.log(torch.sigmoid(x) + EPS)
    w = torch.log(torch.sigmoid(-x) + EPS)
    a = mask1(x.shape[-1])
    z = u @ a.t() + w @ (1.0 - a).t()
    return z[..., torch.as_tensor(rank, dtype=torch.int64)]


def normalised_logits(x, rank=None):
    """Normalised bin logits of a head: ordinal when `rank` is a permutation, the plain categorical head when None."""
    lg = x.double() if rank is None else ordinal_logits(x, rank)
    return lg - lg.logsumexp(-1, keepdim=True)


def entropy(lgn):
    return -(lgn.exp() * lgn).sum(-1)


def top2_margin(score):
    """(argmax with the lowest index winning ties, relative margin (top1 - top2) / top1) per row of a positive score."""
    top = score.topk(min(2, score.shape[-1]), dim=-1).values
    idx = (score == top[..., :1]).double().argmax(-1)
    if score.shape[-1] < 2:
        return idx, torch.full(idx.shape, float("inf"), dtype=torch.float64)
    return idx, (top[..., 0] - top[..., 1]) / top[..., 0]


def sample(lgn, q):
    """The sampling rule argmax(p / q), q[k] belonging to bin k -> (index, relative top-2 margin of p / q)."""
    return top2_margin(lgn.exp() / q.double())


def ppo_loss(logits, values, actions, cmds, old_v, rets, old_lp, adv, K, ranks, C, clip, vc, cc, ec):
    """The PPO loss of agent.py:166-229 with the heads of `ranks` ((steer, throttle), each a rank list or None), float64.
    logits [2C, B, ld] / values [2C, B] are leaves that require grad.  Returns (value term, action term, entropy term,
    total) with the coefficients applied; total.backward() gives d total / d raw."""
    tot_v = tot_a = tot_e = 0
    for hd in range(2):
        cur_v = cur_lp = ent = 0
        for c in range(C):
            lgn = normalised_logits(logits[hd * C + c, :, :K[hd]], ranks[hd])
            lp = lgn.gather(1, actions[hd].view(-1, 1))
            e = entropy(lgn).view(-1, 1)
            msk = (cmds[hd] == c).view(-1, 1)
            cur_v = cur_v + values[hd * C + c].view(-1, 1) * msk
            cur_lp = cur_lp + lp * msk
            ent = ent + e * msk
        ratio = torch.exp(cur_lp - old_lp[hd].view(-1, 1))
        A = adv[hd].view(-1, 1)
        tot_a = tot_a - torch.min(ratio * A, torch.clamp(ratio, 1 - clip, 1 + clip) * A).mean()
        ov, R = old_v[hd].view(-1, 1), rets[hd].view(-1, 1)
        vpc = ov + (cur_v - ov).clamp(-clip, clip)
        tot_v = tot_v + 0.5 * torch.max((cur_v - R).pow(2), (vpc - R).pow(2)).mean()
        tot_e = tot_e + ent.mean()
    return tot_v * vc, tot_a * cc, tot_e * ec, tot_v * vc + tot_a * cc - tot_e * ec
