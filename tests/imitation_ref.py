"""float64 / strict-fp32 statements of the behaviour-cloning path, in plain torch and numpy on the CPU: the yardstick of
tests/test_imitation_cpu.py and tests/test_imitation_gpu.py.

  bc_loss          the imitation loss of cadre_bc_loss as float64 autograd (categorical and ordinal heads, through
                   tests/ordinal_ref.normalised_logits) with its six statistics per head
  mc_returns       the discounted Monte-Carlo return as the numpy loop of the strict fp32 scan (oracle/ppo_ref.gae_returns
                   with V = 0, tau = 1, written out)
  balance_weights  w = T / (C_present * count[command])
  window_rows      obs[t][s] = latent[window[t][s]] | measurements x 6 | zeros
"""
import numpy as np
import torch

from tests import ordinal_ref

BC_STATS_FIELDS = 6


def smoothed_target(a, K, eps):
    """t_k = (1 - eps) [k = a] + eps / K, float64 [len(a)][K]."""
    a = torch.as_tensor(a, dtype=torch.int64).view(-1)
    t = torch.full((a.numel(), K), float(eps) / K, dtype=torch.float64)
    t[torch.arange(a.numel()), a] += 1.0 - float(eps)
    return t


def bc_loss(logits, values, actions, cmds, rets, weights, K, ranks, C, eps, bc, vc, ec, inv_b):
    """logits [2C, B, ld] / values [2C, B] float64 leaves; actions i64 [2][B], cmds [2][B], rets [2][B], weights [2][B] or
    None; K = (K_steer, K_throttle); ranks = (steer, throttle) rank lists or None (categorical).  A row counts for a head
    when its command is in 0 .. C-1 and its action in 0 .. K-1.  Returns (value term, bc term, entropy term, total,
    stats float64 [2][6]) with the coefficients applied; total.backward() gives d total / d raw and d total / d value."""
    tot_v = tot_b = tot_e = 0
    stats = torch.zeros(2, BC_STATS_FIELDS, dtype=torch.float64)
    B = actions.shape[1]
    for hd in range(2):
        a, c = actions[hd].long(), cmds[hd].long()
        ok = (c >= 0) & (c < C) & (a >= 0) & (a < K[hd])
        rows = torch.nonzero(ok).view(-1)
        if rows.numel() == 0:
            continue
        own = logits[hd * C + c[rows], rows, :K[hd]]
        v = values[hd * C + c[rows], rows]
        lgn = ordinal_ref.normalised_logits(own, ranks[hd])
        p = lgn.exp()
        t = smoothed_target(a[rows], K[hd], eps)
        # (0 * -inf never occurs: a zero target is skipped, as the kernel does)
        ce = -torch.where(t != 0, t * lgn, torch.zeros_like(lgn)).sum(-1)
        H = -(p * lgn).sum(-1)
        R = rets[hd].double()[rows]
        w = torch.ones(rows.numel(), dtype=torch.float64) if weights is None else weights[hd].double()[rows]
        tot_v = tot_v + (w * (v - R).pow(2)).sum() * inv_b
        tot_b = tot_b + (w * ce).sum() * inv_b
        tot_e = tot_e + (w * H).sum() * inv_b
        with torch.no_grad():
            top = (p == p.max(-1, keepdim=True).values).double().argmax(-1)       # the lowest index among the largest
            stats[hd, 0] = (top == a[rows]).double().sum() * inv_b
            stats[hd, 1] = -lgn.gather(1, a[rows].view(-1, 1)).sum() * inv_b
            stats[hd, 2] = H.sum() * inv_b
            stats[hd, 3] = (v - R).abs().sum() * inv_b
            stats[hd, 4] = w.sum() * inv_b
            stats[hd, 5] = rows.numel() * inv_b
    tot_v = 0.5 * tot_v * vc
    tot_b = tot_b * bc
    tot_e = tot_e * ec
    return tot_v, tot_b, tot_e, tot_v + tot_b - tot_e, stats


def mc_returns(rewards, masks, gamma):
    """G_t = r_t + gamma m_t G_{t+1} over float32 [T] arrays, G_T = 0: every product and sum rounded to fp32 separately, in
    the order of the rollout-finishing scan with V = 0 and tau = 1 (gae = (r + 0) - 0 + (gamma m) gae)."""
    f = np.float32
    r, m = np.asarray(rewards, f), np.asarray(masks, f)
    g32 = f(gamma)
    out = np.zeros(r.shape[0], f)
    g = f(0.0)
    for t in range(r.shape[0] - 1, -1, -1):
        u1 = f(g32 * m[t])
        u2 = f(u1 * g)
        g = f(r[t] + u2)
        out[t] = g
    return out


def balance_weights(commands):
    cmd = np.asarray(commands, np.int64)
    present = sorted(set(cmd.tolist()))
    count = {c: int((cmd == c).sum()) for c in present}
    return np.array([cmd.size / (len(present) * count[int(c)]) for c in cmd], np.float64)


def window_rows(latent, window, meas, ldo):
    """latent f32 [n][512], window int [T][S], meas f64 [n][3] -> f32 [T][S][ldo]."""
    T, S = window.shape
    out = np.zeros((T, S, ldo), np.float32)
    out[:, :, :512] = latent[window]
    out[:, :, 512:530] = np.tile(meas[window].astype(np.float32), (1, 1, 6))
    return out
