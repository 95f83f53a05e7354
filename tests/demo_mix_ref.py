"""float64 statement of the mixed loss of cadre_ppo_demo_loss (PPO rows + demonstration rows in one minibatch), in plain
torch on the CPU: the yardstick of tests/test_demo_mix_cpu.py and tests/test_demo_mix_gpu.py.

  ppo_rows_loss   the PPO loss of agent.py:166-229 row by row over the PPO rows of each head (kind 0, command in range), with
                  the sums scaled by inv_b and the six update diagnostics of cadre_ppo_loss_stats; on a minibatch of PPO
                  rows only, with inv_b = 1 / B, it is tests/ordinal_ref.ppo_loss
  mixed_loss      ppo_rows_loss + the demonstration terms of tests/imitation_ref.bc_loss (ec = 0) on the demonstration rows,
                  weights from the `adv` slot, means with inv_bd
Both go through tests/ordinal_ref.normalised_logits for ordinal heads.
"""
import torch

from tests import imitation_ref, ordinal_ref

PPO_NSTAT = 6


def ppo_rows_loss(logits, values, actions, cmds, old_v, rets, old_lp, adv, kind, K, ranks, C, clip, vc, cc, ec, inv_b):
    """logits [2C, B, ld] / values [2C, B] float64 leaves; sample arrays [2][B]; kind [2][B] (0: a PPO row).  Returns
    (value term, action term, entropy term, total, stats float64 [2][6]) with the coefficients applied."""
    tot_v = tot_a = tot_e = 0
    stats = torch.zeros(2, PPO_NSTAT, dtype=torch.float64)
    for hd in range(2):
        c = cmds[hd].long()
        rows = torch.nonzero((kind[hd] == 0) & (c >= 0) & (c < C)).view(-1)
        if rows.numel() == 0:
            continue
        lgn = ordinal_ref.normalised_logits(logits[hd * C + c[rows], rows, :K[hd]], ranks[hd])
        lp = lgn.gather(1, actions[hd][rows].long().view(-1, 1)).view(-1)
        H = ordinal_ref.entropy(lgn)
        v = values[hd * C + c[rows], rows]
        A, ov, R = adv[hd].double()[rows], old_v[hd].double()[rows], rets[hd].double()[rows]
        log_r = lp - old_lp[hd].double()[rows]
        ratio = torch.exp(log_r)
        tot_a = tot_a - torch.min(ratio * A, torch.clamp(ratio, 1 - clip, 1 + clip) * A).sum() * inv_b
        vpc = ov + (v - ov).clamp(-clip, clip)
        tot_v = tot_v + 0.5 * torch.max((v - R).pow(2), (vpc - R).pow(2)).sum() * inv_b
        tot_e = tot_e + H.sum() * inv_b
        with torch.no_grad():
            stats[hd, 0] = ((ratio - 1) - log_r).sum() * inv_b
            stats[hd, 1] = (-log_r).sum() * inv_b
            stats[hd, 2] = ((ratio - 1).abs() > clip).double().sum() * inv_b
            stats[hd, 3] = ((v - ov).abs() > clip).double().sum() * inv_b
            stats[hd, 4] = ratio.sum() * inv_b
            stats[hd, 5] = log_r.abs().max()
    return tot_v * vc, tot_a * cc, tot_e * ec, tot_v * vc + tot_a * cc - tot_e * ec, stats


def demo_commands(cmds, kind):
    """The commands with every PPO row marked out of range (-1): what hands only the demonstration rows to bc_loss."""
    out = cmds.clone()
    out[kind == 0] = -1
    return out


def mixed_loss(logits, values, actions, cmds, old_v, rets, old_lp, adv, kind, K, ranks, C, clip, vc, cc, ec, inv_b, eps, dc,
               dvc, inv_bd):
    """Returns dict(losses = (value, action, entropy) of the PPO rows, demo_losses = (cross-entropy, value) of the
    demonstration rows, total = losses[0] + losses[1] - losses[2] + demo_losses[0] + demo_losses[1], stats [2][6] of the PPO
    rows, demo_stats [2][6] of the demonstration rows); total.backward() gives d total / d raw and d total / d value."""
    tv, ta, te, ppo_total, stats = ppo_rows_loss(logits, values, actions, cmds, old_v, rets, old_lp, adv, kind, K, ranks, C,
                                                 clip, vc, cc, ec, inv_b)
    dv, db, _de, demo_total, demo_stats = imitation_ref.bc_loss(logits, values, actions, demo_commands(cmds, kind), rets, adv, K,
                                                                ranks, C, eps, dc, dvc, 0.0, inv_bd)
    return dict(losses=(tv, ta, te), demo_losses=(db, dv), total=ppo_total + demo_total, stats=stats, demo_stats=demo_stats)
