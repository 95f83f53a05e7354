"""float64 statements of the PPG auxiliary phase in plain torch on the CPU: the yardstick of tests/test_phasic_cpu.py and
tests/test_phasic_gpu.py.

  record     the normalised log-probabilities cadre_aux_record writes (categorical and ordinal heads, through
             tests/ordinal_ref.normalised_logits), -inf in columns >= K
  aux_loss   aux_value_coeff 0.5 mean (v - R)^2 + beta_clone mean KL(pi_old || pi) as float64 autograd, with the six statistics
             per head of cadre_aux_loss
"""
import torch

from tests import ordinal_ref

AUX_STATS_FIELDS = 6


def _rows(cmds, row_id, pos, hd, C, R):
    """(unsorted rows u that count for head hd, their workspace positions b, commands c, table rows r)."""
    B = cmds.shape[1]
    u = torch.arange(B)
    b = u if pos is None else pos[hd].long()
    inb = (b >= 0) & (b < B)
    c = torch.full((B,), -1, dtype=torch.int64)
    c[inb] = cmds[hd].long()[b[inb]]
    r = row_id[hd].long()
    ok = inb & (c >= 0) & (c < C) & (r >= 0) & (r < R)
    keep = torch.nonzero(ok).view(-1)
    return keep, b[keep], c[keep], r[keep]


def record(logits, cmds, row_id, pos, K, ranks, C, table):
    """logits [2C, B, ld] float64; cmds [2][B] in workspace order; row_id i64 [2][B] per UNSORTED row; pos [2][B] (the
    workspace position of each unsorted row) or None; table float64 [2][R][64], changed in place and returned: the rows
    addressed get the normalised log-probabilities, -inf in columns >= K."""
    R = table.shape[1]
    for hd in range(2):
        _u, b, c, r = _rows(cmds, row_id, pos, hd, C, R)
        if b.numel() == 0:
            continue
        lgn = ordinal_ref.normalised_logits(logits[hd * C + c, b, :K[hd]].detach(), ranks[hd])
        table[hd, r] = float("-inf")
        table[hd, r, :K[hd]] = lgn
    return table


def aux_loss(logits, values, cmds, rets, table, row_id, pos, K, ranks, C, beta, vc, inv_b):
    """logits [2C, B, ld] / values [2C, B] float64 leaves; cmds, rets [2][B] in workspace order; table [2][R][64] (normalised
    log-probabilities; anything in columns >= K); row_id, pos as in record.  A row counts for a head when its position, its
    command and its row_id are in range.  Returns (value term, KL term, total, stats float64 [2][6]) with the coefficients
    applied; total.backward() gives d total / d raw and d total / d value.  p_old is the softmax of the stored row."""
    tot_v = tot_k = 0
    stats = torch.zeros(2, AUX_STATS_FIELDS, dtype=torch.float64)
    R_rows = table.shape[1]
    for hd in range(2):
        _u, b, c, r = _rows(cmds, row_id, pos, hd, C, R_rows)
        if b.numel() == 0:
            continue
        lgn = ordinal_ref.normalised_logits(logits[hd * C + c, b, :K[hd]], ranks[hd])
        v = values[hd * C + c, b]
        lo = table[hd, r, :K[hd]].double()
        po = torch.softmax(lo, -1)
        # (0 * -inf never occurs: a bin of old probability 0 is skipped, as the kernel does)
        kl = torch.where(po != 0, po * (lo - lgn), torch.zeros_like(lgn)).sum(-1)
        Rt = rets[hd].double()[b]
        tot_v = tot_v + (v - Rt).pow(2).sum() * inv_b
        tot_k = tot_k + kl.sum() * inv_b
        with torch.no_grad():
            stats[hd, 0] = kl.sum() * inv_b
            stats[hd, 1] = kl.max()
            stats[hd, 2] = (v - Rt).abs().sum() * inv_b
            stats[hd, 3] = ordinal_ref.entropy(lgn).sum() * inv_b
            stats[hd, 4] = (v - Rt).pow(2).sum() * inv_b
            stats[hd, 5] = b.numel() * inv_b
    tot_v = 0.5 * tot_v * vc
    tot_k = tot_k * beta
    return tot_v, tot_k, tot_v + tot_k, stats
