"""float64 statement of the exploration-suggestion loss of cadre_ppo_sug_loss in plain torch on the CPU, and the numpy statements
of the mark scan (cadre_suggest_mark) and of the placement of a minibatch's kinds (cadre_suggest_rows): the yardsticks of
tests/test_suggest_cpu.py and tests/test_suggest_gpu.py.

  suggest_loss   the PPO loss of tests/demo_mix_ref.ppo_rows_loss over all rows + sug_coeff inv_b sum over the marked rows of
                 KL(pi || softmax(prior row)), with the four suggestion statistics per head
  mark_scan      the backward scan of include/cadre_hip.h, as written there (`mut` names the scan's one-statement mutants)
  place_kinds    kind[h][pos[h][worker * Bw + b]] = suggest_src[idx]
"""
import numpy as np
import torch

from tests import demo_mix_ref, ordinal_ref

SUG_STATS_FIELDS = 4


def effective_kind(kind, Z):
    """A kind outside 0 .. Z counts as 0."""
    k = np.asarray(kind).astype(np.int64)
    return np.where((k < 1) | (k > Z), 0, k)


def suggest_loss(logits, values, actions, cmds, old_v, rets, old_lp, adv, kind, prior, Z, K, ranks, C, clip, vc, cc, ec, inv_b, sc):
    """logits [2C, B, ld] / values [2C, B] float64 leaves; sample arrays [2][B]; kind int [2][B]; prior float [2][Z + 1][64] RAW
    log-priors.  Returns dict(losses = the three PPO terms, sug_loss, total = losses[0] + losses[1] - losses[2] + sug_loss,
    stats [2][6] of the PPO part, sug_stats [2][4]); total.backward() gives d total / d raw and d total / d value."""
    zero_kind = torch.zeros_like(torch.as_tensor(np.asarray(kind)))
    tv, ta, te, ppo_total, stats = demo_mix_ref.ppo_rows_loss(logits, values, actions, cmds, old_v, rets, old_lp, adv, zero_kind, K,
                                                              ranks, C, clip, vc, cc, ec, inv_b)
    kz = torch.from_numpy(effective_kind(kind, Z))
    pr = torch.as_tensor(np.asarray(prior), dtype=torch.float64)
    sug = torch.zeros((), dtype=torch.float64)
    sstats = torch.zeros(2, SUG_STATS_FIELDS, dtype=torch.float64)
    for hd in range(2):
        c = cmds[hd].long()
        rows = torch.nonzero((kz[hd] != 0) & (c >= 0) & (c < C)).view(-1)
        if rows.numel() == 0:
            continue
        lgn = ordinal_ref.normalised_logits(logits[hd * C + c[rows], rows, :K[hd]], ranks[hd])
        lq = torch.log_softmax(pr[hd, kz[hd][rows], :K[hd]], -1)
        kl = (lgn.exp() * (lgn - lq)).sum(-1)
        sug = sug + kl.sum() * inv_b
        with torch.no_grad():
            mode = lq.argmax(-1)                                   # (argmax: the lowest index among the largest)
            sstats[hd, 0] = rows.numel()
            sstats[hd, 1] = kl.sum() * inv_b
            sstats[hd, 2] = kl.max()
            sstats[hd, 3] = lgn.exp().gather(1, mode.view(-1, 1)).mean()
    sug = sug * sc
    return dict(losses=(tv, ta, te), sug_loss=sug, total=ppo_total + sug, stats=stats, sug_stats=sstats)


def mark_scan(events, masks, time_limits, head, T, Z, horizon, mut=()):
    """events int [>= T], masks float [>= T], time_limits float [>= T] or None, horizon int [2][Z + 1] -> suggest int32 [T]."""
    out = np.zeros(T, np.int32)
    cur = left = 0
    for t in range(T - 1, -1, -1):
        e = int(events[t])
        end = masks[t] == 0 or (time_limits is not None and time_limits[t] != 0)
        is_event = 1 <= e <= Z and horizon[head][e] > 0
        if is_event and "later_event_wins" in mut and left > 0:
            pass                                                   # (mutant: the window of the later event stays open)
        elif is_event:
            cur, left = e, int(horizon[head][e])
            if "window_short" in mut:
                left -= 1
            if "window_long" in mut:
                left += 1
        elif end and "cross_episode" not in mut:
            cur = left = 0
        out[t] = cur if left > 0 else 0
        if left > 0:
            left -= 1
    return out


def place_kinds(suggests, idx, pos, Bt, T, init, mut=()):
    """suggests: per source zi = 2 * worker + head an int array [T] or None; idx int [n_src][Bw]; pos int [2][Bt] or None;
    init int [2][Bt]: what the target holds -> the target after cadre_suggest_rows."""
    out = np.array(init, np.int32, copy=True)
    n_src, Bw = np.shape(idx)
    for zi in range(n_src):
        wi, hd = zi >> 1, zi & 1
        for b in range(Bw):
            ob = wi * Bw + b
            d = ob if (pos is None or "kind_unsorted" in mut) else int(pos[hd][ob])
            if not 0 <= d < Bt:
                continue
            k = 0
            if suggests[zi] is not None:
                t = int(idx[zi][b])
                if not 0 <= t < T:
                    continue
                k = int(suggests[zi][t])
            out[hd, d] = k
    return out
