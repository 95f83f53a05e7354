"""numpy float64 references for the ensemble-evaluation kernels (csrc/ensemble.hip) and the stacked-arena indexing, written
independently of cadre_amd.ppo_agent.evaluate: plain loops over the definitions."""
import numpy as np


def controls(actions, steer_tab, throttle_tab):
    """cadre_ensemble_controls: actions int [N][M][2] -> float64 [N][3].  Each column summed sequentially in float64 in
    agent order, divided by float64(M); with M > 1 a brake < 0.5 becomes 0; a bin outside its table: three NaN."""
    actions = np.asarray(actions, dtype=np.int64)
    N, M = actions.shape[:2]
    steer_tab = np.asarray(steer_tab, dtype=np.float64).reshape(-1)
    throttle_tab = np.asarray(throttle_tab, dtype=np.float64).reshape(-1, 2)
    out = np.empty((N, 3), dtype=np.float64)
    for e in range(N):
        acc = [np.float64(0.0), np.float64(0.0), np.float64(0.0)]
        bad = False
        for m in range(M):
            a0, a1 = int(actions[e, m, 0]), int(actions[e, m, 1])
            if not (0 <= a0 < len(steer_tab) and 0 <= a1 < len(throttle_tab)):
                bad = True
                continue
            acc[0] = acc[0] + steer_tab[a0]
            acc[1] = acc[1] + throttle_tab[a1, 0]
            acc[2] = acc[2] + throttle_tab[a1, 1]
        acc = [v / np.float64(M) for v in acc]
        if M > 1 and acc[2] < 0.5:
            acc[2] = np.float64(0.0)
        out[e] = [np.nan] * 3 if bad else acc
    return out


def ordinal_logits(x, rank):
    """csrc/ordinal.h in float64: x [K] threshold units in rank space -> unnormalised bin logits [K]."""
    x = np.asarray(x, dtype=np.float64)
    eps = np.float64(np.float32(1e-8))
    u = np.log(1.0 / (1.0 + np.exp(-x)) + eps)
    w = np.log(1.0 / (1.0 + np.exp(x)) + eps)
    z = np.array([u[:r + 1].sum() + w[r + 1:].sum() for r in range(len(x))])
    return z[np.asarray(rank, dtype=np.int64)]


def greedy(logits, rank=None):
    """cadre_sample_rows_ens with q == NULL for one row: (first index of the largest probability, its log-prob), float64."""
    x = np.asarray(logits, dtype=np.float64)
    if rank is not None:
        x = ordinal_logits(x, rank)
    lg = x - (x.max() + np.log(np.exp(x - x.max()).sum()))
    k = int(np.argmax(lg))                               # numpy: the first maximum
    return k, float(lg[k])


def net_index(h, j, c, Mg, C):
    """Arena net of group agent j's (head h, command c): heads outermost, then the agents, then the commands."""
    n = 0
    for hh in range(2):
        for jj in range(Mg):
            for cc in range(C):
                if (hh, jj, cc) == (h, j, c):
                    return n
                n += 1
    raise ValueError((h, j, c, Mg, C))


def tiled_seg(commands, C, Mg):
    """Brute force: the (first row, count) run of every stacked net when the rows are sorted by command (stable)."""
    order = sorted(range(len(commands)), key=lambda e: commands[e])
    sorted_cmd = [commands[e] for e in order]
    out = np.zeros((2 * Mg * C, 2), dtype=np.int32)
    for h in range(2):
        for j in range(Mg):
            for c in range(C):
                rows = [r for r, cc in enumerate(sorted_cmd) if cc == c]
                first = rows[0] if rows else sum(1 for cc in sorted_cmd if cc < c)
                out[net_index(h, j, c, Mg, C)] = (first, len(rows))
    return out


def group_split(M, C):
    per, out = 16 // C, []
    while M > 0:
        out.append(min(per, M))
        M -= out[-1]
    return out
