"""Reference statements of the temporal smoothness term (csrc/smooth.hip), each written once:

    pair_valid      the rule that makes (row t, row t + 1) of a storage a pair
    smooth_mates    cadre_smooth_mates: the kinds and the partners of a minibatch's rows (numpy)
    action_jitter   cadre_action_jitter: what a storage's actions did (numpy, float64)
    smooth_pair     the pair statements of cadre_ppo_smooth_loss for the arithmetic classes of tests/loss_parity.py (X64, X32, XVE), with mutants
    smooth_loss_torch the stated term in torch (for autograd)

Plain helper module (no GPU, no fixtures)."""
import numpy as np

from tests import loss_parity as lp

F4, F8 = np.float32, np.float64
# (c_k - mu) -> c_k; the factor 2 dropped; d with the wrong sign on the successor; the mate's mu from the wrong command net; the pair
# counted by both partners
MUTANTS = ("c_not_centred", "no_factor_2", "succ_sign", "mate_wrong_net", "both_count")


def pair_valid(masks, tl, command, t, T, C):
    """masks, tl (or None), command: [T + 1] of one storage."""
    if t < 0 or t > T - 2:
        return False
    if masks[t] == 0:
        return False
    if tl is not None and tl[t] != 0:
        return False
    c = int(command[t])
    return 0 <= c < C and int(command[t + 1]) == c


def smooth_mates(src, idx, nW, E, Bw, T, C, rotation, pos, B):
    """src: 2 nW records (masks, tl or None, command), record 2 w + head; idx int64 [2 (nW + E)][Bw]; pos int32 [2][B] or None.
    -> (row_kind, mate) int32 [2][B] in workspace order."""
    assert B == (nW + E) * Bw
    kind, mate = np.full((2, B), -7, np.int32), np.full((2, B), -7, np.int32)
    P = (lambda h, u: u) if pos is None else (lambda h, u: int(pos[h, u]))
    for h in range(2):
        for w in range(nW):
            k = (w - rotation) % nW
            for r in range(Bw):
                me = P(h, w * Bw + r)
                kind[h, me], mate[h, me] = 0, -1
                if k >= E:
                    continue
                you = P(h, (nW + k) * Bw + r)
                t, t1 = int(idx[2 * w + h][r]), int(idx[2 * (nW + k) + h][r])
                m, tl, cmd = src[2 * w + h]
                ok = pair_valid(m, tl, cmd, t, T, C) and t1 == t + 1
                kind[h, you] = 1
                mate[h, me], mate[h, you] = (you, me) if ok else (-1, -1)
    assert (kind >= 0).all() and (mate >= -1).all()
    return kind, mate


def action_jitter(action, masks, tl, command, T, C, K, ctrl):
    """One storage -> (valid pairs, sum |c[a_{t+1}] - c[a_t]|, max) in float64; the differences are fp32 differences."""
    n, s, mx = 0.0, [], 0.0
    c = np.asarray(ctrl, F4)
    for t in range(T - 1):
        a0, a1 = int(action[t]), int(action[t + 1])
        if not pair_valid(masks, tl, command, t, T, C) or not (0 <= a0 < K and 0 <= a1 < K):
            continue
        d = float(abs(F4(c[a1] - c[a0])))
        n += 1.0
        s.append(d)
        mx = max(mx, d)
    import math
    return n, math.fsum(s), mx


def smooth_pair(X, xb, xmb, ck, cf, succ=False, mut=()):
    """The pair statements on n rows.  xb, xmb [n][K]: the BIN logits (an ordinal head already through lp.ord_logits) of the rows and of
    their mates, typed by X.c; ck [K] typed; cf = smooth_coeff scale_head inv_bp typed.  -> dict(pk, mu, mu_mate, d, gs): gs [n][K] the
    smoothness gradient in bin space, d = mu_own - mu_mate."""
    two = X.c(2.0)
    _lg, pk, _H, _s, _t = lp.front(X, xb, None, ())
    _lgm, pkm, _Hm, _sm, _tm = lp.front(X, xmb, None, ())
    mu = X.sum(pk * ck)
    mu_mate = X.sum(pkm * ck)
    d = mu - mu_mate
    if succ and "succ_sign" in mut:
        d = mu_mate - mu
    gd = cf * d if "no_factor_2" in mut else cf * (two * d)
    centred = ck if "c_not_centred" in mut else ck - mu[..., None]
    gs = gd[..., None] * (pk * centred)
    return dict(pk=pk, mu=mu, mu_mate=mu_mate, d=d, gs=gs)


def smooth_loss_torch(logits_t, logits_t1, ctrl, cf):
    """torch: cf * sum over the rows of (mu(row t) - mu(row t + 1))^2, mu = softmax(logits) . ctrl; both rows differentiated."""
    import torch
    mu = lambda x: (torch.softmax(x, -1) * ctrl).sum(-1)
    d = mu(logits_t) - mu(logits_t1)
    return cf * (d * d).sum()
