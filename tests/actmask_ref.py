"""float64 statement of action masks (csrc/actmask.h, csrc/actmask.hip) in numpy: the yardstick of tests/test_actmask_cpu.py and
tests/test_actmask_gpu.py.

A row of a head carries one 64-bit word; bit k set means bin k may be chosen.  The mask acts in BIN space, behind the ordinal transform
where the head is ordinal: with x the logit of bin k, x = allowed(k) ? x : -inf, and everything behind it runs over the allowed bins only.
A word with no bit among the head's K bins means "unmasked".  In the loss the taken action is allowed by definition (its bit is OR-ed in
after the empty-means-all rule); the sampler picks argmax(p / q) over the allowed bins, the lowest index on ties.

  words / bits         uint64 handling: the K low bits, empty means all, the bool matrix [n][K]
  bin_logits           raw tower outputs -> bin logits (identity, or the ordinal transform of ordinal.h in the statements of
                       tests/loss_parity.ord_logits)
  masked_log_softmax   normalised logits (-inf on forbidden bins), probabilities, entropy, log-sum-exp
  sample               argmax(p / q) over allowed bins with the relative top-2 margin
  loss                 cadre_ppo_am_loss: losses, gradients in closed form, PPO stats, mask stats
  note / place_words   cadre_allowed_note / cadre_allowed_rows

The statements of `loss` are those of tests/loss_parity.ppo_row in its order: with every bit set the selects pick their first operand
everywhere and the result equals tests/loss_parity.run_loss(case, X64()) bit for bit (tests/test_actmask_cpu.py)."""
import numpy as np

F8 = np.float64
ORD_EPS = F8(np.float32(1e-8))
AM_STATS_FIELDS = 4


# ----------------------------------------------------------------------------- words
def all_word(K):
    return (1 << K) - 1


def to_u64(words):
    """int64 storage (or Python ints up to 2^64 - 1) -> uint64 array."""
    w = np.asarray(words)
    if w.dtype == np.int64:
        return w.view(np.uint64)
    return np.array([int(v) & (2 ** 64 - 1) for v in np.reshape(w, -1)], dtype=np.uint64).reshape(np.shape(w))


def to_i64(words):
    """uint64 / Python ints -> the int64 bit patterns the tensors hold."""
    return to_u64(words).view(np.int64)


def effective(words, K, actions=None):
    """The bits of the K bins, empty means all; with `actions` the taken action's bit OR-ed in -> (uint64 words, forced bool)."""
    w = to_u64(words)
    allw = np.uint64(all_word(K))
    m = w & allw
    m = np.where(m == 0, allw, m)
    forced = np.zeros(m.shape, bool)
    if actions is not None:
        a = np.asarray(actions).astype(np.int64)
        ok = (a >= 0) & (a < K)
        bit = np.left_shift(np.uint64(1), np.clip(a, 0, 63).astype(np.uint64))
        forced = ok & ((m & bit) == 0)
        m = np.where(forced, m | bit, m)
    return m, forced


def bits(m, K):
    """uint64 [n] -> bool [n][K]."""
    k = np.arange(K, dtype=np.uint64)
    return ((np.asarray(m, np.uint64)[..., None] >> k) & np.uint64(1)) != 0


def popcount(m):
    return bits(m, 64).sum(-1)


# ----------------------------------------------------------------------------- the head
def bin_logits(x, rank=None):
    """x float64 [n][K] raw -> (bin logits, s, t); s = t = None for a categorical head."""
    x = np.asarray(x, F8)
    if rank is None:
        return x, None, None
    with np.errstate(over="ignore", under="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
        t = 1.0 / (1.0 + np.exp(x))
    u, w = np.log(s + ORD_EPS), np.log(t + ORD_EPS)
    wl = np.concatenate([w[..., 1:], np.zeros_like(w[..., :1])], -1)
    z = np.cumsum(u, -1) + np.cumsum(wl[..., ::-1], -1)[..., ::-1]
    return np.take_along_axis(z, np.broadcast_to(np.asarray(rank, np.int64), z.shape), -1), s, t


def ord_backward(g, s, t, rank):
    binv = np.argsort(np.asarray(rank, np.int64))
    G = np.take_along_axis(g, np.broadcast_to(binv, g.shape), -1)
    pre = np.concatenate([np.zeros_like(G[..., :1]), np.cumsum(G, -1)[..., :-1]], -1)
    suf = np.cumsum(G[..., ::-1], -1)[..., ::-1]
    st = s * t
    return st / (s + ORD_EPS) * suf - st / (t + ORD_EPS) * pre


def masked_log_softmax(xb, on):
    """xb [n][K] bin logits, on bool [n][K] (at least one bin per row) -> (lg, pk, H, lse): lg = -inf and pk = 0 on forbidden bins."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        x = np.where(on, xb, -np.inf)
        mx = x.max(-1)
        se = np.where(on, np.exp(x - mx[..., None]), 0.0).sum(-1)
        lse = mx + np.log(se)
        lg = x - lse[..., None]
        mx2 = lg.max(-1)
        e2 = np.where(on, np.exp(lg - mx2[..., None]), 0.0)
        se2 = e2.sum(-1)
        pk = e2 / se2[..., None]
        H = -np.where(on, pk * lg, 0.0).sum(-1)
    return lg, pk, H, lse


def pressure(xb, lse_m, proper):
    """1 - exp(lse_masked - lse_unmasked) per row; exactly 0 where the mask is not proper."""
    mx = xb.max(-1)
    lse = mx + np.log(np.exp(xb - mx[..., None]).sum(-1))
    return np.where(proper, np.clip(1.0 - np.exp(lse_m - lse), 0.0, 1.0), 0.0)


def sample(raw, q, words, K, rank=None):
    """raw [n][>= K], q [n][>= K], words [n] -> (action, masked logp of it, relative margin between the best and the second-best p / q
    among the allowed bins; inf with one allowed bin).  The lowest index wins ties."""
    xb, _s, _t = bin_logits(np.asarray(raw, F8)[:, :K], rank)
    m, _ = effective(words, K)
    on = bits(m, K)
    lg, _pk, _H, _lse = masked_log_softmax(xb, on)
    with np.errstate(over="ignore", under="ignore"):
        p = np.where(on, np.exp(lg), 0.0)
        p = p / p.sum(-1, keepdims=True)
        score = np.where(on, p / np.asarray(q, F8)[:, :K], -np.inf)
    top = np.sort(score, -1)[:, ::-1]
    act = (score == top[:, :1]).argmax(-1)
    if K < 2:
        margin = np.full(act.shape, np.inf)
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            margin = np.where(np.isfinite(top[:, 1]), (top[:, 0] - top[:, 1]) / top[:, 0], np.inf)
    return act, lg[np.arange(lg.shape[0]), act], margin


def evaluate(raw, actions, words, K, rank=None):
    """cadre_categorical_eval_am: (masked logp of the given actions, masked entropy)."""
    xb, _s, _t = bin_logits(np.asarray(raw, F8)[:, :K], rank)
    m, _ = effective(words, K, actions)
    lg, _pk, H, _lse = masked_log_softmax(xb, bits(m, K))
    return lg[np.arange(lg.shape[0]), np.asarray(actions)], H


# ----------------------------------------------------------------------------- the loss
def loss(logits, values, actions, cmds, old_v, rets, old_lp, adv, allowed, K, ranks, C, clip, vc, cc, ec, inv_b):
    """logits [2C][B][ld] / values [2C][B]; sample arrays [2][B]; allowed [2][B] words; K = (K_steer, K_throttle); ranks = per head a
    rank list or None; the scalars as float64 numbers.  Returns dict(losses [3], total, dlogits [2C][B][ld], dvalues [2C][B] (zeros where
    the kernel writes zeros), stats [2][6], am_stats [2][4], logp / entropy / ratio [2][B] (NaN on rows whose command is out of range))."""
    logits, values = np.asarray(logits, F8), np.asarray(values, F8)
    B = logits.shape[1]
    clip, vc, cc, ec, inv_b = (F8(v) for v in (clip, vc, cc, ec, inv_b))
    dl, dv = np.zeros_like(logits), np.zeros_like(values)
    names = ("val", "act", "ent", "kl", "okl", "cf", "vcf", "r", "alr", "proper", "nbins", "press", "forced")
    tp = {k: np.zeros((2, B)) for k in names}
    logp, ent, rat = (np.full((2, B), np.nan) for _ in range(3))
    for h in range(2):
        Kh = K[h]
        c = np.asarray(cmds[h]).astype(np.int64)
        rows = np.flatnonzero((c >= 0) & (c < C))
        if rows.size == 0:
            continue
        net = h * C + c[rows]
        a = np.asarray(actions[h]).astype(np.int64)[rows]
        xb, s, t = bin_logits(logits[net, rows, :Kh], ranks[h])
        m, forced = effective(np.asarray(allowed)[h][rows], Kh, a)
        on = bits(m, Kh)
        lg, pk, H, lse = masked_log_softmax(xb, on)
        v = values[net, rows]
        ov, R, olp, A = (np.asarray(t_[h], F8)[rows] for t_ in (old_v, rets, old_lp, adv))
        lp = lg[np.arange(rows.size), a]
        lr = lp - olp
        ratio = np.exp(lr)
        s1 = ratio * A
        lo, hi = 1.0 - clip, 1.0 + clip
        rc = np.minimum(np.maximum(ratio, lo), hi)
        s2 = rc * A
        dvv = v - ov
        dvc = np.minimum(np.maximum(dvv, -clip), clip)
        vpc = ov + dvc
        d1, d2 = v - R, vpc - R
        vl, vlc = d1 * d1, d2 * d2
        terms = dict(act=-np.minimum(s1, s2), val=np.maximum(vl, vlc), ent=H, kl=(ratio - 1.0) - lr, okl=-lr,
                     cf=np.where(np.abs(ratio - 1.0) > clip, 1.0, 0.0), vcf=np.where(np.abs(dvv) > clip, 1.0, 0.0), r=ratio,
                     alr=np.abs(lr))
        proper = m != np.uint64(all_word(Kh))
        terms.update(proper=proper.astype(F8), nbins=popcount(m).astype(F8), press=pressure(xb, lse, proper), forced=forced.astype(F8))
        for k_, t_ in terms.items():
            tp[k_][h, rows] = t_
        logp[h, rows], ent[h, rows], rat[h, rows] = lp, H, ratio
        # backward (ties split 0.5 / 0.5 as torch.min / torch.max do)
        in_ratio = (ratio >= lo) & (ratio <= hi)
        tie = 0.5 * A + np.where(in_ratio, 0.5 * A, 0.0)
        dmin = np.where(s1 < s2, A, np.where(s1 > s2, np.where(in_ratio, A, 0.0), tie))
        dlp = cc * inv_b * (-dmin) * ratio
        in_v = (dvv >= -clip) & (dvv <= clip)
        g1, g2 = 2.0 * d1, np.where(in_v, 2.0 * d2, 0.0)
        dmax = np.where(vl > vlc, g1, np.where(vl < vlc, g2, 0.5 * g1 + 0.5 * g2))
        dv[net, rows] = vc * inv_b * 0.5 * dmax
        dH = -ec * inv_b
        hit = np.where(np.arange(Kh)[None, :] == a[:, None], 1.0, 0.0)
        with np.errstate(invalid="ignore"):
            et = -pk * (lg + H[..., None])
            gk = np.where(on, dlp[..., None] * (hit - pk) + dH * et, 0.0)
        if ranks[h] is not None:
            gk = ord_backward(gk, s, t, ranks[h])
        dl[net[:, None], rows[:, None], np.arange(Kh)[None, :]] = gk
    losses = [vc * 0.5 * tp["val"].sum() * inv_b, cc * tp["act"].sum() * inv_b, ec * tp["ent"].sum() * inv_b]
    stats = np.stack([tp[k].sum(-1) * inv_b for k in ("kl", "okl", "cf", "vcf", "r")] + [tp["alr"].max(-1)], 1)
    cnt = np.array([max(1, int(((np.asarray(cmds[h]) >= 0) & (np.asarray(cmds[h]) < C)).sum())) for h in range(2)], F8)
    am = np.stack([tp["proper"].sum(-1) / cnt, tp["nbins"].sum(-1) / cnt, tp["press"].sum(-1) / cnt, tp["forced"].sum(-1)], 1)
    return dict(losses=losses, total=losses[0] + losses[1] - losses[2], dlogits=dl, dvalues=dv, stats=stats, am_stats=am, logp=logp,
                entropy=ent, ratio=rat)


# ----------------------------------------------------------------------------- recording and the words of a minibatch
def note(tensors, slots, words, T):
    """tensors: per storage an int64 array [T + 1] or None (changed in place); allowed[k][slots[k]] = words[k] for 0 <= slot <= T."""
    for k, al in enumerate(tensors):
        s = int(slots[k])
        if al is not None and 0 <= s <= T:
            al[s] = to_i64([words[k]])[0]


def place_words(srcs, idx, pos, Bt, T, init):
    """srcs: per source zi = 2 * worker + head an int64 array [>= T] or None; idx int [n_src][Bw]; pos int [2][Bt] or None; init int64
    [2][Bt]: what the target holds -> the target after cadre_allowed_rows (a source without words gives 0)."""
    out = np.array(init, np.int64, copy=True)
    n_src, Bw = np.shape(idx)
    for zi in range(n_src):
        wi, hd = zi >> 1, zi & 1
        for b in range(Bw):
            ob = wi * Bw + b
            if ob >= Bt:
                continue
            d = ob if pos is None else int(pos[hd][ob])
            if not 0 <= d < Bt:
                continue
            w = 0
            if srcs[zi] is not None:
                t = int(idx[zi][b])
                if not 0 <= t < T:
                    continue
                w = int(srcs[zi][t])
            out[hd, d] = w
    return out
