"""Reference statements of self-imitation learning (csrc/selfimit.hip), each written once:

    sil_row       the SIL row of cadre_ppo_sil_loss for the arithmetic classes of tests/loss_parity.py (X64, X32, XVE), with mutants
    sil_loss_torch the stated loss in torch (for autograd)
    closed_scan   the realised return, the closed / eligible flags (numpy, strict fp32: the statements of cadre_gae_multi with tau = 1, V = 0)
    quantise      the priority of a weight, float64
    draw          the prioritised draw: cumsum + searchsorted in uint64
    scatter       the priority write-back

Plain helper module (no GPU, no fixtures)."""
import numpy as np

from tests import loss_parity as lp

F4, F8 = np.float32, np.float64
Q_MAX = 2 ** 31 - 1
MUTANTS = ("w_unclamped", "dval_sign", "inv_b", "entropy_kept", "w_diff")


def sil_row(X, x, a, v, R, hp, rk=None, mut=()):
    """The SIL row of ppo_sil_loss_kernel from the raw logits of the rows' own net to the gradients, the row's w and the per-row terms of
    the sums.  x [n][K], v, R [n] (typed by X.c), a int [n]; hp = (sil_coeff, sil_value_coeff, inv_bs) as fp32 numbers.  mut: a dict of
    one-statement mutants (MUTANTS): "inv_b" and "entropy_kept" carry the value they need (inv_b; ent_coeff * inv_b)."""
    sc, svc, inv_bs = (X.c(F4(h)) for h in hp)
    one, zero = X.c(1.0), X.c(0.0)
    K = x.shape[-1]
    lg, pk, H, s, t = lp.front(X, x, rk, ())
    lp_ = X.take(lg, np.asarray(a)[:, None])[..., 0]
    dR = R - v
    w = dR if "w_unclamped" in mut else X.fmax(dR, zero)
    terms = dict(pol=(-lp_) * w, val=w * w, w=w, pos=X.count(X.gt(w, zero)), nll=-lp_, adv=X.absv(dR), n=one + zero * w)
    ib = X.c(F4(mut["inv_b"])) if "inv_b" in mut else inv_bs
    dval = -(svc * ib * w)
    if "dval_sign" in mut:
        dval = svc * ib * w
    if "w_diff" in mut:                                   # w differentiated in the policy term: d(-lp w)/dv = lp where w > 0
        dval = dval + X.fwhere(X.gt(w, zero), sc * ib * lp_, zero)
    gw = sc * ib * w
    hit = X.where(lp._onehot(a, K), one, zero)
    gk = gw[..., None] * (pk - hit)
    if "entropy_kept" in mut:
        gk = gk + (-X.c(F4(mut["entropy_kept"]))) * (-pk * (lg + H[..., None]))
    if rk is not None:
        gk = lp.ord_backward(X, gk, s, t, rk, ())
    return gk, dval, w, terms


def sil_loss_torch(logits, values, actions, returns, sil_coeff, sil_value_coeff):
    """torch: sil_coeff * mean(-lp w) + sil_value_coeff * mean(0.5 w^2), w = max(R - v, 0) a CONSTANT in the policy term (detached) and
    differentiated in the value term.  logits [n][K] raw categorical logits, the rest [n].  -> (total, policy term, value term)."""
    import torch
    lg = torch.log_softmax(logits, -1)
    lp_ = lg.gather(1, actions.view(-1, 1)).view(-1)
    w = torch.clamp(returns - values, min=0)
    pol = sil_coeff * (-lp_ * w.detach()).mean()
    val = sil_value_coeff * (0.5 * w * w).mean()
    return pol + val, pol, val


# ----------------------------------------------------------------------------- the buffer's statements
def closed_scan(rewards, masks, time_limits, values, gamma, tail, scale=None, clip_r=None):
    """One storage: rewards, masks, time_limits (or None), values fp32 [T + 1] -> (R fp32 [T], flags int32 [T + 1]: closed | eligible << 1,
    flags[T] = 0).  The scan of cadre_gae_multi with tau = 1 and V = 0 in strict fp32; tail "bootstrap" starts the chains from values[T] and,
    at a time-limit row, from values[t]."""
    T = len(rewards) - 1
    r = np.asarray(rewards, F4).copy()
    if scale is not None:
        r = np.clip(r * F4(scale), -F4(clip_r), F4(clip_r)).astype(F4)
    m = np.asarray(masks, F4)
    keep = (F4(1.0) - np.asarray(time_limits, F4)) if time_limits is not None else np.ones(T + 1, F4)
    V = np.asarray(values, F4)
    g = F4(gamma)
    boot = tail == "bootstrap"
    gae = V[T] if boot else F4(0.0)
    R, flags = np.zeros(T, F4), np.zeros(T + 1, np.int32)
    closed = False
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(T - 1, -1, -1):
            t3 = F4(r[t] + F4(F4(g * F4(0.0)) * m[t]))
            delta = F4(t3 - F4(0.0))
            gae = F4(delta + F4(F4(g * m[t]) * gae))
            gae = F4(gae * keep[t])
            if keep[t] != F4(1.0):
                closed = False
                if boot:
                    gae = V[t]
            elif m[t] == 0:
                closed = True
            R[t] = F4(gae + F4(0.0))
            flags[t] = (1 if closed else 0) | (2 if (closed or boot) else 0)
    return R, flags


def quantise(w, alpha, prio_eps):
    """float64: clamp(floor((w + prio_eps)^alpha 2^16), 1, 2^31 - 1) as int64 (w: fp32 numbers >= 0)."""
    x = np.floor(np.power(np.asarray(w, F8) + F8(prio_eps), F8(alpha)) * 65536.0)
    return np.clip(np.where(np.isnan(x), 1.0, x), 1.0, float(Q_MAX)).astype(np.int64)


def initial_priorities(R, flags, values, alpha, prio_eps):
    """q [T + 1] of one storage at append: quantise(max(R - v, 0)) on eligible rows (fp32 subtraction), 0 elsewhere and on row T."""
    T = len(R)
    w = np.maximum(np.asarray(R, F4) - np.asarray(values, F4)[:T], F4(0.0))
    q = np.zeros(T + 1, np.int64)
    q[:T] = np.where((np.asarray(flags)[:T] & 2) != 0, quantise(w, alpha, prio_eps), 0)
    return q


def draw(q, filled, u):
    """q [Rcap] non-negative integers, u [n] non-negative int64 -> the smallest row r with cum[r] > u mod total, cum the inclusive prefix sum
    of q[:filled] in uint64 (rows >= filled count as 0)."""
    cum = np.cumsum(np.asarray(q)[:filled].astype(np.uint64), dtype=np.uint64)
    total = cum[-1]
    assert total >= 1
    t = np.asarray(u).astype(np.uint64) % total
    return np.searchsorted(cum, t, side="right").astype(np.int64)


def scatter(q, idx, sil_w, pos, B_ppo, alpha, prio_eps):
    """q [Rcap] (a copy is returned) after q[idx[j]] = quantise(sil_w[pos[B_ppo + j]]); pos None: the identity."""
    q = np.array(q, dtype=np.int64)
    for j, r in enumerate(np.asarray(idx)):
        d = B_ppo + j if pos is None else int(pos[B_ppo + j])
        q[int(r)] = int(quantise(max(F4(sil_w[d]), F4(0.0)), alpha, prio_eps))
    return q
