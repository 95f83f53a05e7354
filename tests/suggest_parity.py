"""Element-wise float64 parity bound for cadre_ppo_sug_loss (csrc/suggest.hip): the running first-order bound of tests/loss_parity.py,
|got - v64| <= err64 for EVERY stored element, no factor, no sample, no exempt share, an element whose bound is zero bit-equal.

The row body of a marked row is written ONCE (suggest_row), generic over the operand namespaces lp.X64 / lp.X32 / lp.XVE, from the pieces
loss_parity already states: lp.ord_logits (an ordinal head's bin logits), lp.ppo_row on those bin logits (the PPO statements and their
gradient in bin space), lp.front (lg, p), then the suggestion statements, then lp.ord_backward on the SUM of both gradients, as the kernel
does.  An unmarked row is lp.ppo_row itself.  The sums go through lp.reduce_rows.

The suggestion term has no branch: no comparison of the row body depends on it, so the ambiguous rows of a case are those of its PPO part
(at most one per case, planted ties aside; tests/test_suggest_cpu.py asserts it from the pairs).  The cases are lp.PPO_CASES — the shape
grid, seeds and planted rows of the PPO loss — each with a kind pattern, a prior table and Z laid over it.

`mut` names one-statement mutants of the body (tests/test_suggest_cpu.py).  Plain helper module (no GPU, no fixtures)."""
import numpy as np

from tests import loss_parity as lp
from tests.loss_parity import F4, F8, SENT, VE, X32, XVE, split

SUG_COEFF = F4(0.6)
PATTERNS = ("none", "all", "alt")


def prior_table(seed, Ks, Z):
    """float32 [2][Z + 1][64] RAW log-priors: log of random probabilities with one bin at 1e-6 (K > 1), shifted by a constant per kind
    (the kernel's normalisation has something to do), columns >= K and row 0 a value that is never read."""
    r = np.random.RandomState(1000 + seed)
    out = np.full((2, Z + 1, 64), 2.75, F4)
    for h in range(2):
        K = Ks[h]
        for z in range(1, Z + 1):
            p = r.uniform(0.05, 1.0, K)
            if K > 1:
                p[r.randint(K)] = 1e-6
            if z % 3 == 0 and K > 2:
                p[:] = 0.01
                p[r.randint(K)] = 1.0                                    # a peaked prior
            out[h, z, :K] = (np.log(p / p.sum()) + (1.5 * z - 3.0)).astype(F4)
    return out


def kind_pattern(B, Z, pattern):
    """int32 [2][B]: no row marked / every row marked / alternating rows marked, the kinds cycling through 1 .. Z; with B >= 15 two
    entries hold -1 and Z + 1 (treated as 0)."""
    k = np.zeros((2, B), np.int32)
    if pattern == "none":
        return k
    for h in range(2):
        for b in range(B):
            if pattern == "all" or (b + h) % 2 == 1:
                k[h, b] = 1 + (b // 2 + h) % Z
    if B >= 15:
        k[0, 9], k[1, 10] = -1, Z + 1
    return k


class SugCase:
    """A lp.LossCase of kind "ppo" (operands, planted rows) with a kind array, a prior table and Z."""

    def __init__(self, i, pattern, Z, sug_coeff=SUG_COEFF):
        self.base = lp.LossCase(kind="ppo", **lp.PPO_CASES[i])
        self.i, self.pattern, self.Z = i, pattern, Z
        self.kind = kind_pattern(self.base.B, Z, pattern)
        self.prior = prior_table(self.base.seed, self.base.Ks, Z)
        self.sug_coeff = F4(sug_coeff)

    def eff(self):
        return np.where((self.kind < 1) | (self.kind > self.Z), 0, self.kind)

    def tag(self):
        return "%s pattern %s Z %d" % (self.base.tag(), self.pattern, self.Z)


def suggest_row(X, x, a, v, ov, R, olp, A, hp, y, sc, rk=None, mut=()):
    """A marked row of ppo_sug_loss_kernel.  x [n][K] raw tower outputs, y [n][K] the rows' RAW log-prior rows (typed by X.c), sc the
    fp32 suggestion coefficient, the rest as lp.ppo_row.  Returns (gk, dval, terms); terms gains skl (the row's kl) and pm (the
    probability the policy gives the prior's mode)."""
    inv_b = X.c(F4(hp[4]))
    s = t = None
    xb = x
    if rk is not None:
        xb, s, t = lp.ord_logits(X, x, rk, mut)
    gk, dval, terms = lp.ppo_row(X, xb, a, v, ov, R, olp, A, hp, None, mut)         # bin space: no ord_backward yet
    lg, pk, _H, _s, _t = lp.front(X, xb, None, mut)
    if "prior_raw" in mut:
        lq = y
    else:
        qmx = X.max(y)
        qse = X.sum(X.exp(y - qmx[..., None]))
        lq = y - (qmx + X.log(qse))[..., None]
    df = lg - lq
    kl = X.sum(pk * df)
    coeff = X.c(F4(sc)) * inv_b
    if "kl_reversed" in mut:
        gs = coeff * (pk - X.exp(lq))
    elif "no_centre" in mut:
        gs = coeff * (pk * df)
    else:
        gs = coeff * (pk * (df - kl[..., None]))
    gk = gk + gs
    if rk is not None:
        gk = lp.ord_backward(X, gk, s, t, rk, mut)
    mode = np.argmax(split(y)[0], -1)                                               # the lowest index among the largest raw entries
    terms = dict(terms, skl=kl, pm=X.take(pk, mode[:, None])[..., 0])
    return gk, dval, terms


def run_sug(case, X, hp=None, kind=None, mut=()):
    """One launch of cadre_ppo_sug_loss in the arithmetic of X (an lp.X64 / lp.X32 instance, or the class lp.XVE) -> dict of typed
    outputs: dlogits / dvalues (flat), losses [3], sug_losses [1], stats [6] of typed [2], sug_stats [4] of typed [2]; with XVE `amb`.
    hp overrides the base case's scalars and "sug_coeff"; kind overrides the case's kind array."""
    c = case.base
    hpv = dict(c.hp, sug_coeff=case.sug_coeff)
    hpv.update(hp or {})
    B, C, ldl, Z = c.B, c.C, c.ldl, case.Z
    kz = case.eff() if kind is None else np.where((np.asarray(kind) < 1) | (np.asarray(kind) > Z), 0, np.asarray(kind))
    pair = X is XVE
    mk = (lambda n: XVE(n)) if pair else (lambda n: X)
    if pair:
        dl, dv = VE(np.zeros(c.logits.size)), VE(np.zeros(c.values.size))
    else:
        dl, dv = np.full(c.logits.size, SENT, X.dtype), np.full(c.values.size, SENT, X.dtype)
        for net in range(2 * C):
            for b in range(B):
                dl[net * c.l_ns + b * ldl: net * c.l_ns + (b + 1) * ldl] = 0
                dv[net * c.v_ns + b * c.ldv] = 0
    amb = np.zeros((2, B), bool)
    names = ("val", "act", "ent", "kl", "okl", "cf", "vcf", "r", "alr", "skl", "pm", "n")
    zero_t = (lambda: VE(np.zeros((2, B)))) if pair else (lambda: np.zeros((2, B), X.dtype))
    tp = {k: zero_t() for k in names}

    def put(buf, idx, val):
        v, e = split(val)
        if pair:
            buf.v[idx], buf.e[idx] = v, e
        else:
            buf[idx] = v

    hp5 = (hpv["clip"], hpv["value_coeff"], hpv["clip_coeff"], hpv["ent_coeff"], hpv["inv_b"])
    for h in range(2):
        K = c.Ks[h]
        ok = c.rows(h, None)
        for marked in (False, True):
            rows = ok[(kz[h, ok] != 0) == marked]
            if rows.size == 0:
                continue
            x_ = mk(rows.size)
            cst = x_.c if pair else (lambda a_: np.asarray(a_, x_.dtype))
            args = (cst(c.own_logits(h, rows)), c.actions[h, rows], cst(c.own_values(h, rows)), cst(c.old_v[h, rows]),
                    cst(c.rets[h, rows]), cst(c.old_lp[h, rows]), cst(c.adv[h, rows]), hp5)
            if marked:
                sc = hpv["sug_coeff"]
                if "mean_marked" in mut:                                            # the mean over the marked rows of the head
                    sc = F4(sc) * F4(B) / F4(rows.size)
                y = cst(case.prior[h, kz[h, rows], :K])
                gk, dval, terms = suggest_row(x_, *args, y, sc, c.rk(h), mut)
                terms["n"] = cst(np.ones(rows.size, F4))
            else:
                gk, dval, terms = lp.ppo_row(x_, *args, c.rk(h), mut)
            for k, t in terms.items():
                put(tp[k], (h, rows), t)
            if pair:
                amb[h, rows] |= x_.amb
            net = h * C + c.cmds[h, rows]
            put(dl, (net * c.l_ns + rows * ldl)[:, None] + np.arange(K)[None, :], gk)
            put(dv, net * c.v_ns + rows * c.ldv, dval)
    out = dict(dlogits=dl, dvalues=dv, amb=amb)
    x_ = mk(2)
    cc = x_.c if pair else (lambda a_: np.asarray(a_, x_.dtype))
    red = lambda t, per_head=False: lp.reduce_rows(x_, t, B, per_head)
    half, ib = cc(0.5), cc(hpv["inv_b"])
    out["losses"] = [cc(hpv["value_coeff"]) * half * red(tp["val"]) * ib, cc(hpv["clip_coeff"]) * red(tp["act"]) * ib,
                     cc(hpv["ent_coeff"]) * red(tp["ent"]) * ib]
    sc = hpv["sug_coeff"]
    if "mean_marked" in mut:
        n_m = max(1, int((kz[0, c.rows(0, None)] != 0).sum()))
        sc = F4(sc) * F4(B) / F4(n_m)
    out["sug_losses"] = [cc(F4(sc)) * red(tp["skl"]) * ib]
    out["stats"] = [red(tp[k], True) * ib for k in ("kl", "okl", "cf", "vcf", "r")] + [lp.reduce_rows(x_, tp["alr"], B, True, True)]
    # the suggestion statistics per head: marked rows, mean kl over the minibatch, max kl (0 without a marked row), mean p[mode]
    cnt = red(tp["n"], True)
    cv = split(cnt)[0]
    mkl_v, mkl_e, pm_v, pm_e = np.zeros(2), np.zeros(2), np.zeros(2), np.zeros(2)
    pm_sum = red(tp["pm"], True)
    for h in range(2):
        rows = np.flatnonzero(split(tp["n"])[0][h] != 0)
        if rows.size == 0:
            continue
        kv, ke = split(tp["skl"])
        mkl_v[h] = kv[h, rows].max()
        mkl_e[h] = 0.0 if ke is None else ke[h, rows].max()
        q = (pm_sum[h] if pair else pm_sum[h:h + 1]) / (cnt[h] if pair else cnt[h:h + 1])
        qv, qe = split(q)
        pm_v[h], pm_e[h] = float(np.reshape(qv, -1)[0]), 0.0 if qe is None else float(np.reshape(qe, -1)[0])
    if pair:
        out["sug_stats"] = [cnt, red(tp["skl"], True) * ib, VE(mkl_v, mkl_e), VE(pm_v, pm_e)]
    else:
        out["sug_stats"] = [cnt, red(tp["skl"], True) * ib, mkl_v.astype(x_.dtype), pm_v.astype(x_.dtype)]
    assert (cv == np.round(cv)).all()
    return out


def check_sug(case, got, ref, what, stats=True, quiet=False):
    """got: dict of arrays as a launch (or an X32 emulation) left them; ref: run_sug(case, XVE, ...).  Checks every stored element;
    returns (worst err / bound, ambiguous rows that were not planted)."""
    rep = lp.Report(what)
    ml, mv = lp.written(case.base)
    rep.check("dlogits", got["dlogits"], ref["dlogits"], ml, SENT)
    rep.check("dvalues", got["dvalues"], ref["dvalues"], mv, SENT)
    for name in ("losses", "sug_losses"):
        v = np.array([split(t)[0] for t in ref[name]]).reshape(-1)
        e = np.array([split(t)[1] for t in ref[name]]).reshape(-1)
        rep.check(name, np.asarray(got[name], F8).reshape(-1)[:v.size], VE(v, e))
    if stats:
        v = np.stack([split(t)[0] for t in ref["stats"]], 1)
        e = np.stack([split(t)[1] for t in ref["stats"]], 1)
        rep.check("stats", np.asarray(got["stats"], F8)[:, :6], VE(v, e))
    v = np.stack([split(t)[0] for t in ref["sug_stats"]], 1)
    e = np.stack([split(t)[1] for t in ref["sug_stats"]], 1)
    rep.check("sug_stats", np.asarray(got["sug_stats"], F8)[:, :4], VE(v, e))
    n_amb = int((ref["amb"] & ~case.base.planted).sum())
    rep.finish(n_amb, quiet)
    return rep.worst, n_amb


def emulate_sug(case, order="tree", mut=(), **kw):
    """The X32 emulation's outputs in the layout check_sug takes."""
    o = run_sug(case, X32(order), mut=mut, **kw)
    out = dict(dlogits=o["dlogits"], dvalues=o["dvalues"])
    for name in ("losses", "sug_losses"):
        out[name] = np.array([float(np.reshape(t, -1)[0]) for t in o[name]])
    for name in ("stats", "sug_stats"):
        out[name] = np.stack([np.asarray(t, F8) for t in o[name]], 1)
    return out
