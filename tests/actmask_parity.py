"""Element-wise float64 parity bound for cadre_ppo_am_loss (csrc/actmask.hip): the running first-order bound of tests/loss_parity.py,
|got - v64| <= err64 for EVERY stored element, no factor, no sample, no exempt share, an element whose bound is zero bit-equal.

The mask statements of the kernel are selects (x = on_m ? x : -inf, on_m ? term : 0): they are exact.  A forbidden lane then holds
expf(-inf) = 0 and adds an exact zero to every wave sum, so the masked row IS the unmasked row body on the allowed bins alone.  am_row
states it that way, from the pieces loss_parity already has: lp.ord_logits over all K units (an ordinal head), the allowed columns of the
bin logits, lp.ppo_row on those columns (the PPO statements and their gradient in bin space), exact zeros on the forbidden bins, then
lp.ord_backward over all K units on the masked gradient, as the kernel does.  The bound is the project's own, unchanged: no new constant.

The pressure statistic 1 - expf(lse_masked - lse_unmasked) is stated from the same front statements.  The sums go through lp.reduce_rows.

Inputs of a case (AmCase): logits 2 N(0, 1), bits Bernoulli(1/2) per bin (a row that drew none keeps one bin), the action drawn among the
allowed bins, old_logp the float64 masked log-prob plus N(0, 0.3).  Plain helper module (no GPU, no fixtures)."""
import numpy as np

from tests import actmask_ref as ar
from tests import loss_parity as lp
from tests.loss_parity import F4, F8, SENT, VE, X32, XVE, split

SHAPES_B = (1, 16, 17, 67)
SHAPES_C = (1, 4)
HEADS = ((33, 3), (64, 1))


def random_words(r, n, K, p=0.5):
    """n int64 words: each of the K bins allowed with probability p, at least one; bits >= K random garbage the kernels must ignore."""
    on = r.random_sample((n, K)) < p
    for i in np.flatnonzero(~on.any(-1)):
        on[i, r.randint(K)] = True
    junk = r.random_sample((n, 64)) < 0.5
    junk[:, :K] = on
    w = np.zeros(n, np.uint64)
    for k in range(64):
        w |= junk[:, k].astype(np.uint64) << np.uint64(k)
    return w.view(np.int64)


class AmCase(lp.LossCase):
    """Operands of one cadre_ppo_am_loss case in the addressing of lp.LossCase (kind "ppo"): pitch ldl (40 for K <= 33: columns K .. ldl-1
    and lanes >= ldl exist), net strides that do not coincide, a guard behind the buffers."""

    def __init__(self, seed, B, Ks, C, ordinal=(False, False), words="random", clip=0.1, ent_coeff=0.01):
        r = np.random.RandomState(seed)
        ldl = 64 if max(Ks) > 40 else 40
        self.kind, self.B, self.Ks, self.C, self.ldl, self.seed = "ppo", B, tuple(Ks), C, ldl, seed
        self.ldv, self.l_ns, self.v_ns, self.guard = 3, B * ldl + 24, B * 3 + 5, 40
        self.ord = np.stack([lp.rank_table(Ks[0], ordinal[0]), lp.rank_table(Ks[1], ordinal[1])])
        self.ordinal = tuple(ordinal)
        self.hp = dict(clip=F4(clip), value_coeff=F4(0.5), clip_coeff=F4(1.0), ent_coeff=F4(ent_coeff), inv_b=F4(1.0 / B))
        self.logits = np.full(2 * C * self.l_ns + self.guard, SENT, F4)
        self.values = np.full(2 * C * self.v_ns + self.guard, SENT, F4)
        for net in range(2 * C):
            K = Ks[net // C]
            blk = np.full((B, ldl), F4(3.25))                                       # pitch columns: never read
            blk[:, :K] = (2.0 * r.standard_normal((B, K))).astype(F4)
            self.logits[net * self.l_ns: net * self.l_ns + B * ldl] = blk.reshape(-1)
            self.values[net * self.v_ns: net * self.v_ns + B * self.ldv: self.ldv] = r.standard_normal(B).astype(F4)
        self.cmds = r.randint(0, C, (2, B)).astype(np.int32)
        if B >= 15:
            self.cmds[0, 2], self.cmds[1, 5] = -1, C                                # rows no net owns: exact zeros
        self.allowed = np.stack([random_words(r, B, K) for K in Ks])
        if words == "all":
            self.allowed = np.stack([np.full(B, ar.all_word(K), np.uint64).view(np.int64) for K in Ks])
        elif words == "empty":                                                      # no bit among the K bins: unmasked
            self.allowed = np.stack([(np.full(B, (2 ** 64 - 1) ^ ar.all_word(K), np.uint64) if K < 64 else np.zeros(B, np.uint64)).view(np.int64)
                                     for K in Ks])
        elif words == "single":                                                     # one allowed bin per row
            self.allowed = np.stack([(np.uint64(1) << r.randint(0, K, B).astype(np.uint64)).view(np.int64) for K in Ks])
        self.actions = np.zeros((2, B), np.int64)
        for h in range(2):
            on = ar.bits(ar.effective(self.allowed[h], Ks[h])[0], Ks[h])
            for b in range(B):
                self.actions[h, b] = r.choice(np.flatnonzero(on[b]))
        self.kindrow = np.zeros((2, B), np.int32)
        self.old_v = r.standard_normal((2, B)).astype(F4)
        self.rets = r.standard_normal((2, B)).astype(F4)
        self.adv = r.standard_normal((2, B)).astype(F4)
        self.weights, self.planted = None, np.zeros((2, B), bool)
        self.old_lp = np.zeros((2, B), F4)
        noise = 0.3 * r.standard_normal((2, B))
        for h in range(2):
            rows = self.rows(h, None)
            if rows.size:
                lpm, _H = ar.evaluate(self.own_logits(h, rows).astype(F8), self.actions[h, rows], self.allowed[h, rows], Ks[h], self.rk(h))
                self.old_lp[h, rows] = (lpm + (0.0 if words == "single" else noise[h, rows])).astype(F4)

    def tag(self):
        return "am B %d K %s C %d ldl %d ord %s seed %d" % (self.B, self.Ks, self.C, self.ldl, "".join("o" if o else "c" for o in self.ordinal), self.seed)

    def dense(self):
        """(logits [2C][B][ldl], values [2C][B]) float64: the layout tests/actmask_ref.loss takes."""
        B, C, ldl = self.B, self.C, self.ldl
        lg = np.stack([self.logits[n * self.l_ns: n * self.l_ns + B * ldl].reshape(B, ldl) for n in range(2 * C)]).astype(F8)
        vv = np.stack([self.values[n * self.v_ns: n * self.v_ns + B * self.ldv: self.ldv] for n in range(2 * C)]).astype(F8)
        return lg, vv


def _cat(parts, pair, n_rows, K):
    """Compacted columns back to K bins: exact zeros on the forbidden bins."""
    idx, g = parts
    gv, ge = split(g)
    if pair:
        out = VE(np.zeros((n_rows, K)))
        out.v[:, idx], out.e[:, idx] = gv, ge
        return out
    out = np.zeros((n_rows, K), gv.dtype)
    out[:, idx] = gv
    return out


def am_row(X, x, a, v, ov, R, olp, A, hp, word, rk=None, mut=()):
    """ONE row of ppo_am_loss_kernel (first axis of every operand: 1).  x [1][K] raw tower outputs, word the row's int64 word; the rest as
    lp.ppo_row.  Returns (gk [1][K], dval, terms); terms gains proper, nbins, press, forced."""
    pair = isinstance(X, XVE)
    K = x.shape[-1]
    m, forced = ar.effective(np.asarray([word]), K, None if "no_or" in mut else np.asarray(a))
    on = ar.bits(m, K)[0]
    if "mask_off" in mut:
        on = np.ones(K, bool)
    idx = np.flatnonzero(on)
    s = t = None
    xb = x
    if rk is not None:
        xb, s, t = lp.ord_logits(X, x, rk, mut)
    if "mask_before_ord" in mut and rk is not None:                                 # (mutant: the mask in rank space)
        idx = np.flatnonzero(on[np.argsort(rk)])
    xc = xb[:, idx]
    ac = np.asarray([int(np.flatnonzero(idx == int(a[0]))[0])]) if int(a[0]) in idx else np.asarray([0])
    gkc, dval, terms = lp.ppo_row(X, xc, ac, v, ov, R, olp, A, hp, None, mut)        # bin space, allowed bins only
    gk = _cat((idx, gkc), pair, 1, K)
    if rk is not None:
        gk = lp.ord_backward(X, gk, s, t, rk, mut)
    # the mask statistics: the pressure from the front's own statements on both rows
    proper = idx.size != K
    one, zero = X.c(1.0), X.c(0.0)
    if proper:
        mxm = X.max(xc)
        lse_m = mxm + X.log(X.sum(X.exp(xc - mxm[..., None])))
        mxu = X.max(xb)
        lse_u = mxu + X.log(X.sum(X.exp(xb - mxu[..., None])))
        press = X.fmin(X.fmax(one - X.exp(lse_m - lse_u), zero), one)
    else:
        press = X.c(np.zeros(1))
    cst = X.c
    terms = dict(terms, proper=cst(np.full(1, 1.0 if proper else 0.0)), nbins=cst(np.full(1, float(idx.size))), press=press,
                 forced=cst(np.full(1, 1.0 if forced[0] else 0.0)))
    return gk, dval, terms


def run_am(case, X, hp=None, mut=()):
    """One launch of cadre_ppo_am_loss in the arithmetic of X (an lp.X64 / lp.X32 instance, or the class lp.XVE) -> dict of typed outputs:
    dlogits / dvalues (flat), losses [3], stats [6] of typed [2], am_stats [4] of typed [2]; with XVE `amb`."""
    c = case
    hpv = dict(c.hp)
    hpv.update(hp or {})
    B, C, ldl = c.B, c.C, c.ldl
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
    names = ("val", "act", "ent", "kl", "okl", "cf", "vcf", "r", "alr", "proper", "nbins", "press", "forced", "n")
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
        for b in c.rows(h, None):
            rows = np.asarray([b])
            x_ = mk(1)
            cst = x_.c if pair else (lambda a_: np.asarray(a_, x_.dtype))
            gk, dval, terms = am_row(x_, cst(c.own_logits(h, rows)), c.actions[h, rows], cst(c.own_values(h, rows)),
                                     cst(c.old_v[h, rows]), cst(c.rets[h, rows]), cst(c.old_lp[h, rows]), cst(c.adv[h, rows]), hp5,
                                     c.allowed[h, b], c.rk(h), mut)
            terms["n"] = cst(np.ones(1, F4))
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
    red = lambda t, per_head=False, use_max=False: lp.reduce_rows(x_, t, B, per_head, use_max)
    half, ib = cc(0.5), cc(hpv["inv_b"])
    out["losses"] = [cc(hpv["value_coeff"]) * half * red(tp["val"]) * ib, cc(hpv["clip_coeff"]) * red(tp["act"]) * ib,
                     cc(hpv["ent_coeff"]) * red(tp["ent"]) * ib]
    out["stats"] = [red(tp[k], True) * ib for k in ("kl", "okl", "cf", "vcf", "r")] + [red(tp["alr"], True, True)]
    # the mask statistics per head: shares and means over the head's counted rows (zeros without one), OR-ed rows as a count
    cnt = red(tp["n"], True)
    cv = np.maximum(split(cnt)[0], 1.0)
    den = VE(cv) if pair else cv.astype(x_.dtype)
    out["am_stats"] = [red(tp[k], True) / den for k in ("proper", "nbins", "press")] + [red(tp["forced"], True)]
    return out


def check_am(case, got, ref, what, stats=True, am_stats=True, quiet=False):
    """got: dict of arrays as a launch (or an X32 emulation) left them; ref: run_am(case, XVE, ...).  Checks every stored element; returns
    (worst err / bound, ambiguous rows)."""
    rep = lp.Report(what)
    ml, mv = lp.written(case)
    rep.check("dlogits", got["dlogits"], ref["dlogits"], ml, SENT)
    rep.check("dvalues", got["dvalues"], ref["dvalues"], mv, SENT)
    v = np.array([split(t)[0] for t in ref["losses"]]).reshape(-1)
    e = np.array([split(t)[1] for t in ref["losses"]]).reshape(-1)
    rep.check("losses", np.asarray(got["losses"], F8).reshape(-1)[:3], VE(v, e))
    for name, on, n in (("stats", stats, 6), ("am_stats", am_stats, 4)):
        if on:
            v = np.stack([np.reshape(split(t)[0], -1) for t in ref[name]], 1)
            e = np.stack([np.reshape(split(t)[1], -1) for t in ref[name]], 1)
            rep.check(name, np.asarray(got[name], F8)[:, :n], VE(v, e))
    n_amb = int(ref["amb"].sum())
    rep.finish(n_amb, quiet)
    return rep.worst, n_amb


def emulate_am(case, order="tree", mut=(), **kw):
    """The X32 emulation's outputs in the layout check_am takes."""
    o = run_am(case, X32(order), mut=mut, **kw)
    out = dict(dlogits=o["dlogits"], dvalues=o["dvalues"])
    out["losses"] = np.array([float(np.reshape(t, -1)[0]) for t in o["losses"]])
    for name in ("stats", "am_stats"):
        out[name] = np.stack([np.asarray(t, F8).reshape(-1) for t in o[name]], 1)
    return out
