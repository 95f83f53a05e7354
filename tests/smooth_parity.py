"""The running first-order bound of tests/loss_parity.py for cadre_ppo_smooth_loss: one launch of the kernel in the arithmetic of X64 /
X32 / XVE (the PPO statements through loss_parity.ppo_row, the pair statements through smooth_ref.smooth_pair), and the check of every
stored element.  The pairs of value and running first-order error go through mu, d, the loss and the gradient in the tree order of
wave_sum.  No new tolerance: the unit constants are loss_parity's.

A case is a loss_parity.LossCase(kind="ppo") of B = (nW + E) Bw rows over synthetic storages of T = 2 Bw + 1 rows: worker rows sit on even
t (so that row t + 1 is never a worker row and its command is free), the successor entries are built by the host rule min(t + 1, T - 1),
and the kinds and partners come from smooth_ref.smooth_mates.  Planted in every head, on the slots of the first successor entry: a pair
whose two raw logit rows are bit-equal (d == 0), a slot invalid by mask, by time limit, by a command change, and a slot with t = T - 1.

Plain helper module (no GPU, no fixtures)."""
import numpy as np

from tests import loss_parity as lp
from tests import smooth_ref as ref
from tests.loss_parity import F4, F8, SENT, VE, X32, XVE, split

SMOOTH_HP = dict(smooth_coeff=F4(0.4), scale_steer=F4(1.0), scale_throttle=F4(0.5))
# (Bw, nW, E) -> B: (12, 1, 1) -> 24; (5, 3, 2) -> 25, a partial workgroup and a rotation that leaves a worker unpaired; (8, 3, 3) -> 48;
# (75, 2, 2) -> 300.  Bins (33, 3); C 1 / 4; pitch 64 / 40; plain, ordinal and mixed heads.  Seeds: chosen so that the float64 pairs alone
# meet at most one ambiguous row (loss_parity's condition; tests/test_smooth_cpu.py asserts it).
SMOOTH_CASES = [
    dict(seed=101, Bw=12, nW=1, E=1, step=0, C=4, ldl=64, scale=1.0),
    dict(seed=102, Bw=12, nW=1, E=1, step=3, C=1, ldl=40, scale=4.0, ordinal=(True, True)),
    dict(seed=103, Bw=5, nW=3, E=2, step=1, C=4, ldl=40, scale=1.0, ordinal=(True, False)),
    dict(seed=104, Bw=5, nW=3, E=2, step=2, C=1, ldl=64, scale=4.0),
    dict(seed=105, Bw=8, nW=3, E=3, step=1, C=4, ldl=64, scale=1.0, ordinal=(False, True)),
    dict(seed=106, Bw=8, nW=3, E=3, step=0, C=1, ldl=40, scale=1.0),
    dict(seed=107, Bw=75, nW=2, E=2, step=1, C=4, ldl=64, scale=1.0),
    dict(seed=108, Bw=75, nW=2, E=2, step=0, C=1, ldl=40, scale=4.0, ordinal=(True, True)),
]
SHAPES = [(12, 1, 1), (5, 3, 2), (8, 3, 3), (75, 2, 2)]
PLANTS = ("equal", "mask", "limit", "command", "last")


def case_id(kw):
    return "Bw%d-nW%d-E%d-C%d-ldl%d-%s" % (kw["Bw"], kw["nW"], kw["E"], kw["C"], kw["ldl"],
                                          "".join("o" if o else "c" for o in kw.get("ordinal", (False, False))))


def ctrl_table(Ks):
    """float32 [2][64]: a steer table of the shipped shape (non-monotone in the bin index) and throttle - brake of three bins."""
    c = np.zeros((2, 64), F8)
    for h, K in enumerate(Ks):
        if K == 3:
            c[h, :3] = [0.0 - 1.0, 0.0 - 0.0, 0.7 - 0.0]
        else:
            n = (K + 1) // 2
            c[h, :n] = np.linspace(-0.5, 0.5, n)
            c[h, n:K] = [(0.5 + 0.5 * (j // 2 + 1) / max(1, (K - n + 1) // 2)) * (1.0 if j % 2 == 0 else -1.0) for j in range(K - n)]
    return c.astype(F4)


def smooth_case(kw, layout="random"):
    """The LossCase of one SMOOTH_CASES entry with its storages, pairs and planted slots.  layout "prefix": workspace position = unsorted
    row; "random": a permutation per head (the same pairs at other positions)."""
    kw = dict(kw)
    Bw, nW, E, step = (kw.pop(k) for k in ("Bw", "nW", "E", "step"))
    B = (nW + E) * Bw
    c = lp.LossCase(kind="ppo", B=B, Ks=(33, 3), **kw)
    r = np.random.RandomState(kw["seed"] + 7000)
    C, T = c.C, 2 * Bw + 1
    c.Bw, c.nW, c.E, c.step, c.T, c.layout = Bw, nW, E, step, T, layout
    c.rotation = step * E
    c.pos = None if layout == "prefix" else np.stack([r.permutation(B) for _ in range(2)]).astype(np.int32)
    P = (lambda h, u: u) if c.pos is None else (lambda h, u: int(c.pos[h, u]))
    c.hp.update(SMOOTH_HP)
    c.hp["inv_bp"] = F4(1.0 / (E * Bw))
    c.ctrl = ctrl_table(c.Ks)
    # the step's index block: worker rows on even t, T - 1 among them; successor entries by the host rule
    idx = np.zeros((2 * (nW + E), Bw), np.int64)
    for w in range(nW):
        for h in range(2):
            even = 2 * r.permutation(Bw + 1)[:Bw]
            if T - 1 not in even:
                even[r.randint(Bw)] = T - 1
            idx[2 * w + h] = even
    for k in range(E):
        w = (c.rotation + k) % nW
        for h in range(2):
            idx[2 * (nW + k) + h] = np.minimum(idx[2 * w + h] + 1, T - 1)
    c.idx = idx
    # the storages: masks 1, no time limit, the command of row t from the case's worker row, of row t + 1 from its successor row — which
    # gets the worker row's command (a successor row reads nothing that depends on it but its own net's logits)
    c.src, c.plant = [], {}
    for w in range(nW):
        for h in range(2):
            masks, tl, cmd = np.ones(T + 1, F4), np.zeros(T + 1, F4), np.zeros(T + 1, np.int32)
            k = (w - c.rotation) % nW
            slots = list(range(Bw))
            plant = {}
            if k == 0:                                   # the first successor entry's worker carries the planted slots
                last = int(np.flatnonzero(idx[2 * w + h] == T - 1)[0])
                fam = lambda s: lp.FAMILIES[P(h, w * Bw + s) % len(lp.FAMILIES)]
                rest = sorted((s for s in slots if s != last), key=lambda s: (not c.row_ok(h, P(h, w * Bw + s)), fam(s) != "plain", s))
                assert len(rest) >= 4 and c.row_ok(h, P(h, w * Bw + rest[0])), "no row for the planted slots"
                plant = dict(zip(PLANTS[:4], rest[:4]))
                plant["last"] = last
                c.plant[h] = {name: P(h, w * Bw + s) for name, s in plant.items()}
            for s in slots:
                t = int(idx[2 * w + h][s])
                me = P(h, w * Bw + s)
                cmd[t] = c.cmds[h, me]
                if k < E and t + 1 <= T - 1:
                    you = P(h, (nW + k) * Bw + s)
                    c.cmds[h, you] = c.cmds[h, me]
                    if plant.get("command") == s:
                        c.cmds[h, you] = (c.cmds[h, me] + 1) % C if C > 1 else C
                    cmd[t + 1] = c.cmds[h, you]
                    if plant.get("equal") == s:          # bit-equal raw logit rows (same command, so the same net)
                        net = h * C + c.cmds[h, me]
                        c.logits[net * c.l_ns + you * c.ldl: net * c.l_ns + (you + 1) * c.ldl] = \
                            c.logits[net * c.l_ns + me * c.ldl: net * c.l_ns + (me + 1) * c.ldl]
                elif k < E:                              # t = T - 1: the successor entry rides with the same storage row
                    c.cmds[h, P(h, (nW + k) * Bw + s)] = c.cmds[h, me]
                if plant.get("mask") == s:
                    masks[t] = 0
                if plant.get("limit") == s:
                    tl[t] = 1
            c.src.append((masks, tl, cmd))
    c.kindrow, c.mate = ref.smooth_mates(c.src, idx, nW, E, Bw, T, C, c.rotation, c.pos, B)
    return c


def smooth_cases(layout="random"):
    return [smooth_case(kw, layout) for kw in SMOOTH_CASES]


def paired_rows(case, h, succ):
    """Workspace rows of head h of kind `succ` that have a partner and count (own and mate's command in range)."""
    ok = (case.cmds[h] >= 0) & (case.cmds[h] < case.C) & (case.mate[h] >= 0) & (case.kindrow[h] == (1 if succ else 0))
    rows = np.flatnonzero(ok)
    cm = case.cmds[h, case.mate[h, rows]]
    return rows[(cm >= 0) & (cm < case.C)]


def run_smooth(case, X, hp=None, stats=True, mut=()):
    """One launch of cadre_ppo_smooth_loss in the arithmetic of X -> dict of typed outputs: dlogits / dvalues (flat buffers: SENT where
    the emulation wrote nothing; pairs hold (0, 0) there), smooth_d [2][B], losses [3], stats [6] of [2], smooth_losses [1], smooth_stats
    [4] of [2]; with XVE also `amb` [2][B].  mut: a set of smooth_ref.MUTANTS."""
    hpv = dict(case.hp)
    hpv.update(hp or {})
    B, C, ldl = case.B, case.C, case.ldl
    pair = X is XVE
    mk = (lambda n: XVE(n)) if pair else (lambda n: X)
    if pair:
        dl, dv, sd = VE(np.zeros(case.logits.size)), VE(np.zeros(case.values.size)), VE(np.zeros((2, B)))
    else:
        dt = X.dtype
        dl, dv, sd = np.full(case.logits.size, SENT, dt), np.full(case.values.size, SENT, dt), np.zeros((2, B), dt)
        for net in range(2 * C):
            for b in range(B):
                dl[net * case.l_ns + b * ldl: net * case.l_ns + (b + 1) * ldl] = 0
                dv[net * case.v_ns + b * case.ldv] = 0
    amb = np.zeros((2, B), bool)
    names_p = ("val", "act", "ent", "kl", "okl", "cf", "vcf", "r", "alr")
    names_s = ("n", "ad", "d2")
    zero_t = (lambda: VE(np.zeros((2, B)))) if pair else (lambda: np.zeros((2, B), X.dtype))
    tp, ts = {k: zero_t() for k in names_p}, {k: zero_t() for k in names_s}

    def put(buf, idx, val):
        v, e = split(val)
        if pair:
            buf.v[idx], buf.e[idx] = v, e
        else:
            buf[idx] = v

    def raw(h, rows, cmds):
        net = h * C + cmds
        return case.logits[(net * case.l_ns + rows * ldl)[:, None] + np.arange(case.Ks[h])[None, :]]

    for h in range(2):
        K = case.Ks[h]
        rk = case.rk(h)
        scale = hpv["scale_steer"] if h == 0 else hpv["scale_throttle"]
        for succ in (False, True):
            rows = paired_rows(case, h, True) if succ else case.rows(h, False)
            if rows.size == 0:
                continue
            x_ = mk(rows.size)
            cst = x_.c if pair else (lambda a: np.asarray(a, x_.dtype))
            x = cst(case.own_logits(h, rows))
            s = t = None
            xb = x
            if rk is not None:
                xb, s, t = lp.ord_logits(x_, x, rk, ())
            if not succ:
                hp5 = (hpv["clip"], hpv["value_coeff"], hpv["clip_coeff"], hpv["ent_coeff"], hpv["inv_b"])
                gk, dval, terms = lp.ppo_row(x_, xb, case.actions[h, rows], cst(case.own_values(h, rows)), cst(case.old_v[h, rows]),
                                             cst(case.rets[h, rows]), cst(case.old_lp[h, rows]), cst(case.adv[h, rows]), hp5, None, ())
                for k, term in terms.items():
                    put(tp[k], (h, rows), term)
                has = np.isin(rows, paired_rows(case, h, False))
            else:
                gk, dval, has = None, cst(np.zeros(rows.size, F4)), np.ones(rows.size, bool)
            if has.any():
                sub = rows[has]
                y_ = mk(sub.size)
                cs2 = y_.c if pair else (lambda a: np.asarray(a, y_.dtype))
                m = case.mate[h, sub]
                cm = case.cmds[h, m]
                if "mate_wrong_net" in mut:
                    cm = (cm + 1) % C
                xo, xm = cs2(case.own_logits(h, sub)), cs2(raw(h, m, cm))
                if rk is not None:
                    xo, xm = lp.ord_logits(y_, xo, rk, ())[0], lp.ord_logits(y_, xm, rk, ())[0]
                cf = cs2(F4(hpv["smooth_coeff"])) * cs2(F4(scale)) * cs2(F4(hpv["inv_bp"]))
                o = ref.smooth_pair(y_, xo, xm, cs2(case.ctrl[h, :K]), cf, succ, mut)
                put(sd, (h, sub), o["d"])
                if not succ or "both_count" in mut:
                    d = o["d"]
                    put(ts["d2"], (h, sub), d * d)
                    put(ts["ad"], (h, sub), y_.absv(d))
                    put(ts["n"], (h, sub), cs2(np.ones(sub.size, F4)))
                # the sum of both gradients in bin space, then ord_backward once
                gv, ge = split(o["gs"])
                if succ:
                    gk = o["gs"]
                elif pair:
                    full = VE(np.zeros(gk.v.shape))
                    full.v[has], full.e[has] = gv, ge
                    add = gk + full
                    gk = VE(np.where(has[:, None], add.v, gk.v), np.where(has[:, None], add.e, gk.e))
                else:
                    gk = np.array(gk)
                    gk[has] = gk[has] + gv
                if pair:
                    amb[h, sub] |= y_.amb
            if rk is not None:
                gk = lp.ord_backward(x_, gk, s, t, rk, ())
            if pair:
                amb[h, rows] |= x_.amb
            net = h * C + case.cmds[h, rows]
            put(dl, (net * case.l_ns + rows * ldl)[:, None] + np.arange(K)[None, :], gk)
            put(dv, net * case.v_ns + rows * case.ldv, dval)
    out = dict(dlogits=dl, dvalues=dv, smooth_d=sd, amb=amb)
    x_ = mk(2)
    c = x_.c if pair else (lambda a: np.asarray(a, x_.dtype))
    red = lambda term, per_head=False, use_max=False: lp.reduce_rows(x_, term, B, per_head, use_max)
    half, ib, ibp = c(0.5), c(hpv["inv_b"]), c(hpv["inv_bp"])
    out["losses"] = [c(hpv["value_coeff"]) * half * red(tp["val"]) * ib, c(hpv["clip_coeff"]) * red(tp["act"]) * ib,
                     c(hpv["ent_coeff"]) * red(tp["ent"]) * ib]
    S = red(ts["d2"], True)
    cf0 = c(hpv["smooth_coeff"]) * c(hpv["scale_steer"]) * ibp
    cf1 = c(hpv["smooth_coeff"]) * c(hpv["scale_throttle"]) * ibp
    out["smooth_losses"] = [cf0 * S[0] + cf1 * S[1]]
    if stats:
        out["stats"] = [red(tp[k], True) * ib for k in ("kl", "okl", "cf", "vcf", "r")] + [red(tp["alr"], True, True)]
        out["smooth_stats"] = [red(ts["n"], True), ibp * red(ts["ad"], True), red(ts["ad"], True, True), ibp * S]
    return out


def emulate_smooth(case, order="tree", mut=(), **kw):
    """The X32 emulation's outputs in the layout check_smooth takes."""
    o = run_smooth(case, X32(order), mut=mut, **kw)
    out = dict(dlogits=o["dlogits"], dvalues=o["dvalues"], smooth_d=o["smooth_d"])
    for name in ("losses", "smooth_losses"):
        out[name] = np.array([float(t) for t in o[name]])
    for name in ("stats", "smooth_stats"):
        if name in o:
            out[name] = np.stack([np.asarray(t, F8) for t in o[name]], 1)
    return out


def head_grad(case, buf, h, rows):
    """[n][ldl] rows of a flat dlogits buffer: the rows' own nets."""
    net = h * case.C + case.cmds[h, rows]
    return np.asarray(buf)[(net * case.l_ns + rows * case.ldl)[:, None] + np.arange(case.ldl)[None, :]]


def check_smooth(case, got, want, what, stats=True, quiet=False):
    """got: dict of arrays as a launch (or the X32 emulation) left them; want: run_smooth(case, XVE).  Every stored element of dlogits,
    dvalues, smooth_d, the losses and the statistics within the bound; the two d of a pair exact negatives; unpaired successor rows exact
    zeros; the bit-equal pair d == 0; untouched sentinels still sentinels."""
    rep = lp.Report(what)
    ml, mv = lp.written(case)
    rep.check("dlogits", got["dlogits"], want["dlogits"], ml, SENT)
    rep.check("dvalues", got["dvalues"], want["dvalues"], mv, SENT)
    rep.check("smooth_d", got["smooth_d"], want["smooth_d"])
    for name, n in (("losses", 3), ("smooth_losses", 1)):
        v = np.array([split(t)[0] for t in want[name]])
        e = np.array([split(t)[1] for t in want[name]])
        rep.check(name, np.asarray(got[name], F8)[:n], VE(v, e))
    if stats:
        for name, n in (("stats", 6), ("smooth_stats", 4)):
            v = np.stack([split(t)[0] for t in want[name]], 1)
            e = np.stack([split(t)[1] for t in want[name]], 1)
            rep.check(name, np.asarray(got[name], F8)[:, :n], VE(v, e))
    d = np.asarray(got["smooth_d"], F4)
    for h in range(2):
        i = paired_rows(case, h, False)
        j = case.mate[h, i]
        if not np.array_equal(d[h, i], -d[h, j]):            # (float equality: the same bits but for the sign, +0 == -0)
            rep.bad.append("the two d of a pair are not exact negatives (head %d)" % h)
        lone = np.flatnonzero((case.kindrow[h] == 1) & (case.mate[h] < 0))
        if lone.size and (np.any(d[h, lone] != 0) or np.any(got["dvalues"][(h * case.C + np.clip(case.cmds[h, lone], 0, case.C - 1)) * case.v_ns + lone * case.ldv] != 0)
                          or any(np.any(np.asarray(got["dlogits"])[net * case.l_ns + b * case.ldl: net * case.l_ns + (b + 1) * case.ldl] != 0)
                                 for b in lone for net in range(h * case.C, (h + 1) * case.C))):
            rep.bad.append("an unpaired successor row holds a non-zero d or gradient (head %d)" % h)
        b = case.plant[h]["equal"]
        if case.mate[h, b] >= 0 and (d[h, b] != 0 or d[h, case.mate[h, b]] != 0):
            rep.bad.append("the bit-equal pair does not store d == 0 (head %d)" % h)
    n_amb = int((want["amb"] & ~case.planted).sum())
    rep.finish(n_amb, quiet)
    return rep.worst, n_amb
