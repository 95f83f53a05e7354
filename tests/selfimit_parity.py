"""The running first-order bound of tests/loss_parity.py for cadre_ppo_sil_loss: one launch of the kernel in the arithmetic of X64 / X32 /
XVE (PPO rows through loss_parity.ppo_row, SIL rows through selfimit_ref.sil_row), and the check of every stored element.  The cases are
loss_parity.LossCase(kind="mix") — the rows behind B_ppo in the (sorted) layout are the SIL rows, `rets` their returns R — with rows planted
on R == v (w exactly 0) and R < v.  No new tolerance: the unit constants are loss_parity's.

Plain helper module (no GPU, no fixtures)."""
import numpy as np

from tests import loss_parity as lp
from tests import selfimit_ref as ref
from tests.loss_parity import F4, F8, SENT, VE, X32, XVE, split

SIL_HP = dict(sil_coeff=F4(0.3), sil_value_coeff=F4(0.2))
# B 24 with 12 / 0 / 24 SIL rows and B 300 with 77; bins 33 / 3; C 1 / 4; plain and ordinal heads; pitch 64 and 40.  Seeds: chosen so that
# the float64 pairs alone meet at most one ambiguous row (loss_parity's condition; tests/test_selfimit_cpu.py asserts it).
SIL_CASES = [
    dict(seed=71, B=24, Ks=(33, 3), C=4, ldl=64, scale=1.0, demo_share=0.5),
    dict(seed=72, B=24, Ks=(33, 3), C=1, ldl=40, scale=4.0, demo_share=0.0),
    dict(seed=73, B=24, Ks=(33, 3), C=4, ldl=64, scale=4.0, demo_share=1.0, ordinal=(True, True)),
    dict(seed=74, B=300, Ks=(33, 3), C=4, ldl=64, scale=1.0, demo_share=77.0 / 300.0),
    dict(seed=79, B=300, Ks=(33, 3), C=1, ldl=40, scale=16.0, demo_share=77.0 / 300.0, ordinal=(True, False)),
    dict(seed=76, B=24, Ks=(33, 3), C=4, ldl=64, scale=1.0, demo_share=0.5, ordinal=(False, True)),
]
SIL_ROWS = {24: {0.5: 12, 0.0: 0, 1.0: 24}, 300: {77.0 / 300.0: 77}}


def sil_case(kw):
    """The LossCase of one SIL_CASES entry, with planted SIL rows: the first two countable SIL rows of each head get R == v (w = 0 without
    rounding) and R = v - 1 (R < v)."""
    c = lp.LossCase(kind="mix", **kw)
    assert c.B - c.B_ppo == SIL_ROWS[c.B][kw["demo_share"]]
    c.hp.update(SIL_HP)
    c.hp["inv_bs"] = F4(1.0 / max(1, c.B - c.B_ppo))
    c.zero_rows = [[], []]
    for h in range(2):
        rows = c.rows(h, True)
        for j, b in enumerate(rows[:2]):
            v = c.own_values(h, np.array([b]))[0]
            c.rets[h, b] = v if j == 0 else F4(v - F4(1.0))
            c.zero_rows[h].append(int(b))
    return c


def sil_cases():
    return [sil_case(kw) for kw in SIL_CASES]


def run_sil(case, X, hp=None, stats=True, mut=()):
    """One launch of cadre_ppo_sil_loss in the arithmetic of X -> dict of typed outputs: dlogits / dvalues (flat buffers: SENT where the
    emulation wrote nothing; pairs hold (0, 0) there), sil_w [2][B], losses [3], stats [6] of [2], sil_losses [2], sil_stats [6] of [2]; with
    XVE also `amb` [2][B].  mut: {} or a dict of selfimit_ref.MUTANTS (applied to the SIL rows)."""
    hpv = dict(case.hp)
    hpv.update(hp or {})
    B, C, ldl = case.B, case.C, case.ldl
    pair = X is XVE
    mk = (lambda n: XVE(n)) if pair else (lambda n: X)
    if pair:
        dl, dv, sw = VE(np.zeros(case.logits.size)), VE(np.zeros(case.values.size)), VE(np.zeros((2, B)))
    else:
        dt = X.dtype
        dl, dv, sw = np.full(case.logits.size, SENT, dt), np.full(case.values.size, SENT, dt), np.zeros((2, B), dt)
        for net in range(2 * C):
            for b in range(B):
                dl[net * case.l_ns + b * ldl: net * case.l_ns + (b + 1) * ldl] = 0
                dv[net * case.v_ns + b * case.ldv] = 0
    amb = np.zeros((2, B), bool)
    names_p = ("val", "act", "ent", "kl", "okl", "cf", "vcf", "r", "alr")
    names_s = ("pol", "val", "w", "pos", "nll", "adv", "n")
    zero_t = (lambda: VE(np.zeros((2, B)))) if pair else (lambda: np.zeros((2, B), X.dtype))
    tp, ts = {k: zero_t() for k in names_p}, {k: zero_t() for k in names_s}

    def put(buf, idx, val):
        v, e = split(val)
        if pair:
            buf.v[idx], buf.e[idx] = v, e
        else:
            buf[idx] = v

    for h in range(2):
        K = case.Ks[h]
        for sil in (False, True):
            rows = case.rows(h, sil)
            if rows.size == 0:
                continue
            x_ = mk(rows.size)
            cst = x_.c if pair else (lambda a: np.asarray(a, x_.dtype))
            x, v, a = cst(case.own_logits(h, rows)), cst(case.own_values(h, rows)), case.actions[h, rows]
            if not sil:
                hp5 = (hpv["clip"], hpv["value_coeff"], hpv["clip_coeff"], hpv["ent_coeff"], hpv["inv_b"])
                gk, dval, terms = lp.ppo_row(x_, x, a, v, cst(case.old_v[h, rows]), cst(case.rets[h, rows]), cst(case.old_lp[h, rows]),
                                             cst(case.adv[h, rows]), hp5, case.rk(h), ())
                tdst = tp
            else:
                hp3 = (hpv["sil_coeff"], hpv["sil_value_coeff"], hpv["inv_bs"])
                gk, dval, w, terms = ref.sil_row(x_, x, a, v, cst(case.rets[h, rows]), hp3, case.rk(h), mut)
                put(sw, (h, rows), w)
                tdst = ts
            for k, t in terms.items():
                put(tdst[k], (h, rows), t)
            if pair:
                amb[h, rows] |= x_.amb
            net = h * C + case.cmds[h, rows]
            put(dl, (net * case.l_ns + rows * ldl)[:, None] + np.arange(K)[None, :], gk)
            put(dv, net * case.v_ns + rows * case.ldv, dval)
    out = dict(dlogits=dl, dvalues=dv, sil_w=sw, amb=amb)
    x_ = mk(2)
    c = x_.c if pair else (lambda a: np.asarray(a, x_.dtype))
    red = lambda t, per_head=False, use_max=False: lp.reduce_rows(x_, t, B, per_head, use_max)
    half, ib, ibs = c(0.5), c(hpv["inv_b"]), c(hpv["inv_bs"])
    out["losses"] = [c(hpv["value_coeff"]) * half * red(tp["val"]) * ib, c(hpv["clip_coeff"]) * red(tp["act"]) * ib,
                     c(hpv["ent_coeff"]) * red(tp["ent"]) * ib]
    out["sil_losses"] = [c(hpv["sil_coeff"]) * red(ts["pol"]) * ibs, c(hpv["sil_value_coeff"]) * half * red(ts["val"]) * ibs]
    if stats:
        out["stats"] = [red(tp[k], True) * ib for k in ("kl", "okl", "cf", "vcf", "r")] + [red(tp["alr"], True, True)]
        out["sil_stats"] = [red(ts[k], True) * ibs for k in ("w", "pos", "nll", "adv")] + [red(ts["w"], True, True), red(ts["n"], True)]
    return out


def emulate_sil(case, order="tree", mut=(), **kw):
    """The X32 emulation's outputs in the layout check_sil takes."""
    o = run_sil(case, X32(order), mut=mut, **kw)
    out = dict(dlogits=o["dlogits"], dvalues=o["dvalues"], sil_w=o["sil_w"])
    for name in ("losses", "sil_losses"):
        out[name] = np.array([float(t) for t in o[name]])
    for name in ("stats", "sil_stats"):
        if name in o:
            out[name] = np.stack([np.asarray(t, F8) for t in o[name]], 1)
    return out


def check_sil(case, got, want, what, stats=True, quiet=False):
    """got: dict of arrays as a launch (or the X32 emulation) left them; want: run_sil(case, XVE).  Every stored element of dlogits, dvalues,
    sil_w, the losses and the statistics within the bound; SIL rows with R <= v exact zeros; untouched sentinels still sentinels."""
    rep = lp.Report(what)
    ml, mv = lp.written(case)
    rep.check("dlogits", got["dlogits"], want["dlogits"], ml, SENT)
    rep.check("dvalues", got["dvalues"], want["dvalues"], mv, SENT)
    rep.check("sil_w", got["sil_w"], want["sil_w"])
    for name, n in (("losses", 3), ("sil_losses", 2)):
        v = np.array([split(t)[0] for t in want[name]])
        e = np.array([split(t)[1] for t in want[name]])
        rep.check(name, np.asarray(got[name], F8)[:n], VE(v, e))
    for name in ("stats", "sil_stats"):
        if stats:
            v = np.stack([split(t)[0] for t in want[name]], 1)
            e = np.stack([split(t)[1] for t in want[name]], 1)
            rep.check(name, np.asarray(got[name], F8)[:, :6], VE(v, e))
    # rows with R <= v: w, the value gradient and every logit gradient of the row exactly zero
    for h in range(2):
        rows = case.rows(h, True)
        if rows.size == 0:
            continue
        v, R = case.own_values(h, rows), case.rets[h, rows]
        z = rows[R <= v]
        net = h * case.C + case.cmds[h, z]
        cols = (net * case.l_ns + z * case.ldl)[:, None] + np.arange(case.ldl)[None, :]
        if np.any(np.asarray(got["sil_w"])[h, z] != 0) or np.any(got["dvalues"][net * case.v_ns + z * case.ldv] != 0) or np.any(got["dlogits"][cols] != 0):
            rep.bad.append("a SIL row with R <= v holds a non-zero w or gradient (head %d)" % h)
    n_amb = int((want["amb"] & ~case.planted).sum())
    rep.finish(n_amb, quiet)
    return rep.worst, n_amb


def mutants(case):
    """{name: the mut dict} of selfimit_ref.MUTANTS for a case."""
    return dict(w_unclamped=dict(w_unclamped=1), dval_sign=dict(dval_sign=1), inv_b=dict(inv_b=case.hp["inv_b"]),
                entropy_kept=dict(entropy_kept=F4(case.hp["ent_coeff"]) * F4(case.hp["inv_b"])), w_diff=dict(w_diff=1))
