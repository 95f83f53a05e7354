"""GPU: the loss, policy-head and optimiser kernels through the C ABI against float64 on the operands as stored, EVERY stored element, at the
running first-order bound of tests/loss_parity.py: |got - v64| <= err64, an element whose bound is zero bit-equal, everything the headers
say is written overwritten (the buffers start filled with a sentinel) and a guard band beyond it untouched.  Cases, shapes and planted rows:
tests/loss_parity.py (PPO_CASES, BC_CASES, MIX_CASES, AdamCase), the same the fp32 emulation passes on the CPU.  Every case prints one
line per launch: kernel, shape, worst err / bound, ambiguous rows.  What the older tests assert on the same kernels (repeatability,
poison, the KL gate, bit-equality of the variants with each other) is not repeated — except the one optimiser form that no test tied to
a root (cadre_clip_adam_pack_graph_gated)."""
import numpy as np
import pytest
import torch

from tests import loss_parity as lp
from tests.loss_parity import F4, SENT, VE, XVE

pytestmark = pytest.mark.gpu
F_PPO, F_BC = 8, 6
DECOY = 0.77                      # by-value scalars of a launch that must read the hyper-parameter block instead


def dev(x):
    return torch.as_tensor(x).cuda()


@pytest.fixture(scope="module")
def hip():
    from cadre_amd import hip as h
    h.lib()
    return h


def host(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------- one launch of a loss kernel
class Launch:
    """Device operands of a case and fresh sentinel-filled outputs."""

    def __init__(self, hip, c):
        self.hip, self.c = hip, c
        self.nblk = (c.B + 15) // 16
        self.d = {k: dev(getattr(c, k)) for k in ("logits", "values", "actions", "cmds", "old_v", "rets", "old_lp", "adv", "kindrow")}
        self.w = None if c.weights is None else dev(c.weights)
        self.ord = dev(c.ord)
        self.marker = dev(np.full((2, 64), -1, np.int32))
        self.hp_block = self._block()

    def block(self):
        return self.hp_block

    def _block(self):
        h = self.hip
        hp = torch.zeros(h.HP_FIELDS, dtype=torch.float64)
        for k in ("clip", "value_coeff", "clip_coeff", "ent_coeff"):
            hp[h.HP[k]] = float(self.c.hp[k])
        hp[h.HP["lr"]], hp[h.HP["max_grad_norm"]], hp[h.HP["lr_min"]], hp[h.HP["lr_max"]], hp[h.HP["lr_factor"]] = 3e-4, 250.0, 1e-6, 1e-2, 1.5
        hp[h.HP_DEMO_COEFF], hp[h.HP_DEMO_VALUE_COEFF] = float(self.c.hp["demo_coeff"]), float(self.c.hp["demo_value_coeff"])
        return hp.cuda()

    def outputs(self):
        c = self.c
        o = dict(dl=torch.full((c.logits.size,), float(SENT), device="cuda"), dv=torch.full((c.values.size,), float(SENT), device="cuda"),
                 losses=torch.full((8,), float(SENT), device="cuda"), demo_losses=torch.full((8,), float(SENT), device="cuda"),
                 scratch=torch.full((4 + 6 * self.nblk,), 3.0, device="cuda"), stats=torch.zeros(2, F_PPO, device="cuda"),
                 sscratch=torch.zeros(2 * self.nblk * 6, device="cuda"), dstats=torch.zeros(2, F_BC, device="cuda"),
                 dscratch=torch.zeros(2 * self.nblk * 8, device="cuda"))
        o["scratch"][0] = 0.0                                # the arrival counter: zero on first use, reset by every launch
        return o

    def head(self, with_old=True):
        c, d = self.c, self.d
        a = [d["logits"].data_ptr(), c.ldl, c.l_ns, d["values"].data_ptr(), c.ldv, c.v_ns, d["actions"].data_ptr(), d["cmds"].data_ptr()]
        a += [d["old_v"].data_ptr(), d["rets"].data_ptr(), d["old_lp"].data_ptr(), d["adv"].data_ptr()] if with_old else [d["rets"].data_ptr()]
        return a

    def collect(self, o, stats, dstats=False, grad=True):
        torch.cuda.synchronize()
        assert bool((o["losses"][3:] == float(SENT)).all()) and bool((o["demo_losses"][2:] == float(SENT)).all()), "a loss beyond its slot was written"
        assert int(o["scratch"][:1].view(torch.int32)[0].item()) == 0, "the arrival counter was not reset"
        got = dict(dlogits=host(o["dl"]), dvalues=host(o["dv"]), losses=host(o["losses"])[:3], demo_losses=host(o["demo_losses"])[:2])
        if stats:
            got["stats"] = host(o["stats"])
        if dstats:
            got["demo_stats"] = host(o["dstats"])
        return got

    # ---- the entry points
    def ppo(self, entry, o):
        c, L, hp = self.c, self.hip.lib(), self.c.hp
        sizes = [c.B, c.C, c.Ks[0], c.Ks[1]]
        byval = [float(hp[k]) for k in ("clip", "value_coeff", "clip_coeff", "ent_coeff")]
        tail = [float(hp["inv_b"]), o["losses"].data_ptr(), o["dl"].data_ptr(), o["dv"].data_ptr(), o["scratch"].data_ptr(), None]
        st = [o["stats"].data_ptr(), F_PPO, o["sscratch"].data_ptr(), 0.0, None]
        s = self.hip.stream()
        if entry == "cadre_ppo_loss":
            rc = L.cadre_ppo_loss(*self.head(), *sizes, *byval, *tail, s)
        elif entry == "cadre_ppo_loss_stats":
            rc = L.cadre_ppo_loss_stats(*self.head(), *sizes, *byval, *tail, *st, s)
        elif entry == "cadre_ppo_loss_hp":
            rc = L.cadre_ppo_loss_hp(*self.head(), *sizes, self.block().data_ptr(), *tail, s)
        elif entry == "cadre_ppo_loss_stats_hp":
            rc = L.cadre_ppo_loss_stats_hp(*self.head(), *sizes, self.block().data_ptr(), *tail, *st, s)
        else:
            # cadre_ppo_loss_ord[+stats][+hp][+marker]: with the block, the by-value scalars are decoys
            use_hp, use_st = "+hp" in entry, "+stats" in entry
            table = self.marker if "+marker" in entry else self.ord
            rc = L.cadre_ppo_loss_ord(*self.head(), *sizes, self.block().data_ptr() if use_hp else None, *([DECOY] * 4 if use_hp else byval), *tail,
                                      *(st if use_st else [None, 0, None, 0.0, None]), table.data_ptr(), s)
        self.hip.check(rc, entry)
        return self.collect(o, "stats" in entry)

    def bc(self, o, grad, weights, stats, table):
        c, L, hp = self.c, self.hip.lib(), self.c.hp
        rc = L.cadre_bc_loss(*self.head(False), None if not weights else self.w.data_ptr(), c.B, c.C, c.Ks[0], c.Ks[1], float(hp["smoothing"]),
                             float(hp["bc_coeff"]), float(hp["value_coeff"]), float(hp["ent_coeff"]), float(hp["inv_b"]), o["losses"].data_ptr(),
                             o["dl"].data_ptr() if grad else None, o["dv"].data_ptr() if grad else None, o["scratch"].data_ptr(), None,
                             o["dstats"].data_ptr() if stats else None, F_BC, o["sscratch"].data_ptr() if stats else None,
                             None if table is None else table.data_ptr(), self.hip.stream())
        self.hip.check(rc, "cadre_bc_loss")
        return self.collect(o, False, stats)

    def mix(self, o, use_hp, stats, kinds):
        c, L, hp = self.c, self.hip.lib(), self.c.hp
        byval = [float(hp[k]) for k in ("clip", "value_coeff", "clip_coeff", "ent_coeff")]
        demo = [float(hp["demo_coeff"]), float(hp["demo_value_coeff"])]
        head = self.head() + [kinds.data_ptr(), c.B, c.C, c.Ks[0], c.Ks[1]]
        rc = L.cadre_ppo_demo_loss(*head, self.block().data_ptr() if use_hp else None, *([DECOY] * 4 if use_hp else byval), float(hp["inv_b"]),
                                   float(hp["smoothing"]), *([DECOY] * 2 if use_hp else demo), float(hp["inv_bd"]), o["losses"].data_ptr(),
                                   o["demo_losses"].data_ptr(), o["dl"].data_ptr(), o["dv"].data_ptr(), o["scratch"].data_ptr(),
                                   o["dscratch"].data_ptr(), None, o["stats"].data_ptr() if stats else None, F_PPO,
                                   o["sscratch"].data_ptr() if stats else None, 0.0, None, o["dstats"].data_ptr() if stats else None, F_BC,
                                   self.ord.data_ptr() if any(c.ordinal) else None, self.hip.stream())
        self.hip.check(rc, "cadre_ppo_demo_loss")
        return self.collect(o, stats, stats)


# ----------------------------------------------------------------------------- 2. the PPO loss in its five entry points
@pytest.mark.parametrize("i", range(len(lp.PPO_CASES)), ids=lambda i: "B%d-K%s-C%d" % (lp.PPO_CASES[i]["B"], "x".join(map(str, lp.PPO_CASES[i]["Ks"])), lp.PPO_CASES[i]["C"]))
def test_ppo_loss(hip, i):
    c = lp.LossCase(kind="ppo", **lp.PPO_CASES[i])
    ref = lp.run_loss(c, XVE)
    run = Launch(hip, c)
    if any(c.ordinal):
        entries = ["cadre_ppo_loss_ord", "cadre_ppo_loss_ord+stats", "cadre_ppo_loss_ord+hp", "cadre_ppo_loss_ord+stats+hp"]
    else:
        entries = ["cadre_ppo_loss", "cadre_ppo_loss_stats", "cadre_ppo_loss_hp", "cadre_ppo_loss_stats_hp", "cadre_ppo_loss_ord+stats+hp+marker"]
    for entry in entries:
        got = run.ppo(entry, run.outputs())
        _w, n_amb = lp.check_loss(c, got, ref, "%s %s" % (entry, c.tag()), stats="stats" in entry)
        assert n_amb <= 1


# ----------------------------------------------------------------------------- 3. the imitation loss
@pytest.mark.parametrize("i", range(len(lp.BC_CASES)), ids=lambda i: "B%d-K%s-C%d" % (lp.BC_CASES[i]["B"], "x".join(map(str, lp.BC_CASES[i]["Ks"])), lp.BC_CASES[i]["C"]))
def test_bc_loss(hip, i):
    c = lp.LossCase(kind="bc", **lp.BC_CASES[i])
    run = Launch(hip, c)
    table = run.ord if any(c.ordinal) else None                  # ord NULL where both heads are categorical, else given
    refs = {w: lp.run_loss(c, XVE, weights=w) for w in (True, False)}
    #         GRAD   weights stats  ord
    combos = [(True, True, True, table), (True, False, False, table if table is not None else run.marker),
              (False, True, True, table if table is not None else run.marker), (False, False, False, table)]
    for grad, weights, stats, tb in combos:
        o = run.outputs()
        got = run.bc(o, grad, weights, stats, tb)
        what = "cadre_bc_loss GRAD %d weights %d stats %d ord %s %s" % (grad, weights, stats, "NULL" if tb is None else "given", c.tag())
        if not grad:
            assert (got["dlogits"] == SENT).all() and (got["dvalues"] == SENT).all(), what + ": the evaluation form stored a gradient"
        _w, n_amb = lp.check_loss(c, got, refs[weights], what, stats=stats, grad=grad)
        assert n_amb <= 1


# ----------------------------------------------------------------------------- 4. the mixed loss
@pytest.mark.parametrize("i", range(len(lp.MIX_CASES)), ids=lambda i: "B%d-K%s-C%d" % (lp.MIX_CASES[i]["B"], "x".join(map(str, lp.MIX_CASES[i]["Ks"])), lp.MIX_CASES[i]["C"]))
def test_ppo_demo_loss(hip, i):
    c = lp.LossCase(kind="mix", **lp.MIX_CASES[i])
    assert float(c.hp["inv_b"]) != float(c.hp["inv_bd"])
    run = Launch(hip, c)
    # the kinds from cadre_mix_row_kinds on the sorted layout (pos); a case with an empty side then overrides one head
    kinds = torch.full((2, c.B), 9, dtype=torch.int32, device="cuda")
    pos = dev(c.pos)
    hip.check(hip.lib().cadre_mix_row_kinds(pos.data_ptr(), c.B, c.B_ppo, kinds.data_ptr(), hip.stream()), "cadre_mix_row_kinds")
    want = np.zeros((2, c.B), np.int32)
    for h in range(2):
        want[h, c.pos[h, c.B_ppo:]] = 1
    assert np.array_equal(host(kinds), want)
    if not np.array_equal(want, c.kindrow):
        kinds = run.d["kindrow"]
    assert any(c.rows(h, False).size == 0 for h in range(2)) == (lp.MIX_CASES[i].get("empty") == "no_ppo_head0")
    ref = lp.run_loss(c, XVE)
    for use_hp, stats in ((False, True), (True, False), (True, True)):
        got = run.mix(run.outputs(), use_hp, stats, kinds)
        _w, n_amb = lp.check_loss(c, got, ref, "cadre_ppo_demo_loss hp %s stats %d %s" % ("block" if use_hp else "NULL", stats, c.tag()), stats=stats)
        assert n_amb <= 1


# ----------------------------------------------------------------------------- 1. the front
FRONT = [(33, False, 64), (33, True, 40), (3, False, 64), (3, True, 3), (64, False, 64), (64, True, 64), (1, False, 64), (1, True, 8), (2, True, 64)]


@pytest.mark.parametrize("K,ordinal,ldl", FRONT)
def test_front(hip, K, ordinal, ldl):
    L, R = hip.lib(), 48
    r = np.random.RandomState(100 * K + ordinal)
    x = lp.raw_rows(r, R, K, 4.0, ordinal)
    raw = np.full((R, ldl), 3.25, F4)
    raw[:, :K] = x
    table = lp.rank_table(K, ordinal)
    rk = table[:K].astype(np.int64) if ordinal else None
    X, lg, pk, H = lp.front_reference(x, rk)
    raw_d, tb = dev(raw), dev(table)
    tag = "K %d %s ldl %d" % (K, "ordinal" if ordinal else "categorical", ldl)
    n = np.arange(R)
    # ---- categorical_dist: lg and p of every bin, mode
    lo = torch.full((R * K + 16,), float(SENT), device="cuda"); po = torch.full((R * K + 16,), float(SENT), device="cuda")
    mo = torch.full((R + 4,), -5, dtype=torch.int64, device="cuda")
    if ordinal:
        hip.check(L.cadre_categorical_dist_ord(raw_d.data_ptr(), ldl, R, K, lo.data_ptr(), po.data_ptr(), mo.data_ptr(), tb.data_ptr(), hip.stream()), "dist_ord")
    else:
        hip.check(L.cadre_categorical_dist(raw_d.data_ptr(), ldl, R, K, lo.data_ptr(), po.data_ptr(), mo.data_ptr(), hip.stream()), "dist")
    torch.cuda.synchronize()
    rep = lp.Report("cadre_categorical_dist%s %s" % ("_ord" if ordinal else "", tag))
    mask = np.arange(R * K + 16) < R * K
    rep.check("lg", host(lo), VE(np.concatenate([lg.v.reshape(-1), np.zeros(16)]), np.concatenate([lg.e.reshape(-1), np.zeros(16)])), mask, SENT)
    rep.check("p", host(po), VE(np.concatenate([pk.v.reshape(-1), np.zeros(16)]), np.concatenate([pk.e.reshape(-1), np.zeros(16)])), mask, SENT)
    cand = lp.candidates(pk)
    mode = host(mo)
    assert (mode[R:] == -5).all() and ((mode[:R] >= 0) & (mode[:R] < K)).all()
    assert cand[n, mode[:R]].all(), "%s: a mode outside the candidates" % tag
    free = (cand.sum(-1) > 1) & ~(x == x[:, :1]).all(-1)         # (a row of equal logits ties every bin on purpose: the lowest index must win)
    eq = (x == x[:, :1]).all(-1) & (not ordinal)
    assert (mode[:R][eq] == 0).all()
    rep.finish(int(free.sum()))
    assert free.sum() <= 1
    # ---- categorical_eval: logp of given actions, entropy
    a = r.randint(0, K, R).astype(np.int64)
    lpo = torch.full((R + 4,), float(SENT), device="cuda"); en = torch.full((R + 4,), float(SENT), device="cuda")
    a_d = dev(a)
    if ordinal:
        hip.check(L.cadre_categorical_eval_ord(raw_d.data_ptr(), ldl, a_d.data_ptr(), R, K, lpo.data_ptr(), en.data_ptr(), tb.data_ptr(), hip.stream()), "eval_ord")
    else:
        hip.check(L.cadre_categorical_eval(raw_d.data_ptr(), ldl, a_d.data_ptr(), R, K, lpo.data_ptr(), en.data_ptr(), hip.stream()), "eval")
    torch.cuda.synchronize()
    rep = lp.Report("cadre_categorical_eval%s %s" % ("_ord" if ordinal else "", tag))
    m4 = np.arange(R + 4) < R
    pad = lambda t: VE(np.concatenate([t.v, np.zeros(4)]), np.concatenate([t.e, np.zeros(4)]))
    rep.check("logp", host(lpo), pad(lg[n, a]), m4, SENT)
    rep.check("entropy", host(en), pad(H), m4, SENT)
    rep.finish()
    # ---- sample: argmax(p / q) with p renormalised, logp of the chosen bin
    q = r.exponential(1.0, (R, K)).astype(F4) + F4(1e-3)
    q_d = dev(q)
    act = torch.full((R + 4,), -5, dtype=torch.int64, device="cuda"); slp = torch.full((R + 4,), float(SENT), device="cuda")
    if ordinal:
        hip.check(L.cadre_sample_ord(raw_d.data_ptr(), ldl, q_d.data_ptr(), K, R, K, act.data_ptr(), slp.data_ptr(), tb.data_ptr(), hip.stream()), "sample_ord")
    else:
        hip.check(L.cadre_sample(raw_d.data_ptr(), ldl, q_d.data_ptr(), K, R, K, act.data_ptr(), slp.data_ptr(), hip.stream()), "sample")
    torch.cuda.synchronize()
    score = (pk / X.sum(pk)[..., None]) / VE(q)
    cand = lp.candidates(score)
    got_a = host(act)
    assert (got_a[R:] == -5).all() and ((got_a[:R] >= 0) & (got_a[:R] < K)).all()
    assert cand[n, got_a[:R]].all(), "%s: a sampled index outside the candidates" % tag
    sure = cand.sum(-1) == 1
    assert (got_a[:R][sure] == np.argmax(score.v, -1)[sure]).all()
    rep = lp.Report("cadre_sample%s %s" % ("_ord" if ordinal else "", tag))
    rep.check("logp", host(slp), pad(lg[n, got_a[:R]]), m4, SENT)
    rep.finish(int((~sure).sum()))
    assert (~sure).sum() <= 1


# ----------------------------------------------------------------------------- 5. clip + Adam
def _adam_check(case, what, step, got, prev, g, n2_got, rlo=0, rhi=None):
    ref = lp.adam_step(case, XVE, step, prev[0], g, prev[1], prev[2], n2_got, rlo, rhi)
    rep = lp.Report("%s step %d" % (what, step))
    for name, a, b in zip(("params", "exp_avg", "exp_avg_sq"), got, ref):
        rep.check(name, a, b)
    rep.check("norms2", n2_got, lp.norms2_ref(g, case.seg_off, rlo, rhi if rhi is not None else case.n))
    rep.finish()


@pytest.mark.parametrize("entry,kw", [("cadre_clip_adam", dict(seed=71)), ("cadre_clip_adam", dict(seed=72, aligned=False)),
                                      ("cadre_clip_adam", dict(seed=73, warm=True)), ("cadre_clip_adam_graph", dict(seed=71)),
                                      ("cadre_clip_adam_graph", dict(seed=73, warm=True))],
                         ids=lambda v: v if isinstance(v, str) else "-".join("%s%s" % i for i in v.items()))
def test_clip_adam_whole_arena(hip, entry, kw):
    """Every element of params, exp_avg and exp_avg_sq after each of three steps against a float64 Adam step from the fp32 state the kernel
    started the step from, and norms2 against the exact sum of squares.  The padding of an aligned arena and the empty segment move nothing."""
    L, case = hip.lib(), lp.AdamCase(**kw)
    nm = len(case.sizes)
    guard = 8
    bufs = [torch.full((case.n + guard,), float(SENT), device="cuda") for _ in range(3)]
    for b, a in zip(bufs, (case.p0, case.m0, case.v0)):
        b[:case.n] = dev(a)
    nrm = torch.zeros(nm + 2, dtype=torch.float64, device="cuda")
    off, step_dev = dev(case.seg_off), torch.zeros(1, dtype=torch.int32, device="cuda")
    bites = []
    for step in (1, 2, 3):
        g = case.grads[step - 1]
        g_d = dev(g)
        prev = [host(b)[:case.n].copy() for b in bufs]
        ptrs = [b.data_ptr() for b in bufs]
        if entry == "cadre_clip_adam":
            rc = L.cadre_clip_adam(ptrs[0], g_d.data_ptr(), ptrs[1], ptrs[2], off.data_ptr(), nm, nrm.data_ptr(), case.max_norm, lp.ADAM["lr"],
                                   lp.ADAM["beta1"], lp.ADAM["beta2"], lp.ADAM["eps"], step, hip.stream())
        else:
            rc = L.cadre_clip_adam_graph(ptrs[0], g_d.data_ptr(), ptrs[1], ptrs[2], off.data_ptr(), nm, nrm.data_ptr(), case.max_norm, lp.ADAM["lr"],
                                         lp.ADAM["beta1"], lp.ADAM["beta2"], lp.ADAM["eps"], step_dev.data_ptr(), hip.stream())
        hip.check(rc, entry)
        torch.cuda.synchronize()
        assert all(bool((b[case.n:] == float(SENT)).all()) for b in bufs), "the guard band behind the arena was written"
        n2 = host(nrm)[:nm]
        bites += [np.sqrt(x) > case.max_norm for x, n in zip(n2, case.sizes) if n]
        _adam_check(case, "%s %s" % (entry, kw), step, [host(b)[:case.n] for b in bufs], prev, g, n2)
    assert any(bites) and not all(bites)
    assert entry == "cadre_clip_adam" or int(step_dev.item()) == 3


def test_clip_adam_sharded_pair(hip):
    """cadre_clip_adam_norms + cadre_clip_adam_apply on a shard whose bounds cut through the middle of two segments and leave others
    empty, with shard-local moment buffers; the partial norms of the three ranges are summed as the ranks' all-reduce would."""
    L, case = hip.lib(), lp.AdamCase(seed=74, warm=True)
    nm = len(case.sizes)
    rlo, rhi = 500, int(case.seg_off[2]) + 2000                  # inside segment 0 .. inside segment 2; segments 3, 4, 5 hold no element
    assert rlo % 4 == 0 and rhi % 4 == 0 and case.seg_off[2] < rhi < case.seg_off[3]
    p = torch.full((case.n + 8,), float(SENT), device="cuda"); p[:case.n] = dev(case.p0)
    m = torch.full((rhi - rlo + 8,), float(SENT), device="cuda"); m[:rhi - rlo] = dev(case.m0[rlo:rhi])
    v = torch.full((rhi - rlo + 8,), float(SENT), device="cuda"); v[:rhi - rlo] = dev(case.v0[rlo:rhi])
    off = dev(case.seg_off)
    nrm = torch.zeros(nm + 2, dtype=torch.float64, device="cuda")
    other = [torch.zeros(nm + 2, dtype=torch.float64, device="cuda") for _ in range(2)]
    steps = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(3)]
    m_full, v_full = case.m0.copy(), case.v0.copy()
    for step in (1, 2, 3):
        g = case.grads[step - 1]
        g_d = dev(g)
        prev = [host(p)[:case.n].copy(), m_full.copy(), v_full.copy()]
        for buf, sd, (a, b) in zip([nrm] + other, steps, [(rlo, rhi), (0, rlo), (rhi, case.n)]):
            hip.check(L.cadre_clip_adam_norms(g_d.data_ptr(), off.data_ptr(), nm, buf.data_ptr(), lp.ADAM["lr"], lp.ADAM["beta1"], lp.ADAM["beta2"],
                                              sd.data_ptr(), a, b, hip.stream()), "cadre_clip_adam_norms")
        torch.cuda.synchronize()
        rep = lp.Report("cadre_clip_adam_norms shard [%d, %d) step %d" % (rlo, rhi, step))
        for buf, (a, b) in zip([nrm] + other, [(rlo, rhi), (0, rlo), (rhi, case.n)]):
            rep.check("norms2 [%d, %d)" % (a, b), host(buf)[:nm], lp.norms2_ref(g, case.seg_off, a, b))
        rep.finish()
        assert float(host(nrm)[3]) == 0.0 and float(host(nrm)[5]) == 0.0                     # segments outside the shard, the empty segment
        nrm[:nm] += other[0][:nm] + other[1][:nm]                                             # the all-reduce over three ranks
        hip.check(L.cadre_clip_adam_apply(p.data_ptr(), g_d.data_ptr(), m.data_ptr(), v.data_ptr(), off.data_ptr(), nm, nrm.data_ptr(), case.max_norm,
                                          lp.ADAM["beta1"], lp.ADAM["beta2"], lp.ADAM["eps"], rlo, rhi, hip.stream()), "cadre_clip_adam_apply")
        torch.cuda.synchronize()
        assert bool((p[case.n:] == float(SENT)).all()) and bool((m[rhi - rlo:] == float(SENT)).all()) and bool((v[rhi - rlo:] == float(SENT)).all())
        m_full[rlo:rhi], v_full[rlo:rhi] = host(m)[:rhi - rlo], host(v)[:rhi - rlo]
        n2 = host(nrm)[:nm]
        ref = lp.adam_step(case, XVE, step, prev[0], g, prev[1], prev[2], n2, rlo, rhi)
        rep = lp.Report("cadre_clip_adam_apply shard [%d, %d) step %d" % (rlo, rhi, step))
        for name, a, b in zip(("params", "exp_avg", "exp_avg_sq"), (host(p)[:case.n], m_full, v_full), ref):
            rep.check(name, a, b)                                                             # outside the shard: bound zero, untouched
        rep.finish()
        assert int(steps[0].item()) == step


def test_gated_pack_form_is_chained_to_a_root(hip):
    """cadre_clip_adam_pack_graph_gated was tied to its hyper-parameter twin only (tests/test_hyper_gpu.py), and that twin to it: with
    the gate clear it must equal cadre_clip_adam_pack_graph — which tests/test_kernels_gpu.py ties to cadre_clip_adam_graph — bit for bit
    (parameters, both moments, both packed copies, the step count), and with the gate set it must write none of them."""
    from cadre_amd.arena import PPOArena
    L = hip.lib()
    arenas = [PPOArena("cuda:0", 530, {"steer": 33, "throttle": 3}, 4) for _ in range(2)]
    a0 = arenas[0]
    g = torch.Generator(device="cuda").manual_seed(6)
    p0 = torch.randn(a0.total, device="cuda", generator=g) * 0.05
    n_pack = ((a0.D + 15) // 16) * 4 * (a0.DP // 16) * 256
    packs = [torch.zeros(2, a0.Z, n_pack, device="cuda") for _ in range(2)]
    stop = torch.zeros(1, dtype=torch.int32, device="cuda")
    for a in arenas:
        a.params.copy_(p0)
        a.ensure_adam()

    def step(a, wp, gated):
        head = (hip.ptr(a.params), hip.ptr(a.grads), hip.ptr(a.exp_avg), hip.ptr(a.exp_avg_sq), hip.ptr(a.seg_off), 2 * a.Z, hip.ptr(a.norms2),
                250.0, 3e-4, 0.9, 0.999, 1e-8, hip.ptr(a.step_dev), a.Z, a.size_L, a.o_whh, a.H4, a.DP, a.D, hip.ptr(wp[0]), hip.ptr(wp[1]), wp.stride(1))
        if gated:
            hip.check(L.cadre_clip_adam_pack_graph_gated(*head, hip.ptr(stop), hip.stream()), "cadre_clip_adam_pack_graph_gated")
        else:
            hip.check(L.cadre_clip_adam_pack_graph(*head, hip.stream()), "cadre_clip_adam_pack_graph")

    for s in range(2):
        gr = torch.randn(a0.total, device="cuda", generator=g) * (40.0 if s == 1 else 0.3)
        for a in arenas:
            a.grads.copy_(gr)
        step(arenas[0], packs[0], False)
        step(arenas[1], packs[1], True)
        torch.cuda.synchronize()
        for x, y in ((arenas[0].params, arenas[1].params), (arenas[0].exp_avg, arenas[1].exp_avg), (arenas[0].exp_avg_sq, arenas[1].exp_avg_sq),
                     (packs[0], packs[1]), (arenas[0].step_dev, arenas[1].step_dev)):
            assert torch.equal(x, y), s
    stop.fill_(1)
    before = [t.clone() for t in (arenas[1].params, arenas[1].exp_avg, arenas[1].exp_avg_sq, packs[1], arenas[1].step_dev)]
    step(arenas[1], packs[1], True)
    torch.cuda.synchronize()
    for x, y in zip(before, (arenas[1].params, arenas[1].exp_avg, arenas[1].exp_avg_sq, packs[1], arenas[1].step_dev)):
        assert torch.equal(x, y)
    assert float(packs[1].abs().max()) > 0 and int(arenas[1].step_dev.item()) == 2
