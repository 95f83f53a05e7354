"""GPU: action masks (csrc/actmask.hip, cadre_amd/actmask.py).

  * all bits set (and words with no bit among K) equal today bit for bit: cadre_ppo_am_loss against cadre_ppo_loss_ord, the two
    samplers and the evaluation against their `_ord` twins;
  * random masks: every stored element of cadre_ppo_am_loss within the running first-order bound of tests/actmask_parity.py;
  * exact zeros: forbidden bins of a categorical head, a row with one allowed bin, the sentinel behind ldl;
  * sampling: allowed actions, greedy, the float64 rule where its margin is decisive, and the sampler's logp fed back as old_logp;
  * cadre_allowed_note / cadre_allowed_rows against their numpy statements;
  * through the agent, through an update and through train_vec."""
import functools

import numpy as np
import pytest
import torch

from tests import actmask_parity as ap
from tests import actmask_ref as ar
from tests import loss_parity as lp
from tests.loss_parity import F4, F8, SENT, XVE

pytestmark = pytest.mark.gpu
F_PPO, F_AM = 8, 4
DECOY = 0.77
GUARD = 8
MODES = ((False, True), (True, False), (True, True), (False, False))        # (hp block, stats row)
GRID = [(B, C, Ks, o) for B in ap.SHAPES_B for C in ap.SHAPES_C for Ks in ap.HEADS for o in (False, True)]
GRID_ID = lambda g: "B%d-C%d-K%dx%d-%s" % (g[0], g[1], g[2][0], g[2][1], "ord" if g[3] else "cat")


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@pytest.fixture(scope="module")
def hip():
    from cadre_amd import hip as h
    h.lib()
    return h


@functools.lru_cache(maxsize=None)
def am_case(B, C, Ks, ordinal, words="random"):
    return ap.AmCase(1000 + 7 * B + C + Ks[0], B, Ks, C, (ordinal, ordinal), words)


class AmLaunch:
    """Device operands of an AmCase and fresh sentinel-filled outputs."""

    def __init__(self, hip, case):
        self.hip, self.case, c = hip, case, case
        self.nblk = (c.B + 15) // 16
        self.d = {k: dev(getattr(c, k)) for k in ("logits", "values", "actions", "cmds", "old_v", "rets", "old_lp", "adv", "allowed")}
        self.ord = dev(c.ord)
        hp = torch.zeros(hip.HP_FIELDS, dtype=torch.float64)
        for k in ("clip", "value_coeff", "clip_coeff", "ent_coeff"):
            hp[hip.HP[k]] = float(c.hp[k])
        hp[hip.HP["lr"]], hp[hip.HP["max_grad_norm"]], hp[hip.HP["lr_min"]], hp[hip.HP["lr_max"]], hp[hip.HP["lr_factor"]] = 3e-4, 250.0, 1e-6, 1e-2, 1.5
        self.block = hp.cuda()

    def outputs(self):
        c = self.case
        f = lambda n, v=float(SENT): torch.full((n,), v, device="cuda")
        o = dict(dl=f(c.logits.size), dv=f(c.values.size), losses=f(8), scratch=f(4 + 6 * self.nblk, 3.0),
                 stats=torch.zeros(2, F_PPO, device="cuda"), sscratch=torch.zeros(2 * self.nblk * 6, device="cuda"),
                 am_stats=f(2 * F_AM + GUARD), am_scratch=f(2 * self.nblk * 5 + GUARD, 11.0))          # (needs no initialisation)
        o["scratch"][0] = 0.0
        return o

    def head(self, old_lp=None):
        c, d = self.case, self.d
        return [d["logits"].data_ptr(), c.ldl, c.l_ns, d["values"].data_ptr(), c.ldv, c.v_ns, d["actions"].data_ptr(), d["cmds"].data_ptr(),
                d["old_v"].data_ptr(), d["rets"].data_ptr(), (d["old_lp"] if old_lp is None else old_lp).data_ptr(), d["adv"].data_ptr()]

    def tail(self, o, use_hp, stats, hp_over=None):
        c = self.case
        hp = dict(c.hp, **(hp_over or {}))
        byval = [float(hp[k]) for k in ("clip", "value_coeff", "clip_coeff", "ent_coeff")]
        return [c.B, c.C, c.Ks[0], c.Ks[1], self.block.data_ptr() if use_hp else None, *([DECOY] * 4 if use_hp else byval),
                float(hp["inv_b"]), o["losses"].data_ptr(), o["dl"].data_ptr(), o["dv"].data_ptr(), o["scratch"].data_ptr(), None,
                o["stats"].data_ptr() if stats else None, F_PPO, o["sscratch"].data_ptr() if stats else None, 0.0, None,
                self.ord.data_ptr()]

    def am(self, o, use_hp, stats, allowed=None, am_stats=True, hp_over=None, old_lp=None):
        al = self.d["allowed"] if allowed is None else allowed
        rc = self.hip.lib().cadre_ppo_am_loss(*self.head(old_lp), *self.tail(o, use_hp, stats, hp_over), al.data_ptr(),
                                              o["am_stats"].data_ptr() if am_stats else None, F_AM,
                                              o["am_scratch"].data_ptr() if am_stats else None, self.hip.stream())
        self.hip.check(rc, "cadre_ppo_am_loss")
        return self.collect(o, stats)

    def ord_loss(self, o, use_hp, stats, hp_over=None):
        rc = self.hip.lib().cadre_ppo_loss_ord(*self.head(), *self.tail(o, use_hp, stats, hp_over), self.hip.stream())
        self.hip.check(rc, "cadre_ppo_loss_ord")
        return self.collect(o, stats)

    def collect(self, o, stats):
        torch.cuda.synchronize()
        assert bool((o["losses"][3:] == float(SENT)).all()), "a loss beyond its slot was written"
        assert bool((o["am_stats"][2 * F_AM:] == float(SENT)).all()) and bool((o["am_scratch"][2 * self.nblk * 5:] == 11.0).all())
        assert int(o["scratch"][:1].view(torch.int32)[0].item()) == 0, "the arrival counter was not reset"
        got = dict(dlogits=host(o["dl"]), dvalues=host(o["dv"]), losses=host(o["losses"])[:3],
                   am_stats=host(o["am_stats"])[:2 * F_AM].reshape(2, F_AM))
        if stats:
            got["stats"] = host(o["stats"])
        return got


# ----------------------------------------------------------------------------- 1. all bits set equals today, bit for bit
@pytest.mark.parametrize("g", GRID, ids=GRID_ID)
def test_all_bits_set_is_the_ppo_loss(hip, g):
    for words in ("all", "empty"):
        case = am_case(*g, words=words)
        run = AmLaunch(hip, case)
        for use_hp, stats in MODES:
            want = run.ord_loss(run.outputs(), use_hp, stats)
            for am_stats in (True, False):
                got = run.am(run.outputs(), use_hp, stats, am_stats=am_stats)
                for k in ("dlogits", "dvalues", "losses") + (("stats",) if stats else ()):
                    assert np.array_equal(bits(got[k]), bits(want[k])), (words, use_hp, stats, k)
            am = run.am(run.outputs(), use_hp, stats)["am_stats"]
            for h in (0, 1):
                assert am[h, 0] == 0.0 and am[h, 2] == 0.0 and am[h, 3] == 0.0
                assert am[h, 1] == (float(case.Ks[h]) if len(case.rows(h, None)) else 0.0)


def test_stop_flag_and_gate_equal_the_ppo_loss(hip):
    """target_kl armed: the sticky flag and `applied` come out as from cadre_ppo_loss_ord on the same inputs."""
    case = am_case(17, 4, (33, 3), False, words="all")
    run = AmLaunch(hip, case)
    res = []
    for name in ("ord", "am"):
        o = run.outputs()
        stop = torch.zeros(1, dtype=torch.int32, device="cuda")
        tail = run.tail(o, False, True)
        tail[-3], tail[-2] = 1e-6, stop.data_ptr()                     # target_kl, stop
        L = hip.lib()
        if name == "ord":
            hip.check(L.cadre_ppo_loss_ord(*run.head(), *tail, hip.stream()), name)
        else:
            hip.check(L.cadre_ppo_am_loss(*run.head(), *tail, run.d["allowed"].data_ptr(), None, 0, None, hip.stream()), name)
        torch.cuda.synchronize()
        res.append((int(stop.item()), host(o["stats"]).copy()))
    assert res[0][0] == res[1][0] == 1
    assert np.array_equal(bits(res[0][1]), bits(res[1][1])) and res[1][1][0, 6] == 0.0


class Rows:
    """R rows of one head for the samplers: raw logits [R][ldl], q, words, the rank table."""

    def __init__(self, K, ordinal, R=4096, seed=0, words="random", greedy=False):
        r = np.random.RandomState(50 + K + seed)
        self.K, self.R, self.ldl = K, R, 64
        self.raw = np.full((R, 64), 3.25, F4)
        self.raw[:, :K] = (2.0 * r.standard_normal((R, K))).astype(F4)
        self.q = np.ones((R, 64), F4)
        if not greedy:
            self.q[:, :K] = r.exponential(1.0, (R, K)).astype(F4)
        self.words = ap.random_words(r, R, K)
        if words == "all":
            self.words = np.full(R, ar.all_word(K), np.uint64).view(np.int64)
        self.ord = lp.rank_table(K, ordinal)
        self.rank = self.ord[:K].astype(np.int64) if ordinal else None

    def launch(self, hip, masked=True):
        raw, q, w, o = dev(self.raw), dev(self.q), dev(self.words), dev(self.ord)
        act = torch.full((self.R + GUARD,), -3, dtype=torch.int64, device="cuda")
        logp = torch.full((self.R + GUARD,), float(SENT), device="cuda")
        L = hip.lib()
        if masked:
            hip.check(L.cadre_sample_am(raw.data_ptr(), 64, q.data_ptr(), 64, self.R, self.K, act.data_ptr(), logp.data_ptr(),
                                        o.data_ptr(), w.data_ptr(), hip.stream()), "cadre_sample_am")
        else:
            hip.check(L.cadre_sample_ord(raw.data_ptr(), 64, q.data_ptr(), 64, self.R, self.K, act.data_ptr(), logp.data_ptr(),
                                         o.data_ptr(), hip.stream()), "cadre_sample_ord")
        torch.cuda.synchronize()
        assert bool((act[self.R:] == -3).all()) and bool((logp[self.R:] == float(SENT)).all())
        return host(act)[:self.R], host(logp)[:self.R]


@pytest.mark.parametrize("ordinal", [False, True], ids=["cat", "ord"])
@pytest.mark.parametrize("K", [1, 3, 33, 64])
def test_samplers_with_all_bits_set_equal_the_ord_twins(hip, K, ordinal):
    rows = Rows(K, ordinal, R=67, words="all")
    a0, l0 = rows.launch(hip, masked=False)
    a1, l1 = rows.launch(hip, masked=True)
    assert np.array_equal(a0, a1) and np.array_equal(bits(l0), bits(l1))
    rows.words = np.zeros(rows.R, np.int64) if K == 64 else np.full(rows.R, -1 << K, np.int64)      # no bit among K: unmasked
    a2, l2 = rows.launch(hip, masked=True)
    assert np.array_equal(a0, a2) and np.array_equal(bits(l0), bits(l2))
    # evaluation: the twin's logp / entropy bits
    raw, act, o, w = dev(rows.raw), dev(a0.astype(np.int64)), dev(rows.ord), dev(rows.words)
    out = [torch.full((rows.R,), float(SENT), device="cuda") for _ in range(4)]
    L = hip.lib()
    hip.check(L.cadre_categorical_eval_ord(raw.data_ptr(), 64, act.data_ptr(), rows.R, K, out[0].data_ptr(), out[1].data_ptr(),
                                           o.data_ptr(), hip.stream()), "cadre_categorical_eval_ord")
    hip.check(L.cadre_categorical_eval_am(raw.data_ptr(), 64, act.data_ptr(), rows.R, K, out[2].data_ptr(), out[3].data_ptr(),
                                          o.data_ptr(), w.data_ptr(), hip.stream()), "cadre_categorical_eval_am")
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[2]) and torch.equal(out[1], out[3]) and np.array_equal(bits(host(out[0])), bits(l0))


def sample_rows_operands(N, C, Ks, ordinal, seed, words="random"):
    r = np.random.RandomState(seed)
    ldo, Z = 64, 4 * C
    O3 = (2.0 * r.standard_normal((Z, N, ldo))).astype(F4)
    cmd = r.randint(0, C, N).astype(np.int32)
    pos = r.permutation(N).astype(np.int32)
    q = np.ones((N, 2, 64), F4)
    q[:, 0, :Ks[0]] = r.exponential(1.0, (N, Ks[0]))
    q[:, 1, :Ks[1]] = r.exponential(1.0, (N, Ks[1]))
    w = np.stack([ap.random_words(r, N, K) for K in Ks], 1)
    if words == "all":
        w = np.stack([np.full(N, ar.all_word(K), np.uint64).view(np.int64) for K in Ks], 1)
    o = np.stack([lp.rank_table(K, ordinal) for K in Ks])
    return O3, cmd, pos, q, np.ascontiguousarray(w), o


def launch_sample_rows(hip, ops, N, C, Ks, masked):
    O3, cmd, pos, q, w, o = (dev(t) for t in ops)
    act = torch.full((N, 2), -3, dtype=torch.int64, device="cuda")
    logp, val = torch.full((N, 2), float(SENT), device="cuda"), torch.full((N, 2), float(SENT), device="cuda")
    L = hip.lib()
    args = [O3.data_ptr(), O3.stride(1), O3.stride(0), pos.data_ptr(), cmd.data_ptr(), N, C, q.data_ptr(), Ks[0], Ks[1], act.data_ptr(),
            logp.data_ptr(), val.data_ptr(), o.data_ptr()]
    if masked:
        hip.check(L.cadre_sample_rows_am(*args, w.data_ptr(), hip.stream()), "cadre_sample_rows_am")
    else:
        hip.check(L.cadre_sample_rows_ord(*args, hip.stream()), "cadre_sample_rows_ord")
    torch.cuda.synchronize()
    return host(act), host(logp), host(val)


@pytest.mark.parametrize("ordinal", [False, True], ids=["cat", "ord"])
@pytest.mark.parametrize("N,C,Ks", [(1, 1, (33, 3)), (5, 4, (33, 3)), (3, 4, (64, 1))])
def test_sample_rows_am(hip, N, C, Ks, ordinal):
    ops = sample_rows_operands(N, C, Ks, ordinal, 11 * N + C, words="all")
    want = launch_sample_rows(hip, ops, N, C, Ks, masked=False)
    got = launch_sample_rows(hip, ops, N, C, Ks, masked=True)
    assert np.array_equal(want[0], got[0]) and np.array_equal(bits(want[1]), bits(got[1])) and np.array_equal(bits(want[2]), bits(got[2]))
    # random words: the per-row sampler on the same row gives the same bits (one statement of the rule), and the action is allowed
    ops = sample_rows_operands(N, C, Ks, ordinal, 13 * N + C)
    O3, cmd, pos, q, w, o = ops
    act, logp, val = launch_sample_rows(hip, ops, N, C, Ks, masked=True)
    for h in (0, 1):
        rows = Rows(Ks[h], ordinal, R=N)
        rows.raw = np.ascontiguousarray(O3[2 * (h * C + cmd), pos])
        rows.q, rows.words = np.ascontiguousarray(q[:, h]), np.ascontiguousarray(w[:, h])
        a1, l1 = rows.launch(hip)
        assert np.array_equal(a1, act[:, h]) and np.array_equal(bits(l1), bits(logp[:, h]))
        assert ar.bits(ar.effective(w[:, h], Ks[h])[0], Ks[h])[np.arange(N), act[:, h]].all()
        assert np.array_equal(bits(val[:, h]), bits(O3[2 * (h * C + cmd) + 1, pos, 0]))


# ----------------------------------------------------------------------------- 2. random masks: element-wise parity
@pytest.mark.parametrize("g", GRID, ids=GRID_ID)
def test_ppo_am_loss_within_the_bound(hip, g):
    case = am_case(*g)
    ref = ap.run_am(case, XVE)
    run = AmLaunch(hip, case)
    first = None
    for use_hp, stats in MODES:
        got = run.am(run.outputs(), use_hp, stats)
        what = "cadre_ppo_am_loss hp %s stats %d %s" % ("block" if use_hp else "NULL", stats, case.tag())
        ap.check_am(case, got, ref, what, stats=stats)
        if first is None:
            first = got
        for k in ("dlogits", "dvalues", "losses", "am_stats"):           # the four forms and a second launch: equal bits
            assert np.array_equal(bits(got[k]), bits(first[k])), (what, k)
    assert first["am_stats"][:, 3].sum() == 0                             # the action was drawn among the allowed bins
    if case.B > 1 and case.Ks[1] > 1:
        assert first["am_stats"][:, 0].max() > 0 and first["am_stats"][:, 2].max() > 0


def test_foreign_action_bit_is_ored_in(hip):
    """Rows whose action the word forbids: the bit is OR-ed in, the outputs stay finite and within the bound, the count says how many."""
    base = am_case(17, 4, (33, 3), False)
    case = ap.AmCase(base.seed, 17, (33, 3), 4, (False, False))
    n = [0, 0]
    for h in (0, 1):
        on = ar.bits(ar.effective(case.allowed[h], case.Ks[h])[0], case.Ks[h])
        for b in range(0, 17, 3):
            off = np.flatnonzero(~on[b])
            if off.size and case.row_ok(h, b):
                case.actions[h, b] = off[0]
                n[h] += 1
    assert min(n) >= 1
    got = AmLaunch(hip, case).am(AmLaunch(hip, case).outputs(), False, True)
    ap.check_am(case, got, ap.run_am(case, XVE), "foreign actions " + case.tag())
    assert got["am_stats"][:, 3].tolist() == [float(n[0]), float(n[1])]


# ----------------------------------------------------------------------------- 3. exact zeros
@pytest.mark.parametrize("B,C", [(17, 4), (67, 1)])
def test_forbidden_bins_get_exact_zeros(hip, B, C):
    case = am_case(B, C, (33, 3), False)
    got = AmLaunch(hip, case).am(AmLaunch(hip, case).outputs(), False, True)
    dl = got["dlogits"]
    n_zero = n_live = 0
    for h in (0, 1):
        K = case.Ks[h]
        on = ar.bits(ar.effective(case.allowed[h], K, case.actions[h])[0], K)
        for b in case.rows(h, None):
            base = (h * C + case.cmds[h, b]) * case.l_ns + b * case.ldl
            row = dl[base: base + case.ldl]
            assert (row[:K][~on[b]] == 0.0).all() and (row[K:] == 0.0).all()
            n_zero += int((~on[b]).sum())
            n_live += int((row[:K][on[b]] != 0.0).sum())
    assert n_zero > 0 and n_live > 0
    ml, _mv = lp.written(case)
    assert (dl[~ml] == F4(SENT)).all()                                     # behind ldl and between the nets: untouched


@pytest.mark.parametrize("ordinal", [False, True], ids=["cat", "ord"])
def test_one_allowed_bin(hip, ordinal):
    """logp == 0, entropy 0, ratio 1 (old_logp = 0) and an all-zero dlogits row."""
    case = am_case(17, 4, (33, 3), ordinal, words="single")
    assert not case.old_lp.any()
    run = AmLaunch(hip, case)
    got = run.am(run.outputs(), False, True)
    for h in (0, 1):
        for b in case.rows(h, None):
            base = (h * case.C + case.cmds[h, b]) * case.l_ns + b * case.ldl
            assert (got["dlogits"][base: base + case.ldl] == 0.0).all()
    assert got["losses"][2] == 0.0                                         # entropy
    st = got["stats"]
    n_ok = np.array([len(case.rows(h, None)) for h in (0, 1)], F8)
    assert (st[:, 0] == 0.0).all() and (st[:, 1] == 0.0).all() and (st[:, 5] == 0.0).all()           # kl, -log r, max |log r|
    assert np.allclose(st[:, 4], n_ok / case.B, rtol=1e-6, atol=0)         # mean ratio: one per counted row
    raw = dev(np.ascontiguousarray(case.dense()[0][0].astype(F4)))         # the evaluation kernel on net 0's rows: logp 0, entropy 0
    act, w, o = dev(case.actions[0]), dev(case.allowed[0]), dev(case.ord[0])
    lpo, en = torch.full((case.B,), 1.0, device="cuda"), torch.full((case.B,), 1.0, device="cuda")
    hip.check(hip.lib().cadre_categorical_eval_am(raw.data_ptr(), case.ldl, act.data_ptr(), case.B, case.Ks[0], lpo.data_ptr(), en.data_ptr(),
                                                  o.data_ptr(), w.data_ptr(), hip.stream()), "cadre_categorical_eval_am")
    assert bool((lpo == 0.0).all()) and bool((en == 0.0).all())


# ----------------------------------------------------------------------------- 4. sampling
@pytest.mark.parametrize("ordinal", [False, True], ids=["cat", "ord"])
@pytest.mark.parametrize("K", [3, 33, 64])
def test_sampling_under_random_masks(hip, K, ordinal):
    rows = Rows(K, ordinal)
    act, logp = rows.launch(hip)
    on = ar.bits(ar.effective(rows.words, K)[0], K)
    assert on[np.arange(rows.R), act].all(), "a forbidden action was sampled"
    want, lp64, margin = ar.sample(rows.raw, rows.q, rows.words, K, rows.rank)
    decided = margin >= 1e-4
    print("K %d %s: %d of %d rows left out by the margin" % (K, "ord" if ordinal else "cat", int((~decided).sum()), rows.R))
    assert (~decided).sum() <= 0.01 * rows.R
    assert np.array_equal(act[decided], want[decided])
    assert np.abs(logp[decided] - lp64[decided]).max() < 1e-4
    # greedy: q all ones -> the first largest allowed probability
    g = Rows(K, ordinal, greedy=True)
    ga, _gl = g.launch(hip)
    gw, _l, gm = ar.sample(g.raw, g.q, g.words, K, g.rank)
    assert np.array_equal(ga[gm >= 1e-4], gw[gm >= 1e-4]) and (gm < 1e-4).sum() <= 0.01 * g.R
    assert ar.bits(ar.effective(g.words, K)[0], K)[np.arange(g.R), ga].all()


@pytest.mark.parametrize("ordinal", [False, True], ids=["cat", "ord"])
def test_sampler_logp_fed_back_gives_ratio_one(hip, ordinal):
    """cadre_sample_am's logp as old_logp at unchanged logits: approx-KL exactly 0 and max |log r| exactly 0 in the stats row."""
    case = ap.AmCase(77, 67, (33, 3), 1, (ordinal, ordinal))
    case.cmds[:] = 0
    run = AmLaunch(hip, case)
    old = torch.zeros(2, case.B, device="cuda")
    acts = torch.zeros(2, case.B, dtype=torch.int64, device="cuda")
    r = np.random.RandomState(5)
    logits_d = run.d["logits"]
    for h in (0, 1):
        K = case.Ks[h]
        q = dev(np.concatenate([r.exponential(1.0, (case.B, K)), np.ones((case.B, 64 - K))], 1).astype(F4))
        o = dev(case.ord[h])
        hip.check(hip.lib().cadre_sample_am(logits_d[h * case.l_ns:].data_ptr(), case.ldl, q.data_ptr(), 64, case.B, K, acts[h].data_ptr(),
                                            old[h].data_ptr(), o.data_ptr(), run.d["allowed"][h].data_ptr(), hip.stream()), "cadre_sample_am")
    run.d["actions"] = acts
    got = run.am(run.outputs(), False, True, old_lp=old)
    st = got["stats"]
    assert (st[:, 0] == 0.0).all() and (st[:, 5] == 0.0).all() and np.allclose(st[:, 4], 1.0, rtol=1e-6, atol=0)
    assert got["am_stats"][:, 3].sum() == 0


# ----------------------------------------------------------------------------- 5. cadre_allowed_note / cadre_allowed_rows
@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("cursor", [0, 8])
def test_allowed_note(hip, N, cursor):
    T = 8
    r = np.random.RandomState(N + cursor)
    tens = [torch.full((T + 1 + GUARD,), -9, dtype=torch.int64, device="cuda") for _ in range(2 * N)]
    want = [np.full(T + 1, -9, np.int64) for _ in range(2 * N)]
    table = [t.data_ptr() for t in tens]
    table[1], want[1] = 0, None                                            # a storage without the tensor
    slots = np.full(2 * N, cursor, np.int32)
    slots[2], slots[3] = T + 1, -1                                         # out of range: nothing is written
    words = r.randint(-2 ** 63, 2 ** 63 - 1, 2 * N, dtype=np.int64)
    words[0] = -2 ** 63                                                    # bit 63 alone
    ar.note(want, slots, words, T)
    t_d, s_d, w_d = dev(np.array(table, np.int64)), dev(slots), dev(words)
    hip.check(hip.lib().cadre_allowed_note(t_d.data_ptr(), s_d.data_ptr(), w_d.data_ptr(), 2 * N, T, hip.stream()), "cadre_allowed_note")
    torch.cuda.synchronize()
    for k in range(2 * N):
        got = host(tens[k])
        assert (got[T + 1:] == -9).all()
        if k == 1:
            assert (got == -9).all()
        else:
            assert np.array_equal(got[:T + 1], want[k]), k
    assert host(tens[0])[cursor] == -2 ** 63


@pytest.mark.parametrize("nW", [2, 3])
@pytest.mark.parametrize("sorted_pos", [True, False])
def test_allowed_rows(hip, nW, sorted_pos):
    T, Bw, C = 8, 4, 4
    n_src, Bt = 2 * nW, nW * 4
    r = np.random.RandomState(3 * nW + sorted_pos)
    srcs = [r.randint(-2 ** 63, 2 ** 63 - 1, T + 1, dtype=np.int64) for _ in range(n_src)]
    srcs[3] = None                                                         # a storage without words among the sources
    idx = np.stack([r.permutation(T)[:Bw] for _ in range(n_src)]).astype(np.int64)
    idx[0, 1], idx[1, 2] = T, -1                                           # out-of-range indices: nothing is written
    pos = None
    if sorted_pos:                                                         # the update's own sort
        cmds = dev(r.randint(0, C, (2, Bt)).astype(np.int32))
        pos_d = torch.zeros(2, Bt, dtype=torch.int32, device="cuda")
        seg_d = torch.zeros(2 * C, 2, dtype=torch.int32, device="cuda")
        hip.check(hip.lib().cadre_sort_rows_by_command(cmds.data_ptr(), Bt, C, pos_d.data_ptr(), seg_d.data_ptr(), hip.stream()),
                  "cadre_sort_rows_by_command")
        pos = host(pos_d)
        assert all(sorted(pos[h].tolist()) == list(range(Bt)) for h in (0, 1))
    init = np.full((2, Bt), -9, np.int64)
    want = ar.place_words(srcs, idx, pos, Bt, T, init)
    keep = [None if s is None else dev(s) for s in srcs]
    table = dev(np.array([0 if k is None else k.data_ptr() for k in keep], np.int64))
    out = torch.full((2 * Bt + GUARD,), -9, dtype=torch.int64, device="cuda")
    idx_d = dev(idx)
    hip.check(hip.lib().cadre_allowed_rows(table.data_ptr(), n_src, idx_d.data_ptr(), Bw, T, pos_d.data_ptr() if sorted_pos else None, Bt,
                                           out.data_ptr(), hip.stream()), "cadre_allowed_rows")
    got = host(out)
    assert np.array_equal(got[:2 * Bt].reshape(2, Bt), want) and (got[2 * Bt:] == -9).all()
    assert (want == -9).any() and (want == 0).any() and (np.abs(want) > 9).any()


# ----------------------------------------------------------------------------- 6. through the agent
ALL33, ALL3 = ar.all_word(33), ar.all_word(3)


def agent_words(N, seed):
    """Per environment a (steer, throttle) pair of Python-int words: random steer bins, the throttle head without its last bin on even
    environments and without its first on odd ones."""
    r = np.random.RandomState(seed)
    out = []
    for e in range(N):
        steer = int(ar.to_u64(ap.random_words(r, 1, 33))[0]) & ALL33
        out.append((steer, 0b011 if e % 2 == 0 else 0b110))
    return out


@pytest.mark.parametrize("N", [1, 3])
def test_act_batch_with_allowed(hip, N):
    from ppo_agent.storage import RolloutStorage
    from tests.test_act_batch_gpu import build_agent, env_streams, obs_of, rel
    T = 3
    streams, _ = env_streams(N, 84, 84, 4, T)
    plain, full, masked, single = (build_agent(84, 84) for _ in range(4))
    st = [(RolloutStorage(4, 1, 530, 8, 530, True, 0.99, 0.95, device="cuda:0"), RolloutStorage(4, 1, 530, 8, 530, True, 0.99, 0.95, device="cuda:0"))
          for _ in range(N)]
    bare = RolloutStorage(4, 1, 530, 8, 530, True, 0.99, 0.95, device="cuda:0")
    assert not hasattr(bare, "allowed")
    want_words = [[[], []] for _ in range(N)]
    for t in range(T):
        obs = lambda: [obs_of(streams[e][t]) for e in range(N)]
        torch.manual_seed(40 + t)
        n0 = hip.N_CALLS
        a = plain.act_batch(obs())                                           # allowed=None: today's launches
        calls = hip.N_CALLS - n0
        rng = torch.rand(1).item()
        torch.manual_seed(40 + t)
        n0 = hip.N_CALLS
        b = full.act_batch(obs(), allowed=[(ALL33, ALL3)] * N)               # every bin allowed: the same bits, the same draws
        assert hip.N_CALLS - n0 == calls and torch.rand(1).item() == rng
        assert torch.equal(a.action, b.action) and torch.equal(a.logp, b.logp) and torch.equal(a.value, b.value) and torch.equal(a.feat, b.feat)
        assert not hasattr(a, "allowed")
        words = agent_words(N, 7 * t + N)
        torch.manual_seed(40 + t)
        c = masked.act_batch(obs(), allowed=words if t % 2 == 0 else
                             torch.tensor([[ar.to_i64([s])[0], ar.to_i64([w])[0]] for s, w in words], dtype=torch.int64).cuda())
        assert torch.rand(1).item() == rng                                   # q is drawn for all K bins
        act = host(c.action)
        for e in range(N):
            assert (words[e][0] >> int(act[e, 0])) & 1 and (words[e][1] >> int(act[e, 1])) & 1, (t, e, act[e])
            for h in (0, 1):
                want_words[e][h].append(ar.to_i64([words[e][h]])[0])
        assert bool((c.logp <= 0).all()) and bool(torch.isfinite(c.logp).all())
        RolloutStorage.insert_batch(st, c, [[0.5, 0.25]] * N, [[1.0, 1.0]] * N, [int(o["command"]) for o in obs()], allowed=c.allowed)
        # environment 0 alone under the same word and the same draws (it draws first): the bits of its row do not depend on the batch
        torch.manual_seed(40 + t)
        d = single.act_batch(obs()[:1], allowed=words[:1])
        for k in ("action", "logp", "value", "feat", "allowed"):
            assert torch.equal(getattr(d, k)[0], getattr(c, k)[0]), (t, k)
    torch.cuda.synchronize()
    for e in range(N):
        for h in (0, 1):
            assert st[e][h].allowed.dtype == torch.int64 and host(st[e][h].allowed)[:T].tolist() == want_words[e][h]
            acts = host(st[e][h].action)[:T, 0]
            assert all((ar.to_u64([w])[0] >> np.uint64(a_)) & np.uint64(1) for w, a_ in zip(want_words[e][h], acts))
    with pytest.raises(ValueError, match="allows none"):
        masked.act_batch([obs_of(streams[e][0]) for e in range(N)], allowed=[(ALL33, 0b1000)] * N)
    with pytest.raises(ValueError, match="allowed"):
        masked.act_batch([obs_of(streams[e][0]) for e in range(N)], allowed=[(ALL33, ALL3)] * (N + 1))
    with pytest.raises(ValueError, match="ensemble"):
        masked.ensemble_act_batch([masked], [obs_of(streams[0][0])], allowed=[(ALL33, ALL3)])
    from ppo_agent.evaluate import EnsembleEvaluator
    ev = object.__new__(EnsembleEvaluator)                                     # (refused before the evaluator is looked at)
    with pytest.raises(ValueError, match="ensemble evaluation takes no allowed"):
        ev.act([obs_of(streams[0][0])], allowed=[(ALL33, ALL3)])
    with pytest.raises(ValueError, match="allows none"):                       # a word without a bit among the head's bins, through insert
        RolloutStorage.insert_batch(st, c, [[0.5, 0.25]] * N, [[1.0, 1.0]] * N, [0] * N, allowed=[(ALL33, 0b1000)] * N, n_out=(33, 3))
    with pytest.raises(ValueError, match="allows none"):
        bare.insert(torch.zeros(8, 530, device="cuda"), torch.zeros(1), torch.zeros(1), torch.zeros(1), 0.0, torch.ones(1), None, 0,
                    allowed=0b1000, allowed_bins=3)
    assert not hasattr(bare, "allowed") and st[0][0].step == T


def test_row_bits_do_not_depend_on_the_batch(hip):
    """The same observation under the same word in batches of 1, 3 and 6 environments, at positions 0, 1 and 2, beside companions with
    other commands and words: action, log-probability, value and feature rows are equal bit for bit (greedy, so that the row's q does not
    depend on its position in the draw order)."""
    from tests.test_act_batch_gpu import build_agent, env_streams, obs_of
    streams, _ = env_streams(6, 84, 84, 4, 1)
    words = agent_words(6, 21)
    assert len({int(streams[e][0]["command"]) for e in range(6)}) >= 3

    def run(envs):
        out = build_agent(84, 84).act_batch([obs_of(streams[e][0]) for e in envs], deterministic=True, allowed=[words[e] for e in envs])
        return out, envs.index(0)
    alone, _ = run([0])
    assert (words[0][0] >> int(alone.action[0, 0])) & 1 and (words[0][1] >> int(alone.action[0, 1])) & 1
    for envs in ([0, 1, 2], [3, 4, 0], [5, 0, 3], [0, 1, 2, 3, 4, 5], [4, 0]):
        out, i = run(envs)
        for k in ("action", "logp", "value", "feat", "allowed"):
            assert torch.equal(getattr(out, k)[i], getattr(alone, k)[0]), (envs, k)


def test_act_with_allowed_eager_and_graphed(hip):
    """act(allowed=) through the captured step (eager run, capture, replay) and through act_from_feature: the action is allowed, equals
    act_batch's for the same draws, and allowed=None after masked steps is today's step."""
    from tests.test_act_batch_gpu import build_agent, env_streams, obs_of, rel
    T = 5
    streams, _ = env_streams(1, 84, 84, 1, T)
    one, batch, plain, eager = (build_agent(84, 84) for _ in range(4))
    eager.act_graph, one.act_graph = False, True
    for t in range(T):
        words = agent_words(1, 90 + t)[0]
        outs = []
        for ag in (one, eager):
            torch.manual_seed(60 + t)
            outs.append(ag.act(obs_of(streams[0][t]), allowed=words))
        torch.manual_seed(60 + t)
        b = batch.act_batch([obs_of(streams[0][t])], allowed=[words])
        for f, a, lp, v, _hid in outs:
            assert (words[0] >> int(a[0])) & 1 and (words[1] >> int(a[1])) & 1
            assert [int(a[0]), int(a[1])] == host(b.action[0]).tolist()
            assert rel([float(lp[0]), float(lp[1])], host(b.logp[0])) < 1e-6
    assert any(isinstance(k, tuple) and k[-1] == "mask" for k in one._ag["graphs"]), "the masked step was never captured"
    torch.manual_seed(3)
    x = one.act(obs_of(streams[0][T - 1]))
    torch.manual_seed(3)
    y = plain.act(obs_of(streams[0][T - 1]))
    assert int(x[1][0]) == int(y[1][0]) and int(x[1][1]) == int(y[1][1])
    assert rel([float(x[2][0]), float(x[2][1])], [float(y[2][0]), float(y[2][1])]) < 1e-6


# ----------------------------------------------------------------------------- 7. through an update
def am_cfg(**kw):
    d = dict(use_adv_norm=True, ppo_epoch=1, max_grad_norm=250.0, lr=3e-4)
    d.update(kw)
    return d


def masked_storages(seed, throttle_word, steer_word=ALL33, T=8):
    """Synthetic storages (tests/test_ppo_stats_gpu.storages), one minibatch of T rows, with `allowed` words on every row and the stored
    actions moved into the allowed sets."""
    from tests.test_ppo_stats_gpu import storages
    pair = storages(T, 1, seed)
    for s, w, K in ((pair[0], steer_word, 33), (pair[1], throttle_word, 3)):
        if w is None:
            continue
        s._allowed_tensor()[:] = int(ar.to_i64([w])[0])
        ok = torch.tensor([k for k in range(K) if (w >> k) & 1], device="cuda")
        s.action.copy_(ok[s.action.clamp(0, K - 1) % ok.numel()])
    return pair


def rule_all(obs, info):
    return ALL33, ALL3


def test_update_with_all_ones_masks_is_the_plain_update(tmp_path):
    from cadre_amd.actmask import ActionMasks
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section
    from tests.test_imitation_gpu import make_agent
    res = []
    for masked in (False, True):
        agent = make_agent(tmp_path)
        shared = Shared_grad_buffers(agent.model_dict, agent.device)
        s, t = masked_storages(300, ALL3 if masked else None, ALL33 if masked else None)
        torch.manual_seed(4)
        stt = {}
        kw = dict(actmask=ActionMasks(rule_all, agent.arena.n_out, agent.device)) if masked else {}
        losses = learner_section(agent, s, t, False, am_cfg(ppo_epoch=2), shared, stats=stt, **kw)
        torch.cuda.synchronize()
        assert agent.learner.loss_mode == "ppo"
        res.append((agent.arena.params.clone(), losses, stt, agent.arena.step))
    assert torch.equal(res[0][0], res[1][0]) and res[0][1] == res[1][1] and res[0][3] == res[1][3]
    am = res[1][2]["actmask"]
    assert "actmask" not in res[0][2] and am["steps"] == 2 and am["masked_share"] == (0.0, 0.0) and am["allowed_bins"] == (33.0, 3.0)
    assert am["pressure"] == (0.0, 0.0) and am["forced_rows"] == (0.0, 0.0)


def test_forbidden_bin_keeps_its_weights(tmp_path):
    """The last throttle bin forbidden on every row: its last-layer weight row and bias in every categorical throttle actor are
    bit-unchanged after the steps (zero gradient, zero Adam moments, no decay); the rest is finite and moved."""
    from cadre_amd.actmask import ActionMasks
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section
    from tests.test_imitation_gpu import make_agent
    agent = make_agent(tmp_path)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    s, t = masked_storages(310, 0b011)
    before = agent.arena.params.clone()
    stt = {}
    torch.manual_seed(6)
    learner_section(agent, s, t, False, am_cfg(ppo_epoch=3), shared, stats=stt,
                    actmask=ActionMasks(lambda o, i: (ALL33, 0b011), agent.arena.n_out, agent.device))
    torch.cuda.synchronize()
    after = agent.arena.params
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
    assert stt["actmask"]["masked_share"][1] > 0 and stt["actmask"]["allowed_bins"][1] == pytest.approx(2.0 * stt["actmask"]["masked_share"][1])
    assert stt["actmask"]["masked_share"][0] == 0.0 and stt["actmask"]["forced_rows"] == (0.0, 0.0)
    cmds = set(host(t.command)[:8, 0].tolist())
    moved = 0
    for c in range(4):
        b4, af = agent.arena.views(before, "throttle_ppo_%d" % c), agent.arena.views(after, "throttle_ppo_%d" % c)
        assert torch.equal(b4["control.linear.4.weight"][2], af["control.linear.4.weight"][2]), c
        assert torch.equal(b4["control.linear.4.bias"][2], af["control.linear.4.bias"][2]), c
        if c in cmds:                                                          # a net that owns rows: its other two bins moved
            for k in (0, 1):
                assert not torch.equal(b4["control.linear.4.weight"][k], af["control.linear.4.weight"][k]), (c, k)
            assert not torch.equal(b4["critic.4.weight"], af["critic.4.weight"]) and not torch.equal(b4["control.linear.0.weight"], af["control.linear.0.weight"])
            moved += 1
    assert moved >= 1
    for c in set(host(s.command)[:8, 0].tolist()):
        b4, af = agent.arena.views(before, "steer_ppo_%d" % c), agent.arena.views(after, "steer_ppo_%d" % c)
        assert not torch.equal(b4["control.linear.4.weight"], af["control.linear.4.weight"])


def test_masked_update_gradient_equals_float64_autograd(tmp_path):
    """One step of learner_section (T = 8, one minibatch of 8 rows) against float64 autograd through the oracle's nets of the PPO loss on
    the COMPACTED rows (index_select of the allowed bins, Categorical(logits=...)), per parameter within 2e-4 of the model's max |g| (the
    bar of tests/test_learner_gpu.py for the unmasked update)."""
    from cadre_amd import synth
    from cadre_amd.actmask import ActionMasks
    from oracle import ppo_ref
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section
    from tests.test_imitation_gpu import make_agent
    T, C = 8, 4
    agent = make_agent(tmp_path)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    steer_word = int(ar.to_u64(ap.random_words(np.random.RandomState(2), 1, 33))[0]) & ALL33
    s, t = masked_storages(320, 0b101, steer_word)
    r = np.random.RandomState(9)                                               # per-row words: vary them over the rows
    for stor, K in ((s, 33), (t, 3)):
        w = ap.random_words(r, T, K)
        acts = host(stor.action)[:T, 0]
        w = ar.to_i64(ar.effective(w, K, acts)[0])                            # (the stored action stays allowed)
        stor.allowed[:T] = torch.from_numpy(w).cuda()
    torch.manual_seed(5)
    learner_section(agent, s, t, False, am_cfg(max_grad_norm=1e9, lr=1e-9), shared,
                    actmask=ActionMasks(rule_all, agent.arena.n_out, agent.device))
    torch.cuda.synchronize()
    ring = agent._gather_idx
    idx = ring["slots"][(ring["pos"] - 1) % len(ring["slots"])][0].numpy()    # [2][T]: the step's index vectors
    params = {m: {k: p.double().requires_grad_(True) for k, p in d.items()} for m, d in ppo_ref.to_torch_params(synth.ppo_state(11)).items()}
    f = lambda x: host(x).reshape(x.shape[0], -1)
    lrn = agent.learner
    total = 0
    for hd, (head, K, stor) in enumerate((("steer", 33, s), ("throttle", 3, t))):
        ti = idx[hd]
        x = torch.from_numpy(host(stor._obs)[ti][:, :, :530]).double().permute(1, 0, 2).reshape(-1, 530)
        hid = (torch.from_numpy(host(stor._hn)[ti][:, :530]).double(), torch.from_numpy(host(stor._cn)[ti][:, :530]).double())
        col = {k: torch.from_numpy(f(src)[ti, 0].astype(np.float64)) for k, src in
               (("ov", stor.value_preds), ("ret", stor.returns), ("olp", stor.action_log_probs), ("adv", stor.advantages))}
        act, cmd, words = f(stor.action)[ti, 0], f(stor.command)[ti, 0], host(stor.allowed)[ti]
        on = ar.bits(ar.effective(words, K, act)[0], K)
        nets = {}
        for b in range(T):
            c = int(cmd[b])
            if c not in nets:
                h, _ = ppo_ref.lstm_forward(x, hid, params["%s_lstm_%d" % (head, c)])
                nets[c] = (ppo_ref.mlp3(h, params["%s_ppo_%d" % (head, c)], "control.linear"), ppo_ref.mlp3(h, params["%s_ppo_%d" % (head, c)], "critic").view(-1))
            lg, v = nets[c][0][b], nets[c][1][b]
            keep = torch.from_numpy(np.flatnonzero(on[b]))
            dist = torch.distributions.Categorical(logits=lg.index_select(0, keep))
            lp = dist.log_prob(torch.tensor(int(np.flatnonzero(np.flatnonzero(on[b]) == int(act[b]))[0])))
            ratio = torch.exp(lp - col["olp"][b])
            A, ov, R = col["adv"][b], col["ov"][b], col["ret"][b]
            a_loss = -torch.min(ratio * A, torch.clamp(ratio, 1 - lrn.clip, 1 + lrn.clip) * A)
            vpc = ov + (v - ov).clamp(-lrn.clip, lrn.clip)
            v_loss = 0.5 * torch.max((v - R) ** 2, (vpc - R) ** 2)
            total = total + (lrn.vc * v_loss + lrn.cc * a_loss - lrn.ec * dist.entropy()) / T
    total.backward()
    worst = 0.0
    for mn, d in params.items():
        gv = agent.arena.views(agent.arena.grads, mn)
        grads = [p.grad for p in d.values() if p.grad is not None]
        scale = max([float(g.abs().max()) for g in grads] + [1e-30])
        for k, p in d.items():
            g64 = torch.zeros_like(p) if p.grad is None else p.grad
            err = float((gv[k].cpu().double() - g64).abs().max()) / max(scale, 1e-12)
            worst = max(worst, err if scale > 1e-12 else 0.0)
            if scale > 1e-12:
                assert err < 2e-4, (mn, k, err)
            else:
                assert float(gv[k].abs().max()) == 0.0, (mn, k)
    print("masked section gradient: worst per-parameter error (rel. to model max |g|) %.2e" % worst)


def test_section_refusals(tmp_path):
    import types
    from cadre_amd.actmask import ActionMasks
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section, learner_section_multi
    from tests.test_imitation_gpu import make_agent
    agent = make_agent(tmp_path)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    am = ActionMasks(rule_all, agent.arena.n_out, agent.device)
    s, t = masked_storages(330, 0b011)
    mixer = types.SimpleNamespace(label_smoothing=0.0, entries=lambda *a: [])
    with pytest.raises(ValueError, match="demo_mix"):
        learner_section_multi(agent, [(s, t)], [False], am_cfg(), shared, demo=mixer, actmask=am)
    with pytest.raises(ValueError, match="fused_gather"):
        learner_section(agent, s, t, False, am_cfg(), shared, fused_gather=False, actmask=am)
    with pytest.raises(ValueError, match="actmask excludes"):
        agent.update_policy_from_storages([(s, torch.arange(8), s.advantages, t, torch.arange(8), t.advantages)], actmask=am, evaluate=True)
    with pytest.raises(ValueError, match="set_loss"):
        agent.learner.set_loss("ppo+masks")
    # storages that carry words, without actmask=: the unmasked loss would train against masked old_logp
    with pytest.raises(ValueError, match="carries `allowed` words"):
        learner_section(agent, s, t, False, am_cfg(), shared)
    with pytest.raises(ValueError, match="carries `allowed` words"):
        learner_section_multi(agent, [(s, t)], [False], am_cfg(), shared)
    assert agent.learner.loss_mode == "ppo"


# ----------------------------------------------------------------------------- 8. train_vec with the synthetic env
def test_train_vec_with_a_rule(tmp_path):
    import os
    import types
    from cadre_amd.actmask import allowed_from_controls
    from ppo_agent.train import train_vec
    from tests.helpers import SyntheticEnv, topology_cfgs
    train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path), T=8, episodes=1)
    for k in ("port", "routes", "scenarios", "town"):
        env_cfg[k] = list(env_cfg[k]) * 2
    steer_word = allowed_from_controls(agent_cfg.STEER_CONTROL, -0.5, 0.5)        # no extreme steer bins
    seen = []

    def rule(obs, info):
        seen.append(info)
        brake_only = (len(seen) // 2) % 2 == 1                                 # every other step: no "accelerate" bin
        return steer_word, (0b011 if brake_only else 0b111)
    lines, snap = [], {}
    logger = types.SimpleNamespace(log=lines.append)

    def callback(event, **state):
        if event == "rollout":
            snap["rows"] = [[(host(s.action)[:8, 0].copy(), host(s.allowed)[:8].copy()) for s in pair] for pair in state["rollouts"]]
    train_cfg.update(save_interval=10 ** 6, log_stats=True, action_mask=rule)
    os.makedirs(str(tmp_path), exist_ok=True)
    agent = train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, 2, env_cls=SyntheticEnv, logger=logger, callback=callback)
    torch.cuda.synchronize()
    assert agent.learner.loss_mode == "ppo" and bool(torch.isfinite(agent.arena.params).all())
    # (the rule runs before every act: None after a reset, else the environment's last info)
    assert len(seen) == 16 and seen[0] is None and seen[1] is None and sum(isinstance(x, dict) and "action_done" in x for x in seen) >= 8
    n_masked = 0
    for pair in snap["rows"]:
        for h, (acts, words) in enumerate(pair):
            K = (33, 3)[h]
            on = ar.bits(ar.effective(words, K)[0], K)
            assert on[np.arange(8), acts].all(), "a stored action violates its word"
            assert (ar.to_u64(words) & np.uint64(ar.all_word(K)) != 0).all()
            n_masked += int((~on).any(-1).sum())
    assert n_masked >= 16 + 4
    stat = [x for x in lines if "masked rows" in x]
    assert len(stat) == 1
    shares = stat[0].split("masked rows: ")[1].split(",")[0].split("/")
    assert float(shares[0]) == 1.0 and 0.0 < float(shares[1]) < 1.0, stat[0]
    with pytest.raises(ValueError, match="not part of a checkpoint"):
        train_cfg.update(checkpoint_interval=2)
        train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, 2, env_cls=SyntheticEnv, logger=logger)
