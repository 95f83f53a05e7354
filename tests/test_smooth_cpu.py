"""CPU: the temporal smoothness term (cadre_amd/smooth.py, tests/smooth_ref.py, tests/smooth_parity.py) — the configuration and its
refusals, the rotation rule, the control tables, the reference statements against float64 autograd, the mutants against the running
bound, the ambiguity cap of the cases, and the bindings."""
import types

import numpy as np
import pytest
import torch

from tests import loss_parity as lp
from tests import smooth_parity as sp
from tests import smooth_ref as ref
from tests.loss_parity import F4, F8, X64, XVE

IDS = [sp.case_id(kw) for kw in sp.SMOOTH_CASES]


# ----------------------------------------------------------------------------- configuration
def test_config_defaults_and_refusals():
    from cadre_amd.smooth import smooth_config, smooth_runner
    assert smooth_config(None) is None
    assert smooth_config(dict(coeff=0.25)) == dict(coeff=0.25, entries=None, head_scale=(1.0, 1.0))
    cfg = smooth_config(dict(coeff=("linear", 1, 0), entries=2, head_scale=[2, 0]))
    assert cfg == dict(coeff=("linear", 1, 0), entries=2, head_scale=(2.0, 0.0))
    f = lambda x: 1.0 - x
    assert smooth_config(dict(coeff=f))["coeff"] is f
    for bad, why in ((3, "None or a dict"), ({}, "needs coeff"), (dict(coeff=1, beta=2), "unknown"), (dict(coeff="x"), "coeff must"),
                     (dict(coeff=True), "coeff must"), (dict(coeff=float("nan")), "coeff must"), (dict(coeff=("linear", 1)), "coeff must"),
                     (dict(coeff=1, entries=0), "entries"), (dict(coeff=1, entries=1.5), "entries"), (dict(coeff=1, entries=True), "entries"),
                     (dict(coeff=1, head_scale=(1, -1)), "head_scale"), (dict(coeff=1, head_scale=(1,)), "head_scale"),
                     (dict(coeff=1, head_scale=(1, float("inf"))), "head_scale")):
        with pytest.raises(ValueError, match=why):
            smooth_config(bad)
    assert smooth_runner(None, None) is None
    for kw, why in ((dict(demo_mix={}), "demo_mix"), (dict(suggest={}), "one kind array"), (dict(self_imitation={}), "self_imitation"),
                    (dict(sample_reuse={}), "sample_reuse"), (dict(fused_gather=False), "fused_gather")):
        with pytest.raises(ValueError, match=why):
            smooth_runner(None, dict(coeff=0.1), **kw)


def test_section_refusals_come_before_any_device_work():
    from cadre_amd.ppo_agent.train import _check_smooth
    _check_smooth(None, object(), object(), object(), object(), False)
    for args, why in (((object(), None, None, None), "excludes demo"), ((None, object(), None, None), "excludes demo"),
                      ((None, None, None, object()), "excludes demo"), ((None, None, object(), None), "excludes reuse")):
        with pytest.raises(ValueError, match=why):
            _check_smooth(object(), *args)
    with pytest.raises(ValueError, match="fused_gather"):
        _check_smooth(object(), None, None, None, None, False)


# ----------------------------------------------------------------------------- the rotation rule
def test_rotation_rule():
    """Successor entry k of step s belongs to worker (s E + k) mod nW; with E < nW every worker is paired equally often over nW steps, and
    the numpy statement of cadre_smooth_mates leaves exactly the other workers' rows without a partner."""
    from cadre_amd.smooth import smooth_worker, successor_index
    assert [smooth_worker(s, 2, 3, k) for s in range(3) for k in range(2)] == [0, 1, 2, 0, 1, 2]
    assert [smooth_worker(s, 3, 3, k) for s in range(2) for k in range(3)] == [0, 1, 2, 0, 1, 2]
    assert [smooth_worker(s, 1, 4, 0) for s in range(5)] == [0, 1, 2, 3, 0]
    for bad in ((0, 0, 3, 0), (0, 4, 3, 0), (0, 2, 3, 2), (-1, 1, 1, 0), (0, 1, 0, 0), (True, 1, 1, 0)):
        with pytest.raises(ValueError):
            smooth_worker(*bad)
    assert successor_index(torch.tensor([0, 5, 6, 7]), 8).tolist() == [1, 6, 7, 7]
    Bw, nW, E, T, C = 5, 3, 2, 11, 2
    for step in range(4):
        src = [(np.ones(T + 1, F4), None, np.zeros(T + 1, np.int32)) for _ in range(2 * nW)]
        idx = np.zeros((2 * (nW + E), Bw), np.int64)
        idx[:2 * nW] = np.arange(Bw)[None, :]
        for k in range(E):
            idx[2 * (nW + k): 2 * (nW + k) + 2] = idx[0] + 1
        kind, mate = ref.smooth_mates(src, idx, nW, E, Bw, T, C, step * E, None, (nW + E) * Bw)
        paired = sorted(smooth_worker(step, E, nW, k) for k in range(E))
        for w in range(nW):
            got = mate[:, w * Bw:(w + 1) * Bw]
            assert (got >= 0).all() if w in paired else (got == -1).all()
        assert (kind[:, :nW * Bw] == 0).all() and (kind[:, nW * Bw:] == 1).all()
        i = np.flatnonzero(mate[0] >= 0)
        assert np.array_equal(mate[0][mate[0][i]], i)                      # partners name each other


def test_pair_rule():
    T, C = 6, 2
    m, tl, cmd = np.ones(T + 1, F4), np.zeros(T + 1, F4), np.zeros(T + 1, np.int32)
    ok = lambda t: ref.pair_valid(m, tl, cmd, t, T, C)
    assert [ok(t) for t in range(-1, T + 1)] == [False] + [True] * (T - 1) + [False, False]
    m[1], tl[2], cmd[4] = 0, 1, 1
    assert [ok(t) for t in range(T)] == [True, False, False, False, False, False]
    assert ref.pair_valid(m, None, cmd, 2, T, C)                           # NULL time limits: no cuts
    cmd[:] = C
    assert not ref.pair_valid(np.ones(T + 1, F4), None, cmd, 0, T, C)      # a command out of range


# ----------------------------------------------------------------------------- the control tables
def test_smooth_tables():
    from cadre_amd.smooth import control_values, smooth_tables
    steer = {k: -0.5 + k / 32.0 for k in range(33)}
    thr = {0: [0.0, 1.0], 1: [0.0, 0.0], 2: [0.7, 0.0]}
    agent = types.SimpleNamespace(STEER_CONTROL=steer, THROTTLE_CONTROL=thr, arena=types.SimpleNamespace(n_out=(33, 3), device="cpu"))
    t = smooth_tables(agent)
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, 64) and t.is_contiguous()
    want = np.zeros((2, 64), F8)
    want[0, :33] = [steer[k] for k in range(33)]
    want[1, :3] = [-1.0, 0.0, 0.7]
    assert np.array_equal(t.numpy(), want.astype(F4))
    # throttle - brake is formed in float64 and rounded once
    a, b = 0.1 + 2.0 ** -30, 0.1
    assert control_values([0.0], [[a, b]])[1, 0] == F4(a - b) and F4(a - b) != F4(F4(a) - F4(b))
    for bad in (([float("nan")], [[0, 0]]), ([0.0] * 65, [[0, 0]]), ([0.0], [[0, 0, 0]])):
        with pytest.raises(ValueError):
            control_values(*bad)
    with pytest.raises(ValueError):
        smooth_tables(types.SimpleNamespace(STEER_CONTROL={0: 0.0}, THROTTLE_CONTROL=thr, arena=agent.arena))


# ----------------------------------------------------------------------------- the statements against autograd
@pytest.mark.parametrize("K", [33, 3])
def test_pair_statements_against_float64_autograd(K):
    """d and the gradient into both rows (plain heads) against torch float64 autograd of cf sum d^2."""
    r = np.random.RandomState(K)
    n, cf = 7, 0.37
    x, xm = r.standard_normal((n, K)) * 2.0, r.standard_normal((n, K)) * 2.0
    ck = sp.ctrl_table((33, 3))[0 if K == 33 else 1, :K].astype(F8)
    X = X64()
    own = ref.smooth_pair(X, X.c(x), X.c(xm), X.c(ck), X.c(cf))
    succ = ref.smooth_pair(X, X.c(xm), X.c(x), X.c(ck), X.c(cf), succ=True)
    tx, tm = torch.tensor(x, requires_grad=True), torch.tensor(xm, requires_grad=True)
    total = ref.smooth_loss_torch(tx, tm, torch.tensor(ck), cf)
    total.backward()
    assert np.array_equal(own["d"], -succ["d"]) and np.array_equal(own["mu"], succ["mu_mate"])
    assert abs(float(total.detach()) - cf * float((own["d"] ** 2).sum())) < 1e-13
    assert np.abs(own["gs"] - tx.grad.numpy()).max() < 1e-13 and np.abs(succ["gs"] - tm.grad.numpy()).max() < 1e-13
    assert np.abs(own["gs"]).max() > 1e-3


def test_pair_statements_through_an_ordinal_head():
    """An ordinal head: the bin-space gradient through ord_backward against central differences of cf d^2 in the threshold units."""
    K, cf = 33, 0.5
    r = np.random.RandomState(5)
    rk = lp.rank_table(K, True)[:K].astype(np.int64)
    x, xm = r.standard_normal((1, K)), r.standard_normal((1, K))
    ck = sp.ctrl_table((33, 3))[0, :K].astype(F8)
    X = X64()

    def total(a, b):
        o = ref.smooth_pair(X, lp.ord_logits(X, a, rk)[0], lp.ord_logits(X, b, rk)[0], ck, X.c(cf))
        return cf * float(o["d"][0] ** 2)
    xb, s, t = lp.ord_logits(X, x, rk)
    g = lp.ord_backward(X, ref.smooth_pair(X, xb, lp.ord_logits(X, xm, rk)[0], ck, X.c(cf))["gs"], s, t, rk)
    eps = 1e-6
    for j in range(K):
        e = np.zeros((1, K))
        e[0, j] = eps
        fd = (total(x + e, xm) - total(x - e, xm)) / (2 * eps)
        assert abs(fd - g[0, j]) < 1e-8, (j, fd, g[0, j])


# ----------------------------------------------------------------------------- the cases, the bound and the mutants
@pytest.mark.parametrize("i", range(len(sp.SMOOTH_CASES)), ids=IDS)
def test_cases_hold_their_planted_rows_and_the_ambiguity_cap(i):
    """Every case: the five planted slots per head do what they were planted for, and the float64 pairs alone meet at most one ambiguous
    row (loss_parity's condition); both layouts hold the same pairs."""
    kw = sp.SMOOTH_CASES[i]
    for layout in ("prefix", "random"):
        c = sp.smooth_case(kw, layout)
        assert c.B == {(12, 1, 1): 24, (5, 3, 2): 25, (8, 3, 3): 48, (75, 2, 2): 300}[(c.Bw, c.nW, c.E)]
        for h in range(2):
            p = c.plant[h]
            assert c.mate[h, p["equal"]] >= 0 and c.kindrow[h, p["equal"]] == 0
            assert all(c.mate[h, p[k]] == -1 for k in ("mask", "limit", "command", "last"))
            assert sp.paired_rows(c, h, False).size >= 3
        want = sp.run_smooth(c, XVE)
        assert int((want["amb"] & ~c.planted).sum()) <= 1
    assert sorted({(kw["Bw"], kw["nW"], kw["E"]) for kw in sp.SMOOTH_CASES}) == sorted(sp.SHAPES)


@pytest.mark.parametrize("i", range(len(sp.SMOOTH_CASES)), ids=IDS)
def test_emulation_is_inside_the_bound_and_every_mutant_outside(i):
    """The fp32 emulation in the kernel's order and in strictly sequential order passes the check; every mutant of the pair statements
    fails it (the wrong command net needs more than one net)."""
    c = sp.smooth_case(sp.SMOOTH_CASES[i])
    want = sp.run_smooth(c, XVE)
    for order in ("tree", "seq"):
        sp.check_smooth(c, sp.emulate_smooth(c, order), want, "emulation %s %s" % (order, c.tag()), quiet=True)
    for m in ref.MUTANTS:
        if m == "mate_wrong_net" and c.C == 1:
            continue
        with pytest.raises(AssertionError):
            sp.check_smooth(c, sp.emulate_smooth(c, mut={m}), want, m, quiet=True)


def test_the_two_partners_hold_the_same_mu_bits_in_the_emulation():
    c = sp.smooth_case(sp.SMOOTH_CASES[0])
    got = sp.emulate_smooth(c)
    for h in range(2):
        i = sp.paired_rows(c, h, False)
        assert np.array_equal(got["smooth_d"][h, i], -got["smooth_d"][h, c.mate[h, i]]) and np.abs(got["smooth_d"][h, i]).max() > 0


def test_jitter_statement():
    T, C, K = 9, 2, 3
    ctrl = sp.ctrl_table((33, 3))[1]
    a = np.array([0, 2, 2, 1, 5, 0, 0, 1, 2, 0], np.int64)
    m, cmd = np.ones(T + 1, F4), np.zeros(T + 1, np.int32)
    m[5] = 0
    n, s, mx = ref.action_jitter(a, m, None, cmd, T, C, K, ctrl)
    # pairs t = 0, 1, 2 and 6, 7 count (t = 3, 4: action 5 is no bin; t = 5: the episode ended)
    want = [abs(F4(ctrl[a[t + 1]] - ctrl[a[t]])) for t in (0, 1, 2, 6, 7)]
    assert n == 5.0 and abs(s - float(np.sum(want, dtype=F8))) < 1e-15 and mx == float(max(want))


# ----------------------------------------------------------------------------- the bindings
def test_hip_declares_the_three_symbols():
    from cadre_amd import hip
    for name, n in (("cadre_smooth_mates", 13), ("cadre_ppo_smooth_loss", 46), ("cadre_action_jitter", 9)):
        assert name in hip.SYMBOLS and len(hip.SYMBOLS[name]) == n
    assert hip.HP_SMOOTH_COEFF == 15 and hip.HP_FIELDS == 16 and hip.SMOOTH_STATS_FIELDS == 4
    import os
    header = open(os.path.join(os.path.dirname(hip.__file__), "..", "include", "cadre_hip.h")).read()
    for name in ("cadre_smooth_mates", "cadre_ppo_smooth_loss", "cadre_action_jitter", "CADRE_HP_SMOOTH_COEFF = 15",
                 "#define CADRE_SMOOTH_STATS_FIELDS 4", "#define CADRE_HP_FIELDS 16"):
        assert name in header
