"""No GPU: self-imitation learning (cadre_amd/selfimit.py, csrc/selfimit.hip).

  * train_cfg["self_imitation"] validation and every start-up refusal, each with its reason;
  * the entry points are declared, bound and exported, the ABI version stays 15, bad arguments are refused before any launch;
  * the float64 SIL row of tests/selfimit_ref.py is torch autograd of the stated loss;
  * the fp32 emulation of the whole kernel passes the running bound of tests/loss_parity.py in two summation orders at every case of the
    GPU file, and every mutant of the row leaves it;
  * the numpy statements of the scan, the quantisation, the draw and the write-back on hand cases."""
import os
import re

import numpy as np
import pytest
import torch

from tests import selfimit_parity as sp
from tests import selfimit_ref as ref
from tests.loss_parity import F4, F8, X64, XVE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cadre_ppo_sil_loss", "cadre_sil_prepare", "cadre_sil_draw", "cadre_sil_scatter")


@pytest.fixture(scope="module")
def cases():
    return sp.sil_cases()


@pytest.fixture(scope="module")
def refs(cases):
    return [sp.run_sil(c, XVE) for c in cases]


# ----------------------------------------------------------------------------- configuration
def good_cfg(**over):
    cfg = dict(rollouts=4, coeff=0.1)
    cfg.update(over)
    return cfg


def test_config_accepts_and_fills_defaults():
    from cadre_amd.ppo_agent.selfimit import SIL_KEYS, sil_config
    assert sil_config(None) is None
    cfg = sil_config(good_cfg())
    assert cfg == dict(rollouts=4, coeff=0.1, value_coeff=0.01, alpha=0.6, prio_eps=1e-3, tail="drop", blocks=1, seed=0)
    assert set(cfg) == set(SIL_KEYS)
    assert sil_config(good_cfg(coeff=("linear", 0.1, 0.0)))["coeff"] == ("linear", 0.1, 0.0)
    assert callable(sil_config(good_cfg(coeff=lambda e, n: 0.1))["coeff"])
    full = sil_config(good_cfg(value_coeff=0.5, alpha=1, prio_eps=0, tail="bootstrap", blocks=2, seed=-3))
    assert (full["value_coeff"], full["alpha"], full["prio_eps"], full["tail"], full["blocks"], full["seed"]) == (0.5, 1.0, 0.0, "bootstrap", 2, -3)


@pytest.mark.parametrize("bad", [
    "text", dict(coeff=0.1), dict(rollouts=2), good_cfg(extra=1), good_cfg(rollouts=0), good_cfg(rollouts=1.5), good_cfg(rollouts=True),
    good_cfg(coeff="x"), good_cfg(coeff=float("nan")), good_cfg(coeff=True), good_cfg(coeff=("linear", 1.0)), good_cfg(coeff=("cosine", 1.0, 0.0)),
    good_cfg(value_coeff="x"), good_cfg(value_coeff=float("inf")), good_cfg(alpha=0), good_cfg(alpha=-1.0), good_cfg(alpha=float("nan")),
    good_cfg(prio_eps=-1e-3), good_cfg(prio_eps=float("inf")), good_cfg(tail="keep"), good_cfg(tail=None), good_cfg(blocks=0),
    good_cfg(blocks=1.5), good_cfg(seed=1.5), good_cfg(seed=True),
])
def test_config_refusals(bad):
    from cadre_amd.selfimit import sil_config
    with pytest.raises(ValueError, match="self_imitation"):
        sil_config(bad)


class _World(object):
    def __init__(self, n):
        self.n = n

    def dist_world(self):
        return self.n


def test_runner_refusals_say_why():
    from cadre_amd import hip
    from cadre_amd.selfimit import SilRunner, sil_runner
    assert sil_runner(None, None) is None
    assert isinstance(sil_runner(None, good_cfg(), _World(1)), SilRunner)
    with pytest.raises(ValueError, match="demo_mix and suggest.*one kind array"):
        sil_runner(None, good_cfg(), demo_mix=dict(episodes="d"))
    with pytest.raises(ValueError, match="demo_mix and suggest.*one kind array"):
        sil_runner(None, good_cfg(), suggest=dict(coeff=0.1))
    with pytest.raises(ValueError, match="sample_reuse"):
        sil_runner(None, good_cfg(), sample_reuse=dict(rollouts=2))
    for kw in (dict(checkpoint_interval=2), dict(resume_from="x.pt")):
        with pytest.raises(ValueError, match="not part of a checkpoint"):
            sil_runner(None, good_cfg(), **kw)
    with pytest.raises(ValueError, match="fused_gather"):
        sil_runner(None, good_cfg(), fused_gather=False)
    with pytest.raises(hip.CadreHipError, match="in-process chief"):
        sil_runner(None, good_cfg(), in_process_chief=False)
    with pytest.raises(hip.CadreHipError, match="single rank"):
        sil_runner(None, good_cfg(), _World(2))


def test_train_helpers_refuse_and_pass_through():
    from cadre_amd.ppo_agent import train as tr
    assert tr.self_imitation(None, dict()) is None and tr.self_imitation(None, dict(self_imitation=None)) is None
    assert tr.apply_sil(None, None, 0, 4) is None and tr._sil_kw(None, 8, 0, 0, 0) == {}
    with pytest.raises(ValueError, match="sample_reuse"):
        tr.self_imitation(None, dict(self_imitation=good_cfg(), sample_reuse=dict(rollouts=2)))
    with pytest.raises(ValueError, match="not part of a checkpoint"):
        tr.self_imitation(None, dict(self_imitation=good_cfg()), ck_interval=1)
    for kw in (dict(demo=1), dict(suggest=1), dict(reuse=1)):
        args = dict(demo=None, suggest=None, reuse=None)
        args.update(kw)
        with pytest.raises(ValueError, match="sil excludes"):
            tr._check_sil(object(), **args)
    with pytest.raises(ValueError, match="fused_gather"):
        tr._check_sil(object(), None, None, None, False)


def test_words_are_a_pure_function_of_the_key():
    from cadre_amd.selfimit import sil_words
    state = torch.get_rng_state()
    a, b = sil_words(3, 0, 5, 1, 2, 8, 2), sil_words(3, 0, 5, 1, 2, 8, 2)
    assert torch.equal(torch.get_rng_state(), state)                   # the global generator is not touched
    assert a.shape == (2, 16) and a.dtype == torch.int64 and torch.equal(a, b) and int(a.min()) >= 0
    for other in ((4, 0, 5, 1, 2, 8, 2), (3, 1, 5, 1, 2, 8, 2), (3, 0, 6, 1, 2, 8, 2), (3, 0, 5, 0, 2, 8, 2), (3, 0, 5, 1, 3, 8, 2)):
        assert not torch.equal(sil_words(*other), a)
    with pytest.raises(ValueError):
        sil_words(3, 0, -1, 0, 0, 8, 1)


# ----------------------------------------------------------------------------- the entry points, by name
def test_entry_points_declared_bound_exported():
    from cadre_amd import build, hip
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    L = hip.lib()
    for name in NEW:
        assert hasattr(L, name) and name in hip.SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr), name
    assert "selfimit.hip" in build.SOURCES
    assert L.cadre_abi_version() == hip.ABI_VERSION == 15                  # entry points only added
    m = re.search(r"CADRE_HP_SIL_COEFF = (\d+), CADRE_HP_SIL_VALUE_COEFF = (\d+)", hdr)
    assert m and (int(m.group(1)), int(m.group(2))) == (hip.HP_SIL_COEFF, hip.HP_SIL_VALUE_COEFF) == (13, 14)
    assert int(re.search(r"#define CADRE_HP_FIELDS (\d+)", hdr).group(1)) == hip.HP_FIELDS == 16
    assert "sil_coeff" not in hip.HP_INDEX and len(hip.HP_INDEX) == 12
    assert int(re.search(r"#define CADRE_SIL_STATS_FIELDS (\d+)", hdr).group(1)) == hip.SIL_STATS_FIELDS == 6
    assert "CADRE_HP_SIL_VALUE_COEFF are reserved" in hdr
    assert len(hip.SYMBOLS["cadre_ppo_sil_loss"]) == 43


def loss_args(**over):
    """Arguments of cadre_ppo_sil_loss that pass every check (pointers are never dereferenced on the host)."""
    p = 64
    a = dict(logits=p, ldl=64, l_ns=64, values=p, ldv=1, v_ns=1, actions=p, commands=p, old_values=p, returns=p, old_logp=p, adv=p,
             kind=p, B=8, C=4, nS=33, nT=3, hp=None, clip=0.1, vc=0.1, cc=1.0, ec=0.01, inv_b=0.25, sc=0.5, svc=0.1, inv_bs=0.25,
             losses=p, sil_losses=p, sil_w=p, dl=p, dv=p, scratch=p, sil_scratch=p, poison=None, stats_row=None, F=0, stats_scratch=None,
             target_kl=0.0, stop=None, sil_stats=None, sil_F=0, ord=p, stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("over,msg", [
    (dict(kind=None), "null row_kind"), (dict(sil_losses=None), "bad argument"), (dict(sil_w=None), "bad argument"),
    (dict(sil_scratch=None), "bad argument"), (dict(logits=None), "bad argument"), (dict(B=0), "bad argument"), (dict(ldl=32), "bad argument"),
    (dict(inv_bs=float("inf")), "inv_bs"), (dict(inv_bs=float("nan")), "inv_bs"), (dict(inv_bs=0.0), "inv_bs"),
    (dict(sc=0.0, svc=0.0, sil_stats=64, sil_F=6, inv_bs=float("nan")), "inv_bs"), (dict(hp=64, inv_bs=float("nan")), "inv_bs"),
    (dict(sc=float("nan")), "finite"), (dict(svc=float("inf")), "finite"), (dict(sil_stats=64, sil_F=5), "SIL stats"),
    (dict(stats_row=64, F=8), "stats argument"), (dict(hp=12), "hyper-parameter block"),
])
def test_loss_entry_refuses_before_any_launch(over, msg):
    from cadre_amd import hip
    L = hip.lib()
    rc = L.cadre_ppo_sil_loss(*loss_args(**over))
    assert rc < 0 and msg in L.cadre_last_error().decode(), L.cadre_last_error().decode()


def test_small_entries_refuse_before_any_launch():
    from cadre_amd import hip
    L = hip.lib()
    err = lambda: L.cadre_last_error().decode()
    ok_prep = [64, 2, 16, 0.99, None, 0.0, 0, 0.6, 1e-3, None]
    for i, v, msg in ((0, None, "null"), (1, 0, "bad argument"), (2, 1, "bad argument"), (2, 3001, "bad argument"), (3, 1.5, "bad argument"),
                      (6, 2, "tail"), (7, 0.0, "alpha"), (7, -1.0, "alpha"), (7, float("nan"), "alpha"), (8, -1e-3, "prio_eps"),
                      (8, float("inf"), "prio_eps")):
        a = list(ok_prep)
        a[i] = v
        assert L.cadre_sil_prepare(*a) < 0 and "cadre_sil_prepare" in err() and msg in err(), (i, v, err())
    assert L.cadre_sil_prepare(64, 2, 16, 0.99, 64, 0.0, 0, 0.6, 1e-3, None) < 0            # a state without clip_r > 0
    ok_draw = [64, 100, 100, 64, 8, 64, 64, None]
    for i, v in ((0, None), (3, None), (5, None), (6, None), (1, 0), (2, 0), (2, 101), (4, 0)):
        a = list(ok_draw)
        a[i] = v
        assert L.cadre_sil_draw(*a) < 0 and "cadre_sil_draw" in err(), (i, v)
    ok_scat = [64, 100, 64, 8, 64, None, 24, 16, 0.6, 1e-3, None]
    for i, v in ((0, None), (2, None), (4, None), (1, 0), (3, 0), (6, 0), (7, -1), (7, 17), (8, 0.0), (9, -1.0)):
        a = list(ok_scat)
        a[i] = v
        assert L.cadre_sil_scatter(*a) < 0 and "cadre_sil_scatter" in err(), (i, v)


# ----------------------------------------------------------------------------- the row against autograd
@pytest.mark.parametrize("K,n", [(33, 40), (3, 17), (1, 5)])
def test_float64_row_is_autograd_of_the_stated_loss(K, n):
    r = np.random.RandomState(K + n)
    x, v, R = r.standard_normal((n, K)) * 2.0, r.standard_normal(n), r.standard_normal(n)
    R[0], R[1 % n] = v[0], v[1 % n] - 0.5                   # w = 0 rows
    a = r.randint(0, K, n)
    sc, svc, inv_bs = 0.3, 0.2, 1.0 / n
    gk, dval, w, terms = ref.sil_row(X64(), x, a, v, R, (sc, svc, inv_bs))
    # (the coefficients pass through fp32 in the row, as the kernel's arguments do)
    sc32, svc32, ib32 = float(F4(sc)), float(F4(svc)), float(F4(inv_bs))
    lg, vv = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(v).requires_grad_(True)
    total, pol, val = ref.sil_loss_torch(lg, vv, torch.from_numpy(a), torch.from_numpy(R), sc32, svc32)
    (total * (n * ib32)).backward()                         # mean over n rows -> sum times inv_bs
    assert np.abs(gk - lg.grad.numpy()).max() <= 1e-14 and np.abs(dval - vv.grad.numpy()).max() <= 1e-14
    assert np.array_equal(w, np.maximum(R - v, 0)) and w[0] == 0 and np.all(gk[0] == 0) and dval[0] == 0
    assert abs(sc32 * terms["pol"].sum() * ib32 - float(pol.detach()) * n * ib32) <= 1e-14
    assert abs(svc32 * 0.5 * terms["val"].sum() * ib32 - float(val.detach()) * n * ib32) <= 1e-14


# ----------------------------------------------------------------------------- the emulation passes, the mutants do not
@pytest.mark.parametrize("i", range(len(sp.SIL_CASES)))
def test_emulation_passes_in_two_orders(cases, refs, i):
    case, want = cases[i], refs[i]
    for order in ("tree", "seq"):
        worst, n_amb = sp.check_sil(case, sp.emulate_sil(case, order), want, "emulation %s %s" % (order, case.tag()))
        assert n_amb <= 1
    n_sil = sum(case.rows(h, True).size for h in range(2))
    if case.B_ppo == case.B:
        assert n_sil == 0 and all(float(t.v) == 0.0 and float(t.e) == 0.0 for t in want["sil_losses"])
    else:
        assert n_sil > 0 and float(want["sil_losses"][0].v) != 0.0 and all(len(z) == 2 for z in case.zero_rows)


@pytest.mark.parametrize("mut", ref.MUTANTS)
def test_row_mutants_are_rejected(cases, refs, mut):
    worst = 0.0
    for i in (0, 3, 4, 5):                                  # the cases with both kinds of rows (inv_b != inv_bs)
        case = cases[i]
        assert float(case.hp["inv_b"]) != float(case.hp["inv_bs"])
        bad = None
        try:
            sp.check_sil(case, sp.emulate_sil(case, "tree", mut=sp.mutants(case)[mut]), refs[i], "mutant %s %s" % (mut, case.tag()), quiet=True)
        except AssertionError as e:
            bad = str(e)
        assert bad is not None, "mutant %s passes the bound at %s" % (mut, case.tag())
        worst = max([worst] + [float(x) for x in re.findall(r"err / bound ([0-9.eE+-]+)", bad)])
    print("row mutant %s: worst err / bound %.3g" % (mut, worst))


# ----------------------------------------------------------------------------- the buffer's statements on hand cases
def test_draw_statement_on_hand_cases():
    one = np.array([5])
    assert ref.draw(one, 1, np.array([0, 4, 5, 123456789])).tolist() == [0, 0, 0, 0]                 # a single row
    q = np.array([0, 0, 3, 0, 0, 2, 0, ref.Q_MAX, 0, 1, 0])                                           # runs of zeros, a row at the cap
    total = int(q.sum())
    u = np.array([0, 2, 3, 4, 5, 5 + ref.Q_MAX - 1, 5 + ref.Q_MAX, total - 1, total, total + 3, 2 ** 62 - 1])
    want = [2, 2, 5, 5, 7, 7, 9, 9, 2, 5, None]
    got = ref.draw(q, q.size, u)
    assert got[:-1].tolist() == want[:-1] and q[got[-1]] > 0
    assert np.all(q[got] > 0)
    # a filled count below Rcap: the rows behind it never come
    got = ref.draw(q, 6, np.arange(40))
    assert set(got.tolist()) == {2, 5} and got[:5].tolist() == [2, 2, 2, 5, 5] and got[5] == 2
    # sums past 2^32 stay exact
    big = np.full(5, ref.Q_MAX)
    assert ref.draw(big, 5, np.array([ref.Q_MAX * 4, ref.Q_MAX * 4 - 1, ref.Q_MAX * 5])).tolist() == [4, 3, 0]


def test_quantise_statement():
    q = ref.quantise(np.array([0.0, 1.0, 1e-9, 1e30], F4), 0.6, 1e-3)
    assert q[0] == int(np.floor(1e-3 ** 0.6 * 65536)) and q[1] == int(np.floor(1.001 ** 0.6 * 65536)) and q[3] == ref.Q_MAX
    assert ref.quantise(np.array([0.0], F4), 1.0, 0.0)[0] == 1 and ref.quantise(np.array([0.0], F4), 2.0, 1e-9)[0] == 1


def test_scan_statement_on_hand_cases():
    T, g = 6, 0.5
    r = np.array([1, 2, 4, 8, 16, 32, 99], F4)
    V = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 10.0], F4)
    m = np.ones(T + 1, F4)
    R, f = ref.closed_scan(r, m, None, V, g, "drop")                       # no end: nothing closed, nothing eligible
    assert f.tolist() == [0] * 7 and R[5] == 32 and R[4] == 32
    Rb, fb = ref.closed_scan(r, m, None, V, g, "bootstrap")
    assert fb.tolist() == [2] * 6 + [0] and Rb[5] == 37 and Rb[4] == 16 + 0.5 * 37
    m[5] = 0                                                               # an end at the last row: everything closed
    R, f = ref.closed_scan(r, m, None, V, g, "drop")
    assert f.tolist() == [3] * 6 + [0] and R.tolist() == [1 + 1 + 1 + 1 + 1 + 1, 2 + 2 + 2 + 2 + 2, 4 + 4 + 4 + 4, 8 + 8 + 8, 32, 32]
    assert np.array_equal(ref.closed_scan(r, m, None, V, g, "bootstrap")[0], R)
    m[:] = 1
    m[1] = m[3] = 0                                                        # two ends and a cut tail
    R, f = ref.closed_scan(r, m, None, V, g, "drop")
    assert f.tolist() == [3, 3, 3, 3, 0, 0, 0] and R[:4].tolist() == [2, 2, 8, 8]
    Rb, fb = ref.closed_scan(r, m, None, V, g, "bootstrap")
    assert fb.tolist() == [3, 3, 3, 3, 2, 2, 0] and np.array_equal(Rb[:4], R[:4]) and Rb[5] == 37
    tl = np.zeros(T + 1, F4)
    tl[3] = 1                                                              # the second end is a time limit: rows 2 .. 3 are not closed
    R, f = ref.closed_scan(r, m, tl, V, g, "drop")
    assert f.tolist() == [3, 3, 0, 0, 0, 0, 0] and R[3] == 0 and R[2] == 4 and R[:2].tolist() == [2, 2]
    Rb, fb = ref.closed_scan(r, m, tl, V, g, "bootstrap")
    assert fb.tolist() == [3, 3, 2, 2, 2, 2, 0] and Rb[3] == 0.5 and Rb[2] == 4 + 0.5 * 0.5 and np.array_equal(Rb[:2], R[:2])
    q = ref.initial_priorities(R, f, V, 0.6, 1e-3)
    assert np.all(q[2:] == 0) and np.all(q[:2] == ref.quantise(np.array([1.5, 1.5], F4), 0.6, 1e-3))
    # with a reward scale: the staged reward is clamp(r * scale, +-clip)
    Rs, _f = ref.closed_scan(r, m, tl, V, g, "drop", scale=0.5, clip_r=3.0)
    assert Rs[:2].tolist() == [0.5 + 0.5, 1.0]


def test_scatter_statement():
    q = np.array([5, 0, 7, 9])
    w = np.array([0.0, 2.0, 0.5, 1.0], F4)
    got = ref.scatter(q, [2, 0, 2], w, None, 1, 1.0, 0.0)                  # SIL rows are unsorted rows 1 .. 3; row 2 drawn twice
    assert got.tolist() == [int(0.5 * 65536), 0, 65536, 9]
    pos = np.array([3, 2, 1, 0])
    assert ref.scatter(q, [3], w, pos, 3, 1.0, 0.0).tolist() == [5, 0, 7, 1]
