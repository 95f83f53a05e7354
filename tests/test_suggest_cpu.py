"""No GPU: exploration suggestions (cadre_amd/suggest.py, csrc/suggest.hip).

  * train_cfg["suggest"] validation: every refusal, the name -> code map, the helpers;
  * the float64 row body of tests/suggest_parity.py is the autograd reference of tests/suggest_ref.py (1e-12 on categorical heads, a
    twentieth of the bound on ordinal heads, as tests/test_loss_parity_cpu.py documents for its own);
  * the fp32 emulation passes the bound in two summation orders at every case of the GPU file; every case meets at most one ambiguous
    row (planted ties aside), from the pairs alone — the suggestion term adds no branch;
  * every mutant is rejected; its excess is printed;
  * the entry points are declared, bound and exported, and the ABI version stays 15."""
import os
import re

import numpy as np
import pytest
import torch

from tests import loss_parity as lp
from tests import suggest_parity as sp
from tests import suggest_ref
from tests.loss_parity import F8, X64, XVE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (case of lp.PPO_CASES, kind pattern, Z): every shape of the grid, the three patterns, Z = 1 and 8
GRID = [(0, "all", 1), (1, "alt", 8), (2, "all", 8), (3, "alt", 1), (4, "all", 8), (5, "alt", 8), (6, "alt", 8), (7, "all", 1),
        (8, "alt", 8), (9, "all", 8), (1, "none", 8), (6, "none", 1)]


@pytest.fixture(scope="module")
def cases():
    return {g: sp.SugCase(*g) for g in GRID}


@pytest.fixture(scope="module")
def refs(cases):
    return {g: sp.run_sug(c, XVE) for g, c in cases.items()}


# ----------------------------------------------------------------------------- configuration
def good_cfg(**over):
    from cadre_amd.suggest import peaked_prior, uniform_prior
    cfg = dict(coeff=0.05, events=dict(blocked=dict(head="throttle", prior=peaked_prior(3, 0, 0.8), horizon=20),
                                       route_deviation=dict(head="steer", prior=uniform_prior(33), horizon=10)))
    cfg.update(over)
    return cfg


def test_config_accepts_and_normalises():
    from cadre_amd.suggest import suggest_config
    assert suggest_config(None) is None
    cfg = suggest_config(good_cfg(coeff=("linear", 0.1, 0.0)))
    assert cfg["coeff"] == ("linear", 0.1, 0.0) and list(cfg["events"]) == ["blocked", "route_deviation"]
    ev = cfg["events"]["blocked"]
    assert ev["log_prior"].dtype == np.float32 and ev["horizon"] == 20 and abs(sum(ev["prior"]) - 1.0) < 1e-15
    # normalised in float64, then log, then rounded once
    raw = suggest_config(good_cfg(events=dict(e=dict(head="steer", prior=[2.0, 6.0], horizon=1))))["events"]["e"]
    assert np.array_equal(raw["log_prior"], np.log(np.array([0.25, 0.75])).astype(np.float32))
    assert callable(suggest_config(good_cfg(coeff=lambda e, n: 0.1))["coeff"])


@pytest.mark.parametrize("bad", [
    "text", dict(coeff=0.1), dict(events={}), good_cfg(extra=1), good_cfg(coeff="x"), good_cfg(coeff=float("nan")), good_cfg(coeff=True),
    good_cfg(coeff=("linear", 1.0)), good_cfg(coeff=("cosine", 1.0, 0.0)), good_cfg(events={}), good_cfg(events=[1]),
    good_cfg(events={"e": dict(head="brake", prior=[0.5, 0.5], horizon=1)}),
    good_cfg(events={"e": dict(head="steer", prior=[0.5, 0.5])}),
    good_cfg(events={"e": dict(head="steer", prior=[0.5, 0.5], horizon=1, extra=2)}),
    good_cfg(events={"e": dict(head="steer", prior=[0.5, 0.5], horizon=0)}),
    good_cfg(events={"e": dict(head="steer", prior=[0.5, 0.5], horizon=1.5)}),
    good_cfg(events={"e": dict(head="steer", prior=[1.0, 0.0], horizon=1)}),
    good_cfg(events={"e": dict(head="steer", prior=[1.0, -0.1], horizon=1)}),
    good_cfg(events={"e": dict(head="steer", prior=[1.0, float("inf")], horizon=1)}),
    good_cfg(events={"e": dict(head="steer", prior=[], horizon=1)}),
    good_cfg(events={"e": dict(head="steer", prior=[0.1] * 65, horizon=1)}),
    good_cfg(events={"e": dict(head="steer", prior="ab", horizon=1)}),
    good_cfg(events={"": dict(head="steer", prior=[0.5, 0.5], horizon=1)}),
    good_cfg(events={"e%d" % i: dict(head="steer", prior=[0.5, 0.5], horizon=1) for i in range(9)}),
])
def test_config_refusals(bad):
    from cadre_amd.suggest import suggest_config
    with pytest.raises(ValueError, match="suggest"):
        suggest_config(bad)


def test_helpers_and_messages():
    from cadre_amd.ppo_agent.suggest import events_from_message, peaked_prior, uniform_prior
    assert uniform_prior(4) == [0.25] * 4
    p = peaked_prior(3, 2, 0.8)
    assert p[2] == 0.8 and abs(sum(p) - 1.0) < 1e-15 and min(p) > 0
    for bad in ((3, 3, 0.5), (3, 0, 1.0), (3, 0, 0.0), (0, 0, 0.5), (65, 0, 0.5)):
        with pytest.raises(ValueError):
            peaked_prior(*bad)
    steer = {"collision static", "route deviation", "outside route!"}
    throttle = {"collision pedestrians!", "collision vehicles!", "vehicle blocked", "exceed speed"}
    for msg in steer | throttle:
        s, t = events_from_message(msg)
        assert (s is not None) == (msg in steer) and (t is not None) == (msg in throttle), msg
    assert events_from_message("vehicle blocked") == (None, "blocked")
    assert events_from_message("success") == (None, None) and events_from_message("") == (None, None)


def test_runner_refusals_say_why():
    from cadre_amd.suggest import suggest_runner
    assert suggest_runner(None, None) is None
    with pytest.raises(ValueError, match="fused_gather"):
        suggest_runner(None, good_cfg(), fused_gather=False)
    with pytest.raises(ValueError, match="demo_mix"):
        suggest_runner(None, good_cfg(), demo_mix=dict(episodes="d"))
    for kw in (dict(checkpoint_interval=2), dict(resume_from="x.pt")):
        with pytest.raises(ValueError, match="not part of a checkpoint"):
            suggest_runner(None, good_cfg(), **kw)


# ----------------------------------------------------------------------------- the mark scan and its mutants
def scan_case(T, Z, seed):
    r = np.random.RandomState(seed)
    ev = np.zeros(T + 1, np.int32)
    masks = np.ones(T + 1, np.float32)
    tl = np.zeros(T + 1, np.float32)
    hz = np.zeros((2, Z + 1), np.int32)
    hz[:, 1:] = r.randint(1, 6, (2, Z))
    return r, ev, masks, tl, hz


def test_mark_scan_statement_and_mutants():
    T, Z = 24, 2
    _r, ev, masks, tl, hz = scan_case(T, Z, 3)
    hz[0] = [0, 3, 5]
    ev[20], masks[20] = 2, 0          # a window of 5 rows: 16 .. 20
    ev[18], masks[18] = 1, 0          # a nearer event two rows before, window 3: 16 .. 18
    masks[10] = 0                     # an episode end without an event
    ev[12], masks[12] = 1, 0          # window 10 .. 12 must stop at the end on row 10 (row 10 belongs to the episode before)
    tl[5] = 1
    ev[6], masks[6] = 2, 0            # window 2 .. 6 cut by the time limit on row 5
    want = suggest_ref.mark_scan(ev, masks, tl, 0, T, Z, hz)
    expect = np.zeros(T, np.int32)
    expect[19:21] = 2
    expect[16:19] = 1
    expect[11:13] = 1
    expect[6] = 2
    assert np.array_equal(want, expect)
    # codes outside 1 .. Z are ignored, a storage without time limits ignores the flags
    ev2 = ev.copy()
    ev2[22], ev2[1] = Z + 1, -1
    assert np.array_equal(suggest_ref.mark_scan(ev2, masks, tl, 0, T, Z, hz), expect)
    no_tl = suggest_ref.mark_scan(ev, masks, None, 0, T, Z, hz)
    assert np.array_equal(no_tl[2:7], [2] * 5)
    for mut in ("window_short", "window_long", "cross_episode", "later_event_wins"):
        got = suggest_ref.mark_scan(ev, masks, tl, 0, T, Z, hz, mut=(mut,))
        n = int((got != expect).sum())
        print("mark mutant %s: %d of %d rows differ" % (mut, n, T))
        assert n > 0, mut


def test_place_kinds_mutant():
    r = np.random.RandomState(5)
    T, Bw, n_src = 12, 5, 4
    Bt = Bw * n_src // 2
    sug = [r.randint(0, 3, T).astype(np.int32) for _ in range(n_src)]
    sug[3] = None
    idx = r.randint(0, T, (n_src, Bw))
    pos = np.stack([r.permutation(Bt) for _ in range(2)])
    init = np.full((2, Bt), 9, np.int32)
    want = suggest_ref.place_kinds(sug, idx, pos, Bt, T, init)
    for zi in range(n_src):
        for b in range(Bw):
            assert want[zi & 1, pos[zi & 1][(zi >> 1) * Bw + b]] == (0 if sug[zi] is None else sug[zi][idx[zi][b]])
    assert not np.array_equal(suggest_ref.place_kinds(sug, idx, pos, Bt, T, init, mut=("kind_unsorted",)), want)


# ----------------------------------------------------------------------------- the reference is the right function
def _grid(case, buf, ld, ns, n):
    net, b, k = np.meshgrid(np.arange(2 * case.C), np.arange(case.B), np.arange(n), indexing="ij")
    return np.asarray(buf)[net * ns + b * ld + k]


@pytest.mark.parametrize("g", [(1, "alt", 8), (2, "all", 8), (5, "alt", 8), (8, "alt", 8), (7, "all", 1)])
def test_float64_body_equals_the_autograd_reference(cases, refs, g):
    case, bound = cases[g], refs[g]
    c = case.base
    hp = {k: float(v) for k, v in c.hp.items()}
    lg = torch.from_numpy(_grid(c, c.logits, c.ldl, c.l_ns, c.ldl).astype(F8)).requires_grad_(True)
    vv = torch.from_numpy(_grid(c, c.values, c.ldv, c.v_ns, 1)[..., 0].astype(F8)).requires_grad_(True)
    ranks = tuple(None if c.rk(h) is None else c.rk(h).tolist() for h in range(2))
    t = lambda a: torch.from_numpy(np.asarray(a))
    out = suggest_ref.suggest_loss(lg, vv, t(c.actions), t(c.cmds), t(c.old_v), t(c.rets), t(c.old_lp), t(c.adv), case.kind, case.prior,
                                   case.Z, c.Ks, ranks, c.C, hp["clip"], hp["value_coeff"], hp["clip_coeff"], hp["ent_coeff"], hp["inv_b"],
                                   float(case.sug_coeff))
    out["total"].backward()
    got = sp.run_sug(case, X64())
    slack = 0.05 if any(c.ordinal) else 0.0

    def close(gv, w, e, name):
        w = np.asarray(w, F8)
        assert (np.abs(np.asarray(gv, F8) - w) <= 1e-12 * max(1.0, float(np.abs(w).max())) + slack * np.asarray(e)).all(), name

    close(_grid(c, got["dlogits"], c.ldl, c.l_ns, c.ldl), lg.grad.numpy(), _grid(c, bound["dlogits"].e, c.ldl, c.l_ns, c.ldl), "dlogits")
    close(_grid(c, got["dvalues"], c.ldv, c.v_ns, 1)[..., 0], vv.grad.numpy(), _grid(c, bound["dvalues"].e, c.ldv, c.v_ns, 1)[..., 0], "dvalues")
    close([float(x) for x in got["losses"]], [float(x.detach()) for x in out["losses"]], [float(x.e) for x in bound["losses"]], "losses")
    close([float(got["sug_losses"][0])], [float(out["sug_loss"].detach())], [float(bound["sug_losses"][0].e)], "sug_losses")
    close(np.stack(got["sug_stats"], 1), out["sug_stats"].numpy(), np.stack([x.e for x in bound["sug_stats"]], 1), "sug_stats")
    close(np.stack(got["stats"], 1), out["stats"].numpy(), np.stack([x.e for x in bound["stats"]], 1), "stats")


# ----------------------------------------------------------------------------- the honest orders pass, the rows stay unambiguous
@pytest.mark.parametrize("g", GRID, ids=lambda g: "case%d-%s-Z%d" % g)
def test_emulation_passes_in_two_orders(cases, refs, g):
    case, ref = cases[g], refs[g]
    for order in ("tree", "seq"):
        worst, n_amb = sp.check_sug(case, sp.emulate_sug(case, order), ref, "emulation %s %s" % (order, case.tag()))
        assert n_amb <= 1
    # the suggestion term adds no ambiguous row: the PPO part alone has the same ones
    assert np.array_equal(ref["amb"], lp.run_loss(case.base, XVE)["amb"])
    if g[1] == "none":
        assert float(ref["sug_losses"][0].v) == 0.0 and float(ref["sug_losses"][0].e) == 0.0
        plain = lp.run_loss(case.base, XVE)
        assert np.array_equal(ref["dlogits"].v, plain["dlogits"].v) and np.array_equal(ref["dlogits"].e, plain["dlogits"].e)


# ----------------------------------------------------------------------------- mutants
MUTANTS = ("kl_reversed", "no_centre", "prior_raw", "mean_marked")


@pytest.mark.parametrize("mut", MUTANTS)
def test_loss_mutants_are_rejected(cases, refs, mut):
    worst = 0.0
    for g in ((1, "alt", 8), (6, "alt", 8), (5, "alt", 8)):
        case = cases[g]
        rep_bad = None
        try:
            sp.check_sug(case, sp.emulate_sug(case, "tree", mut={mut}), refs[g], "mutant %s %s" % (mut, case.tag()), quiet=True)
        except AssertionError as e:
            rep_bad = str(e)
        assert rep_bad is not None, "mutant %s passes the bound at %s" % (mut, case.tag())
        worst = max([worst] + [float(x) for x in re.findall(r"err / bound ([0-9.eE+-]+)", rep_bad)])
    print("loss mutant %s: worst err / bound %.3g" % (mut, worst))
    assert worst > 1.0


def test_kind_at_unsorted_index_is_rejected(cases, refs):
    g = (6, "alt", 8)
    case, c = cases[g], cases[g].base
    r = np.random.RandomState(7)
    pos = np.stack([r.permutation(c.B) for _ in range(2)])
    # the kinds of the case, as a storage's `suggest` read through a sorted layout: placed right they are the case's, placed at the
    # unsorted index they are not
    src = [case.kind[h][pos[h]] for h in range(2)]
    idx = np.stack([np.arange(c.B), np.arange(c.B)])
    init = np.zeros((2, c.B), np.int32)
    right = suggest_ref.place_kinds(src, idx, pos, c.B, c.B, init)
    assert np.array_equal(right, case.kind)
    wrong = suggest_ref.place_kinds(src, idx, pos, c.B, c.B, init, mut=("kind_unsorted",))
    with pytest.raises(AssertionError, match="outside the bound|not exact"):
        sp.check_sug(case, sp.emulate_sug(case, "tree", kind=wrong), refs[g], "kind at the unsorted index", quiet=True)


# ----------------------------------------------------------------------------- the entry points, by name
def test_entry_points_declared_bound_exported():
    from cadre_amd import build, hip
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    L = hip.lib()
    for name in ("cadre_suggest_note", "cadre_suggest_mark", "cadre_suggest_rows", "cadre_ppo_sug_loss"):
        assert hasattr(L, name) and name in hip.SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr), name
    assert "suggest.hip" in build.SOURCES
    assert L.cadre_abi_version() == hip.ABI_VERSION == 15                  # entry points only added
    m = re.search(r"CADRE_HP_SUGGEST_COEFF = (\d+)", hdr)
    assert m and int(m.group(1)) == hip.HP_SUGGEST_COEFF == 12
    assert int(re.search(r"#define CADRE_SUG_STATS_FIELDS (\d+)", hdr).group(1)) == hip.SUG_STATS_FIELDS == 4
    assert len(hip.SYMBOLS["cadre_ppo_sug_loss"]) == 42 and len(hip.SYMBOLS["cadre_suggest_rows"]) == 9


def sug_args(**over):
    """Arguments of cadre_ppo_sug_loss that pass every check (pointers are never dereferenced on the host)."""
    p = 64
    a = dict(logits=p, ldl=64, l_ns=64, values=p, ldv=1, v_ns=1, actions=p, commands=p, old_values=p, returns=p, old_logp=p, adv=p,
             kind=p, prior=p, Z=2, B=8, C=4, nS=33, nT=3, hp=None, clip=0.1, vc=0.1, cc=1.0, ec=0.01, inv_b=0.25, sc=0.5, losses=p,
             sug_losses=p, dl=p, dv=p, scratch=p, sug_scratch=p, poison=None, stats_row=None, F=0, stats_scratch=None, target_kl=0.0,
             stop=None, sug_stats=None, sug_F=0, ord=p, stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("over,msg", [
    (dict(kind=None), "null kind"), (dict(prior=None), "null prior"), (dict(sug_losses=None), "sug_losses"),
    (dict(sug_scratch=None), "sug_scratch"), (dict(Z=0), "Z"), (dict(Z=9), "Z"), (dict(sc=float("inf")), "finite"),
    (dict(sc=float("nan")), "finite"), (dict(ord=None), "rank table"), (dict(B=0), "bad argument"), (dict(ldl=32), "bad argument"),
    (dict(logits=None), "bad argument"), (dict(sug_stats=64, sug_F=3), "suggestion stats"), (dict(stats_row=64, F=8), "stats argument"),
    (dict(hp=12), "hyper-parameter block"),
])
def test_loss_entry_refuses_before_any_launch(over, msg):
    from cadre_amd import hip
    L = hip.lib()
    rc = L.cadre_ppo_sug_loss(*sug_args(**over))
    assert rc < 0 and msg in L.cadre_last_error().decode(), L.cadre_last_error().decode()


def test_small_entries_refuse_before_any_launch():
    from cadre_amd import hip
    L = hip.lib()
    assert L.cadre_suggest_note(None, 64, 64, 2, 8, None) < 0 and L.cadre_suggest_note(64, 64, 64, 0, 8, None) < 0
    assert L.cadre_suggest_mark(64, 2, 8, 0, 64, None) < 0 and L.cadre_suggest_mark(64, 2, 8, 9, 64, None) < 0
    assert L.cadre_suggest_mark(64, 0, 8, 1, 64, None) < 0 and L.cadre_suggest_mark(64, 2, 8, 1, None, None) < 0
    assert L.cadre_suggest_rows(64, 3, 64, 4, 8, None, 8, 64, None) < 0 and L.cadre_suggest_rows(64, 4, 64, 5, 8, None, 8, 64, None) < 0
    assert L.cadre_suggest_rows(64, 2, 64, 4, 8, None, 8, None, None) < 0


# ----------------------------------------------------------------------------- host-side pieces that need no device
def test_set_loss_and_storage_refusals_without_a_device():
    from cadre_amd.ppo_agent.storage import RolloutStorage
    for bad in (-1, 1.5, True, "x"):
        with pytest.raises(ValueError, match="event code"):
            RolloutStorage._event_code(bad)
    s = RolloutStorage(4, 1, 6, 2, 6, True, 0.9, 0.9)
    assert getattr(s, "events", None) is None
    obs = torch.zeros(2, 6)
    one = torch.zeros(1)
    s.insert(obs, one, one, one, 0.0, one, None, 0)
    assert getattr(s, "events", None) is None                        # never saw an event: nothing allocated
    s.insert(obs, one, one, one, 0.0, one, None, 0, event=3)
    assert s.events.dtype == torch.int32 and s.events.tolist() == [0, 3, 0, 0, 0] and s.suggest.shape == (4,)
    for _ in range(4):                                               # the cursor wraps at T + 1: the stale code is overwritten
        s.insert(obs, one, one, one, 0.0, one, None, 0)
    assert s.step == 1 and s.events.tolist() == [0, 3, 0, 0, 0]
    s.insert(obs, one, one, one, 0.0, one, None, 0)
    assert s.events.tolist() == [0, 0, 0, 0, 0]
