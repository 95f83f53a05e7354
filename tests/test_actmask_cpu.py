"""No GPU: action masks (cadre_amd/actmask.py, csrc/actmask.hip).

  * the float64 statement of tests/actmask_ref.py: gradients against torch float64 autograd on the COMPACTED rows (index_select of the
    allowed bins, Categorical(logits=...)) to 1e-12; with all bits set it equals the existing loss reference (tests/loss_parity.run_loss
    in float64) bit for bit; the sampler's rule and the statistics;
  * the (value, error) row body of tests/actmask_parity.py equals that statement, and the fp32 emulation passes the bound in two
    summation orders at every shape of the GPU file; the one-statement mutants are rejected;
  * allowed_word / allowed_from_controls, bin 63 included; actmask_config validation and every refusal;
  * storages: lazy allocation, .to(), insert / insert_batch argument checks;
  * the entry points are declared, bound and exported, refuse bad arguments before any launch, and the ABI version stays 15."""
import os
import re

import numpy as np
import pytest
import torch

from tests import actmask_parity as ap
from tests import actmask_ref as ar
from tests import loss_parity as lp
from tests.loss_parity import F8, X64, XVE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = [(B, C, Ks, o) for B in ap.SHAPES_B for C in ap.SHAPES_C for Ks in ap.HEADS for o in (False, True)]
GRID_ID = lambda g: "B%d-C%d-K%dx%d-%s" % (g[0], g[1], g[2][0], g[2][1], "ord" if g[3] else "cat")
SMALL = [g for g in GRID if g[0] in (1, 17)]


def case_of(g, words="random"):
    B, C, Ks, o = g
    return ap.AmCase(1000 + 7 * B + C + Ks[0], B, Ks, C, (o, o), words)


def ref_loss(c, allowed=None):
    lg, vv = c.dense()
    hp = {k: float(v) for k, v in c.hp.items()}
    return ar.loss(lg, vv, c.actions, c.cmds, c.old_v, c.rets, c.old_lp, c.adv, c.allowed if allowed is None else allowed, c.Ks,
                   [c.rk(0), c.rk(1)], c.C, hp["clip"], hp["value_coeff"], hp["clip_coeff"], hp["ent_coeff"], hp["inv_b"])


def flat_dl(c, dl):
    out = np.zeros(c.logits.size)
    for n in range(2 * c.C):
        out[n * c.l_ns: n * c.l_ns + c.B * c.ldl] = dl[n].reshape(-1)
    return out


# ----------------------------------------------------------------------------- the float64 statement
@pytest.mark.parametrize("g", SMALL, ids=GRID_ID)
def test_reference_gradients_equal_autograd_on_compacted_rows(g):
    from tests import ordinal_ref
    c = case_of(g)
    out = ref_loss(c)
    lg, vv = c.dense()
    L = torch.from_numpy(lg).requires_grad_(True)
    V = torch.from_numpy(vv).requires_grad_(True)
    hp = {k: float(v) for k, v in c.hp.items()}
    tot_v = tot_a = tot_e = 0
    for h in range(2):
        K = c.Ks[h]
        m, _ = ar.effective(c.allowed[h], K, c.actions[h])
        on = ar.bits(m, K)
        for b in c.rows(h, None):
            net = h * c.C + int(c.cmds[h, b])
            raw = L[net, b, :K]
            xb = raw if c.rk(h) is None else ordinal_ref.ordinal_logits(raw, c.rk(h))
            keep = torch.from_numpy(np.flatnonzero(on[b]))
            dist = torch.distributions.Categorical(logits=xb.index_select(0, keep))
            lp_ = dist.log_prob(torch.tensor(int(np.flatnonzero(np.flatnonzero(on[b]) == c.actions[h, b])[0])))
            ratio = torch.exp(lp_ - float(c.old_lp[h, b]))
            A, ov, R, v = float(c.adv[h, b]), float(c.old_v[h, b]), float(c.rets[h, b]), V[net, b]
            tot_a = tot_a - torch.min(ratio * A, torch.clamp(ratio, 1 - hp["clip"], 1 + hp["clip"]) * A)
            vpc = ov + (v - ov).clamp(-hp["clip"], hp["clip"])
            tot_v = tot_v + 0.5 * torch.max((v - R) ** 2, (vpc - R) ** 2)
            tot_e = tot_e + dist.entropy()
            assert abs(float(lp_.detach()) - out["logp"][h, b]) <= 1e-12 and abs(float(dist.entropy().detach()) - out["entropy"][h, b]) <= 1e-12
    total = (hp["value_coeff"] * tot_v + hp["clip_coeff"] * tot_a - hp["ent_coeff"] * tot_e) * hp["inv_b"]
    total.backward()
    assert abs(float(total.detach()) - out["total"]) <= 1e-12 * max(1.0, abs(out["total"]))
    assert np.abs(L.grad.numpy() - out["dlogits"]).max() <= 1e-12
    assert np.abs(V.grad.numpy() - out["dvalues"]).max() <= 1e-12
    if c.B > 1:
        assert np.abs(out["dlogits"]).max() > 1e-4


@pytest.mark.parametrize("words", ["all", "empty"])
@pytest.mark.parametrize("g", SMALL, ids=GRID_ID)
def test_all_bits_set_is_the_existing_loss_reference_bit_for_bit(g, words):
    c = case_of(g, words)
    out = ref_loss(c)
    base = lp.run_loss(c, X64())
    ml, mv = lp.written(c)
    assert np.array_equal(flat_dl(c, out["dlogits"])[ml], base["dlogits"][ml])
    dv = np.zeros(c.values.size)
    for n in range(2 * c.C):
        dv[n * c.v_ns: n * c.v_ns + c.B * c.ldv: c.ldv] = out["dvalues"][n]
    assert np.array_equal(dv[mv], base["dvalues"][mv])
    assert [float(a) for a in out["losses"]] == [float(b) for b in base["losses"]]
    assert np.array_equal(out["stats"], np.stack(base["stats"], 1))
    assert not out["am_stats"][:, [0, 2, 3]].any()


def test_reference_statistics_and_one_allowed_bin():
    c = case_of((17, 4, (33, 3), False), "single")
    out = ref_loss(c)
    for h in range(2):
        rows = c.rows(h, None)
        assert (out["logp"][h, rows] == 0.0).all() and (out["entropy"][h, rows] == 0.0).all() and (out["ratio"][h, rows] == 1.0).all()
    assert not out["dlogits"].any()
    assert out["am_stats"][1, 1] == 1.0 and out["am_stats"][1, 0] == 1.0                   # one bin per counted row
    # the pressure is the forbidden mass of the unmasked head; a foreign action is OR-ed in and counted
    c = case_of((17, 4, (33, 3), False))
    h, b = 0, int(c.rows(0, None)[0])
    on = ar.bits(ar.effective(c.allowed[h], 33)[0], 33)[b]
    x = c.own_logits(h, np.asarray([b])).astype(F8)[0]
    p = np.exp(x - x.max()); p /= p.sum()
    lg, vv = c.dense()
    one = ap.am_row(X64(), x[None], c.actions[h, [b]], *(np.zeros(1) for _ in range(5)), (0.1, 0.5, 1.0, 0.01, 1.0), c.allowed[h, b])[2]
    assert abs(float(one["press"][0]) - p[~on].sum()) < 1e-12
    c.actions[h, b] = int(np.flatnonzero(~on)[0])
    out = ref_loss(c)
    assert out["am_stats"][0, 3] == 1.0 and np.isfinite(out["logp"][h, b]) and np.isfinite(out["dlogits"]).all()


def test_sampling_rule_of_the_reference():
    raw = np.log(np.array([[0.1, 0.2, 0.3, 0.4], [0.25, 0.25, 0.25, 0.25]]))
    q = np.ones((2, 4))
    act, lp_, margin = ar.sample(raw, q, np.array([0b0111, 0b1010], np.int64), 4)
    assert act.tolist() == [2, 1]                                          # greedy: the first largest ALLOWED probability
    assert abs(lp_[0] - np.log(0.3 / 0.6)) < 1e-15 and abs(lp_[1] - np.log(0.5)) < 1e-15 and margin[1] == 0.0
    act, _l, _m = ar.sample(raw, np.array([[1.0, 1.0, 100.0, 1.0]] * 2), np.array([0b0111, 0], np.int64), 4)
    assert act.tolist() == [1, 0]                                          # q divides; the empty word is unmasked
    assert ar.sample(raw, q, np.array([0b1000, 0b0001], np.int64), 4)[2].tolist() == [np.inf, np.inf]
    # with a fixed seed the margin leaves out at most 1 of 4096 rows in float64 (the GPU test's condition is 1 %)
    for K in (3, 33, 64):
        r = np.random.RandomState(50 + K)
        x = 2.0 * r.standard_normal((4096, K))
        qq = r.exponential(1.0, (4096, K))
        assert (ar.sample(x, qq, ap.random_words(r, 4096, K), K)[2] < 1e-4).sum() <= 1


def test_note_and_place_words_statements():
    tens = [np.zeros(5, np.int64), None, np.zeros(5, np.int64)]
    ar.note(tens, [4, 0, 5], [2 ** 63, 7, 9], 4)
    assert tens[0].tolist() == [0, 0, 0, 0, -2 ** 63] and tens[2].tolist() == [0] * 5      # slot 5 > T: nothing is written
    srcs = [np.arange(10, 15, dtype=np.int64), None]
    got = ar.place_words(srcs, np.array([[0, 3], [1, 2]]), np.array([[1, 0], [0, 1]]), 2, 4, np.full((2, 2), -9, np.int64))
    assert got.tolist() == [[13, 10], [0, 0]]


# ----------------------------------------------------------------------------- the (value, error) row body
@pytest.mark.parametrize("g", GRID, ids=GRID_ID)
def test_parity_body_equals_the_reference_and_the_emulation_passes(g):
    c = case_of(g)
    ref = ap.run_am(c, XVE)
    x64 = ap.run_am(c, X64())
    out = ref_loss(c)
    ml, _mv = lp.written(c)
    assert np.abs(flat_dl(c, out["dlogits"])[ml] - x64["dlogits"][ml]).max() <= 1e-12
    assert max(abs(float(a) - float(b)) for a, b in zip(out["losses"], x64["losses"])) <= 1e-12
    assert np.abs(np.stack([np.reshape(t, -1) for t in x64["am_stats"]], 1) - out["am_stats"]).max() <= 1e-12
    assert np.abs(np.stack([np.reshape(t, -1) for t in x64["stats"]], 1) - out["stats"]).max() <= 1e-12
    for order in ("tree", "seq"):
        worst, n_amb = ap.check_am(c, ap.emulate_am(c, order), ref, "%s emulation %s" % (c.tag(), order), quiet=True)
        assert worst <= 1.0 and n_amb <= 1


@pytest.mark.parametrize("mut", ["mask_off", "no_or", "mask_before_ord"])
def test_mask_mutants_are_rejected(mut):
    """The bound tells the kernel's statements from: no mask at all, no OR of the taken action, the mask applied in rank space."""
    c = case_of((17, 4, (33, 3), mut == "mask_before_ord"))
    if mut == "no_or":
        on = ar.bits(ar.effective(c.allowed[0], 33)[0], 33)
        b = int(c.rows(0, None)[0])
        c.actions[0, b] = int(np.flatnonzero(~on[b])[0])
    ref = ap.run_am(c, XVE)
    with np.errstate(all="ignore"):
        got = ap.emulate_am(c, "tree", mut=(mut,))
    with pytest.raises(AssertionError):
        ap.check_am(c, got, ref, mut, quiet=True)


# ----------------------------------------------------------------------------- words and configuration
def test_allowed_word_and_from_controls():
    from cadre_amd.actmask import all_word, allowed_from_controls, allowed_word, check_word, word_i64, word_pair
    assert allowed_word([0, 2], 3) == 0b101 and allowed_word(range(33), 33) == all_word(33) == 2 ** 33 - 1
    assert allowed_word([63], 64) == 2 ** 63 and word_i64(2 ** 63) == -2 ** 63 and word_i64(all_word(64)) == -1
    assert all_word(64) == 2 ** 64 - 1 and ar.to_u64(np.array([word_i64(2 ** 63)], np.int64))[0] == np.uint64(2 ** 63)
    for bad in ([], [3], [-1], [1.5], [True]):
        with pytest.raises(ValueError, match="allowed_word"):
            allowed_word(bad, 3)
    with pytest.raises(ValueError, match="K="):
        allowed_word([0], 65)
    steer = {i: (i - 16) / 16.0 for i in range(33)}
    assert allowed_from_controls(steer, -0.5, 0.5) == allowed_word(range(8, 25), 33)
    thr = {0: [0, 0], 1: [0, 1], 2: [0.6, 0]}
    assert allowed_from_controls(thr, 0.0, 0.0) == 0b011                      # no "accelerate" bin
    assert allowed_from_controls(thr, 0, 1, key=lambda v: v[1]) == 0b111 and allowed_from_controls([0.0, 0.5, 1.0], 0.4, 2) == 0b110
    assert allowed_from_controls([float(k) for k in range(64)], 63, 63) == 2 ** 63
    with pytest.raises(ValueError, match="no bin"):
        allowed_from_controls(steer, 2.0, 3.0)
    with pytest.raises(ValueError, match="0 .. K-1"):
        allowed_from_controls({1: 0.0, 2: 1.0}, 0, 1)
    assert check_word(-1, 3) == 2 ** 64 - 1 and check_word(2 ** 63, 64) == 2 ** 63
    for bad, K in ((0, 3), (0b1000, 3), (2 ** 64, 64), (1.0, 3), (True, 3), ("1", 3)):
        with pytest.raises(ValueError):
            check_word(bad, K)
    assert word_pair((5, 1), (33, 3)) == (5, 1)
    for bad in (5, (5,), (5, 1, 1), "ab", (5, 0b1000)):
        with pytest.raises(ValueError):
            word_pair(bad, (33, 3))


def test_config_and_section_object():
    from cadre_amd.actmask import ActionMasks, actmask_config, actmask_stats_text
    rule = lambda obs, info: (1, 1)
    assert actmask_config(None) is None and actmask_config(rule) == dict(rule=rule) and actmask_config(dict(rule=rule)) == dict(rule=rule)
    for bad in (5, "rule", dict(), dict(rule=3), dict(rule=rule, coeff=1.0), [rule]):
        with pytest.raises(ValueError, match="action_mask"):
            actmask_config(bad)
    am = ActionMasks(rule, (33, 3), "cpu")
    assert am.words({}, None) == (1, 1) and am.summary() is None
    with pytest.raises(ValueError, match="allows none"):
        ActionMasks(lambda o, i: (1, 0b1000), (33, 3), "cpu").words({}, None)
    with pytest.raises(ValueError, match="pair"):
        ActionMasks(lambda o, i: 7, (33, 3), "cpu").words({}, None)
    with pytest.raises(ValueError, match="no configuration"):
        ActionMasks(None, (33, 3), "cpu")
    text = actmask_stats_text(dict(actmask=dict(masked_share=(1.0, 0.5), allowed_bins=(17.0, 2.5), pressure=(0.25, 0.125), forced_rows=(0.0, 1.0))))
    assert "masked rows: 1.00/0.50" in text and "allowed bins: 17.0/2.5" in text and "forced: 0/1" in text


@pytest.mark.parametrize("key", ["demo_mix", "suggest", "self_imitation", "smoothness", "sample_reuse", "aux_phase"])
def test_runner_refuses_the_loss_twins(key):
    from cadre_amd.actmask import actmask_runner
    with pytest.raises(ValueError, match="action_mask excludes train_cfg.%s" % key):
        actmask_runner(None, lambda o, i: (1, 1), **{key: dict(x=1)})


def test_runner_refusals_say_why():
    import types
    from cadre_amd.actmask import actmask_runner
    from cadre_amd.ppo_agent import train
    rule = lambda o, i: (1, 1)
    agent = types.SimpleNamespace(arena=types.SimpleNamespace(n_out=(33, 3)), device="cpu")
    assert actmask_runner(agent, None, demo_mix=dict(x=1)) is None               # key absent: nothing is checked, nothing runs
    with pytest.raises(ValueError, match="fused_gather=True"):
        actmask_runner(agent, rule, fused_gather=False)
    for kw in (dict(checkpoint_interval=2), dict(resume_from="x.pt")):
        with pytest.raises(ValueError, match="not part of a checkpoint"):
            actmask_runner(agent, rule, **kw)
    assert actmask_runner(agent, dict(rule=rule)).n_out == (33, 3)
    # the training loops read the same keys
    assert train.action_masks(agent, dict(lr=1.0)) is None
    with pytest.raises(ValueError, match="self_imitation"):
        train.action_masks(agent, dict(action_mask=rule, self_imitation=dict(x=1)))
    with pytest.raises(ValueError, match="not part of a checkpoint"):
        train.action_masks(agent, dict(action_mask=rule), True, 2, None)
    with pytest.raises(ValueError, match="sample_reuse"):
        train._check_actmask(object(), None, None, object(), None, None)
    train._check_actmask(None, object(), object(), object(), object(), object(), False)   # no masks: nothing is refused
    # ensemble evaluation and the learner's mode list
    from cadre_amd.ppo_agent.evaluate import EnsembleEvaluator, ensemble_act_batch
    with pytest.raises(ValueError, match="ensemble"):
        ensemble_act_batch([object()], [{}], allowed=[(1, 1)])
    with pytest.raises(ValueError, match="ensemble evaluation takes no allowed"):     # the evaluator's own act, reached directly
        EnsembleEvaluator.act(object.__new__(EnsembleEvaluator), [{}], allowed=[(1, 1)])


# ----------------------------------------------------------------------------- storages
def test_storage_allocates_lazily_and_checks_its_arguments():
    from cadre_amd.ppo_agent.storage import RolloutStorage
    s = RolloutStorage(4, 1, 6, 2, 6, True, 0.9, 0.9)
    obs, one = torch.zeros(2, 6), torch.zeros(1)
    s.insert(obs, one, one, one, 0.0, one, None, 0)
    assert getattr(s, "allowed", None) is None                       # never saw a word: no such tensor
    s.insert(obs, one, one, one, 0.0, one, None, 0, allowed=2 ** 63 + 1)
    assert s.allowed.dtype == torch.int64 and s.allowed.tolist() == [0, -2 ** 63 + 1, 0, 0, 0]
    for _ in range(4):                                               # the cursor wraps at T + 1: the stale word is overwritten
        s.insert(obs, one, one, one, 0.0, one, None, 0)
    assert s.step == 1 and s.allowed.tolist() == [0, -2 ** 63 + 1, 0, 0, 0]
    s.insert(obs, one, one, one, 0.0, one, None, 0)
    assert s.allowed.tolist() == [0] * 5
    for bad in (0, 2 ** 64, 1.0, True, "1", -2 ** 63 - 1):
        with pytest.raises(ValueError, match="allowed word"):
            s.insert(obs, one, one, one, 0.0, one, None, 0, allowed=bad)
    assert s.step == 2                                               # a refused insert moved nothing
    for bad, K in ((0b1000, 3), (2 ** 33, 33), (-8, 3)):            # no bit among the head's K bins: refused where K is given
        with pytest.raises(ValueError, match="allows none"):
            s.insert(obs, one, one, one, 0.0, one, None, 0, allowed=bad, allowed_bins=K)
    assert s.step == 2 and s.allowed.tolist() == [0] * 5
    s.insert(obs, one, one, one, 0.0, one, None, 0, allowed=5)
    s.to("cpu")
    assert s.allowed.tolist() == [0, 0, 5, 0, 0]                     # .to() carries it
    plain = RolloutStorage(4, 1, 6, 2, 6, True, 0.9, 0.9)
    plain.to("cpu")
    assert not hasattr(plain, "allowed")
    pairs = [(RolloutStorage(4, 1, 6, 2, 6, True, 0.9, 0.9), RolloutStorage(4, 1, 6, 2, 6, True, 0.9, 0.9))]
    args = ([None], [[0.0, 0.0]], [[1.0, 1.0]], [0])
    for bad in ([(1, 1), (1, 1)], [(1,)], [5], [(1, 0)], torch.zeros(1, 2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="allowed"):
            RolloutStorage.insert_batch(pairs, *args, allowed=bad)
    for bad in ([(2 ** 33, 1)], [(1, 0b1000)]):
        with pytest.raises(ValueError, match="allows none"):
            RolloutStorage.insert_batch(pairs, *args, allowed=bad, n_out=(33, 3))
    assert not hasattr(pairs[0][0], "allowed")


# ----------------------------------------------------------------------------- the entry points, by name
NAMES = ("cadre_sample_am", "cadre_sample_rows_am", "cadre_categorical_eval_am", "cadre_allowed_note", "cadre_allowed_rows",
         "cadre_ppo_am_loss")


def test_entry_points_declared_bound_exported():
    from cadre_amd import build, hip
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    L = hip.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in hip.SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr), name
    assert "actmask.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "cadre_amd", "csrc", "actmask.h"))
    assert L.cadre_abi_version() == hip.ABI_VERSION == 15                  # entry points only added
    assert int(re.search(r"#define CADRE_AM_STATS_FIELDS (\d+)", hdr).group(1)) == hip.AM_STATS_FIELDS == 4
    assert len(hip.SYMBOLS["cadre_ppo_am_loss"]) == len(hip.SYMBOLS["cadre_ppo_loss_ord"]) + 4
    assert len(hip.SYMBOLS["cadre_sample_am"]) == len(hip.SYMBOLS["cadre_sample_ord"]) + 1
    assert len(hip.SYMBOLS["cadre_sample_rows_am"]) == len(hip.SYMBOLS["cadre_sample_rows_ord"]) + 1
    assert hip.SYMBOLS["cadre_allowed_rows"] == hip.SYMBOLS["cadre_suggest_rows"]


def am_args(**over):
    """Arguments of cadre_ppo_am_loss that pass every check (pointers are never dereferenced on the host)."""
    p = 64
    a = dict(logits=p, ldl=64, l_ns=64, values=p, ldv=1, v_ns=1, actions=p, commands=p, old_values=p, returns=p, old_logp=p, adv=p,
             B=8, C=4, nS=33, nT=3, hp=None, clip=0.1, vc=0.1, cc=1.0, ec=0.01, inv_b=0.25, losses=p, dl=p, dv=p, scratch=p, poison=None,
             stats_row=None, F=0, stats_scratch=None, target_kl=0.0, stop=None, ord=p, allowed=p, am_stats=None, am_F=0,
             am_scratch=None, stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("over,msg", [
    (dict(allowed=None), "null allowed"), (dict(ord=None), "rank table"), (dict(B=0), "bad argument"), (dict(ldl=32), "bad argument"),
    (dict(nS=65), "bad argument"), (dict(logits=None), "bad argument"), (dict(am_stats=64, am_F=3, am_scratch=64), "mask stats"),
    (dict(am_stats=64, am_F=4), "mask stats"), (dict(stats_row=64, F=8), "stats argument"), (dict(hp=12), "hyper-parameter block"),
])
def test_loss_entry_refuses_before_any_launch(over, msg):
    from cadre_amd import hip
    L = hip.lib()
    rc = L.cadre_ppo_am_loss(*am_args(**over))
    assert rc < 0 and msg in L.cadre_last_error().decode(), L.cadre_last_error().decode()


def test_small_entries_refuse_before_any_launch():
    from cadre_amd import hip
    L = hip.lib()
    assert L.cadre_sample_am(64, 64, 64, 64, 4, 33, 64, 64, 64, None, None) < 0 and "allowed" in L.cadre_last_error().decode()
    assert L.cadre_sample_am(64, 64, 64, 64, 4, 33, 64, 64, None, 64, None) < 0 and L.cadre_sample_am(64, 32, 64, 64, 4, 33, 64, 64, 64, 64, None) < 0
    assert L.cadre_sample_am(64, 64, 64, 64, 0, 33, 64, 64, 64, 64, None) < 0 and L.cadre_sample_am(64, 64, 64, 64, 4, 65, 64, 64, 64, 64, None) < 0
    rows = lambda **o: list(dict(dict(O3=64, ldo=64, z_str=640, pos=64, cmd=64, N=4, C=4, q=64, K0=33, K1=3, action=64, logp=64, value=64,
                                      ord=64, allowed=64, stream=None), **o).values())
    for o in (dict(allowed=None), dict(ord=None), dict(N=0), dict(C=17), dict(K0=65), dict(ldo=32), dict(z_str=64), dict(q=None)):
        assert L.cadre_sample_rows_am(*rows(**o)) < 0, o
    assert L.cadre_categorical_eval_am(64, 64, 64, 4, 33, 64, 64, 64, None, None) < 0
    assert L.cadre_categorical_eval_am(64, 64, 64, 4, 33, 64, 64, None, 64, None) < 0 and L.cadre_categorical_eval_am(64, 16, 64, 4, 33, 64, 64, 64, 64, None) < 0
    assert L.cadre_allowed_note(None, 64, 64, 2, 8, None) < 0 and L.cadre_allowed_note(64, 64, 64, 0, 8, None) < 0
    assert L.cadre_allowed_note(64, 64, None, 2, 8, None) < 0 and L.cadre_allowed_note(64, 64, 64, 2, 0, None) < 0
    assert L.cadre_allowed_rows(64, 3, 64, 4, 8, None, 8, 64, None) < 0 and L.cadre_allowed_rows(64, 4, 64, 5, 8, None, 8, 64, None) < 0
    assert L.cadre_allowed_rows(64, 2, 64, 4, 8, None, 8, None, None) < 0


def test_set_loss_takes_the_mode_and_refuses_a_near_miss():
    import types
    from cadre_amd.learner import PPOLearnerHIP
    stub = types.SimpleNamespace(loss_mode="ppo", _hp_on=False)
    PPOLearnerHIP.set_loss(stub, "ppo+mask")
    assert stub.loss_mode == "ppo+mask"
    with pytest.raises(ValueError, match="set_loss: mode 'ppo\\+masks'"):
        PPOLearnerHIP.set_loss(stub, "ppo+masks")
    assert stub.loss_mode == "ppo+mask"
    key = PPOLearnerHIP._mode_key(types.SimpleNamespace(loss_mode="ppo+mask", stats=False, target_kl=None, _adaptive=None, _hp_on=False,
                                                         a=types.SimpleNamespace(ord=None), consensus=False,
                                                         _loss_stats=lambda: False))
    assert key == (("mask",),)                                       # a mode of its own among the graph keys
