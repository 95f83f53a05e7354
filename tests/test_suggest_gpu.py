"""GPU: exploration suggestions (csrc/suggest.hip, cadre_amd/suggest.py).

  * cadre_suggest_mark against the numpy scan of tests/suggest_ref.py, torch.equal;
  * cadre_suggest_note through RolloutStorage.insert_batch(events=), and the launches of a storage that never saw an event;
  * cadre_suggest_rows against tests/suggest_ref.place_kinds;
  * cadre_ppo_sug_loss: every output element within the running first-order bound of tests/suggest_parity.py, and the exact
    statements of the header (kind 0 == cadre_ppo_loss_ord bit for bit, coefficient 0, logits equal to the prior row, repeatability);
  * end to end: the section's gradient against float64 autograd of the mixed loss, a train_vec run with a synthetic "blocked" event,
    the direction of the suggestion term alone, and the refused combinations."""
import os
import types

import numpy as np
import pytest
import torch

from tests import loss_parity as lp
from tests import suggest_parity as sp
from tests import suggest_ref
from tests.loss_parity import F4, SENT, XVE

pytestmark = pytest.mark.gpu
F_PPO, F_SUG = 8, 4
DECOY = 0.77
GUARD = 8


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def hip():
    from cadre_amd import hip as h
    h.lib()
    return h


# ----------------------------------------------------------------------------- cadre_suggest_mark
def mark_storage(r, T, Z, k, with_tl):
    """events / masks / time_limits of one storage: the placements the header names, then random ones."""
    ev = np.zeros(T + 1, np.int32)
    masks = np.ones(T + 1, np.float32)
    tl = np.zeros(T + 1, np.float32)
    ev[T] = 1                                                        # (slot T is never read)
    if T >= 1:
        ev[T - 1] = 1 + k % Z                                        # an event on the last row
        if k % 2 == 0:
            ev[0] = Z                                                # and on row 0
    if T >= 7:
        ev[5], masks[5] = 1, 0.0
        ev[3], masks[3] = Z, 0.0                                     # two events closer than a horizon
        ev[1] = Z + 1                                                # ignored codes
        ev[2] = -1
    if T >= 128:
        for t in r.randint(8, T - 1, 12):
            ev[t], masks[t] = r.randint(1, Z + 1), 0.0
        for t in r.randint(8, T - 1, 6):
            masks[t] = 0.0                                           # episode ends without an event, some inside a window
        for t in r.randint(8, T - 1, 5):
            tl[t] = 1.0
        e = int(r.randint(40, T - 1))
        ev[e], masks[e - 1], tl[e - 2] = 1, 0.0, 1.0                 # an end and a time limit right inside a window
    return ev, masks, (tl if with_tl else None)


@pytest.mark.parametrize("T", [1, 2, 7, 128, 200])
@pytest.mark.parametrize("n,Z", [(1, 1), (2, 8), (5, 8), (5, 1)])
def test_suggest_mark(hip, T, n, Z):
    r = np.random.RandomState(100 * T + 10 * n + Z)
    hz = np.zeros((2, Z + 1), np.int32)
    hz[:, 0] = 99                                                    # entry 0 is unused
    hz[:, 1:] = np.array([1, 3, T + 5])[r.randint(0, 3, (2, Z))]
    hz[0, 1], hz[1, Z] = 3, T + 5
    if Z == 8:
        hz[0, 4] = 0                                                 # a kind this head has no window for
    keep, rows, want = [], [], []
    for k in range(n):
        ev, masks, tl = mark_storage(r, T, Z, k, with_tl=(k % 2 == 0))
        out = torch.full((T + GUARD,), -5, dtype=torch.int32, device="cuda")
        d = (dev(ev), dev(masks.reshape(-1, 1)), None if tl is None else dev(tl.reshape(-1, 1)), out)
        keep.append(d)
        rows.append([d[0].data_ptr(), d[1].data_ptr(), 0 if tl is None else d[2].data_ptr(), out.data_ptr()])
        want.append(suggest_ref.mark_scan(ev, masks, tl, k & 1, T, Z, hz))
    table, hz_d = dev(np.array(rows, np.int64)), dev(hz)
    hip.check(hip.lib().cadre_suggest_mark(table.data_ptr(), n, T, Z, hz_d.data_ptr(), hip.stream()), "cadre_suggest_mark")
    torch.cuda.synchronize()
    for k in range(n):
        got = keep[k][3].cpu()
        assert torch.equal(got[:T], torch.from_numpy(want[k])), (k, got[:T].tolist(), want[k].tolist())
        assert bool((got[T:] == -5).all()), "the guard band behind suggest was written"
    assert any(w.max() > 0 for w in want)
    if T >= 128:
        assert all((w == 0).any() for w in want)                     # (marked and unmarked rows both occur)


# ----------------------------------------------------------------------------- cadre_suggest_note / insert_batch(events=)
def small_storages(N, T=4):
    from ppo_agent.storage import RolloutStorage
    return [(RolloutStorage(T, 1, 530, 8, 530, True, 0.99, 0.95, device="cuda:0"),
             RolloutStorage(T, 1, 530, 8, 530, True, 0.99, 0.95, device="cuda:0")) for _ in range(N)]


class Outputs(types.SimpleNamespace):
    """What insert_batch reads of act_batch's result: one buffer per output kind, len() = environments."""

    def __len__(self):
        return self.feat.shape[0]


def fake_outputs(N, seed):
    r = np.random.RandomState(seed)
    return Outputs(feat=dev(r.standard_normal((N, 8, 544)).astype(np.float32)),
                                 action=dev(r.randint(0, 3, (N, 2)).astype(np.int64)),
                                 logp=dev(r.standard_normal((N, 2)).astype(np.float32)),
                                 value=dev(r.standard_normal((N, 2)).astype(np.float32)))


@pytest.mark.parametrize("N", [1, 3])
def test_insert_batch_events(hip, N):
    from ppo_agent.storage import RolloutStorage
    T = 4
    st = small_storages(N, T)
    plain = small_storages(N, T)
    want = [[np.zeros(T + 1, np.int32), np.zeros(T + 1, np.int32)] for _ in range(N)]
    steps = [None, [3] * N, [(1, 2)] + [0] * (N - 1), None, [(0, 7)] * N, [5] * N, None]     # 7 steps: the cursor wraps at T + 1
    for i, evs in enumerate(steps):
        outs = fake_outputs(N, i)
        args = ([[0.5, 0.25]] * N, [[1.0, 1.0]] * N, [1] * N)
        n0 = hip.N_CALLS
        RolloutStorage.insert_batch(plain, outs, *args)
        assert hip.N_CALLS - n0 == 1                                 # a storage that never got an event: today's single launch
        slot = st[0][0].step
        n0 = hip.N_CALLS
        RolloutStorage.insert_batch(st, outs, *args, **({} if evs is None else dict(events=evs)))
        seen = i >= 1
        assert hip.N_CALLS - n0 == (2 if seen else 1)
        for e in range(N):
            pair = (0, 0) if evs is None else (evs[e] if isinstance(evs[e], tuple) else (evs[e], evs[e]))
            want[e][0][slot], want[e][1][slot] = pair
    torch.cuda.synchronize()
    for e in range(N):
        for h in range(2):
            assert getattr(plain[e][h], "events", None) is None and not hasattr(plain[e][h], "suggest")
            assert st[e][h].events.dtype == torch.int32 and st[e][h].events.cpu().tolist() == want[e][h].tolist(), (e, h)
            assert st[e][h].step == len(steps) % (T + 1)
            for k in ("action", "rewards", "masks", "_obs"):        # the rows themselves are today's
                assert torch.equal(getattr(st[e][h], k), getattr(plain[e][h], k))
    with pytest.raises(ValueError, match="event"):
        RolloutStorage.insert_batch(st, fake_outputs(N, 0), [[0.5, 0.25]] * N, [[1.0, 1.0]] * N, [1] * N, events=[-1] * N)
    moved = small_storages(1, T)[0][0]
    moved.insert(torch.zeros(8, 530, device="cuda"), torch.zeros(1), torch.zeros(1), torch.zeros(1), 0.0, torch.ones(1), None, 0, event=2)
    moved.to("cpu")
    assert moved.events.device.type == "cpu" and moved.events.tolist() == [2, 0, 0, 0, 0] and moved.suggest.device.type == "cpu"


# ----------------------------------------------------------------------------- cadre_suggest_rows
@pytest.mark.parametrize("Bw,n_src", [(1, 2), (17, 2), (1, 6), (17, 6)])
@pytest.mark.parametrize("sorted_pos", [True, False])
def test_suggest_rows(hip, Bw, n_src, sorted_pos):
    r = np.random.RandomState(7 * Bw + n_src + sorted_pos)
    T, Bt = 23, Bw * n_src // 2
    sug = [r.randint(0, 4, T).astype(np.int32) for _ in range(n_src)]
    if n_src > 2:
        sug[3] = None                                                # a storage without marks among the sources
    idx = r.randint(0, T, (n_src, Bw)).astype(np.int64)
    pos = np.stack([r.permutation(Bt) for _ in range(2)]).astype(np.int32) if sorted_pos else None
    if Bw > 1:
        idx[0, 2], idx[1, 3] = T, -1                                 # out-of-range indices: nothing is written
        if pos is not None:
            pos[0, 5], pos[1, 0] = Bt, -1                            # out-of-range positions: nothing is written
    init = np.full((2, Bt), -9, np.int32)
    want = suggest_ref.place_kinds(sug, idx, pos, Bt, T, init)
    keep = [None if s is None else dev(s) for s in sug]
    table = dev(np.array([0 if k is None else k.data_ptr() for k in keep], np.int64))
    out = torch.full((2 * Bt + GUARD,), -9, dtype=torch.int32, device="cuda")
    idx_d, pos_d = dev(idx), (None if pos is None else dev(pos))
    hip.check(hip.lib().cadre_suggest_rows(table.data_ptr(), n_src, idx_d.data_ptr(), Bw, T, None if pos is None else pos_d.data_ptr(),
                                           Bt, out.data_ptr(), hip.stream()), "cadre_suggest_rows")
    got = out.cpu().numpy()
    assert np.array_equal(got[:2 * Bt].reshape(2, Bt), want) and (got[2 * Bt:] == -9).all()
    if Bw > 1:
        assert (want == -9).any() and (want >= 0).any()               # the sentinel stayed where nothing was addressed


# ----------------------------------------------------------------------------- cadre_ppo_sug_loss
class SugLaunch:
    """Device operands of a SugCase and fresh sentinel-filled outputs."""

    def __init__(self, hip, case):
        self.hip, self.case, c = hip, case, case.base
        self.nblk = (c.B + 15) // 16
        self.d = {k: dev(getattr(c, k)) for k in ("logits", "values", "actions", "cmds", "old_v", "rets", "old_lp", "adv")}
        self.ord = dev(c.ord)
        self.prior = dev(case.prior)
        hp = torch.zeros(hip.HP_FIELDS, dtype=torch.float64)
        for k in ("clip", "value_coeff", "clip_coeff", "ent_coeff"):
            hp[hip.HP[k]] = float(c.hp[k])
        hp[hip.HP["lr"]], hp[hip.HP["max_grad_norm"]], hp[hip.HP["lr_min"]], hp[hip.HP["lr_max"]], hp[hip.HP["lr_factor"]] = 3e-4, 250.0, 1e-6, 1e-2, 1.5
        hp[hip.HP_SUGGEST_COEFF] = float(case.sug_coeff)
        self.block = hp.cuda()

    def outputs(self):
        c = self.case.base
        f = lambda n, v=float(SENT): torch.full((n,), v, device="cuda")
        o = dict(dl=f(c.logits.size), dv=f(c.values.size), losses=f(8), sug_losses=f(8), scratch=f(4 + 6 * self.nblk, 3.0),
                 stats=torch.zeros(2, F_PPO, device="cuda"), sscratch=torch.zeros(2 * self.nblk * 6, device="cuda"),
                 sug_stats=f(2 * F_SUG + GUARD), sug_scratch=f(2 * self.nblk * 4 + GUARD, 11.0))      # (needs no initialisation)
        o["scratch"][0] = 0.0
        return o

    def head(self):
        c, d = self.case.base, self.d
        return [d["logits"].data_ptr(), c.ldl, c.l_ns, d["values"].data_ptr(), c.ldv, c.v_ns, d["actions"].data_ptr(), d["cmds"].data_ptr(),
                d["old_v"].data_ptr(), d["rets"].data_ptr(), d["old_lp"].data_ptr(), d["adv"].data_ptr()]

    def sug(self, o, kind, use_hp, stats, sug_coeff=None, hp_over=None, prior=None, poison=None):
        case, c, L = self.case, self.case.base, self.hip.lib()
        hp = dict(c.hp, **(hp_over or {}))
        byval = [float(hp[k]) for k in ("clip", "value_coeff", "clip_coeff", "ent_coeff")]
        sc = float(case.sug_coeff if sug_coeff is None else sug_coeff)
        rc = L.cadre_ppo_sug_loss(*self.head(), kind.data_ptr(), (self.prior if prior is None else prior).data_ptr(), case.Z, c.B, c.C,
                                  c.Ks[0], c.Ks[1], self.block.data_ptr() if use_hp else None, *([DECOY] * 4 if use_hp else byval),
                                  float(hp["inv_b"]), DECOY if use_hp else sc, o["losses"].data_ptr(), o["sug_losses"].data_ptr(),
                                  o["dl"].data_ptr(), o["dv"].data_ptr(), o["scratch"].data_ptr(), o["sug_scratch"].data_ptr(), poison,
                                  o["stats"].data_ptr() if stats else None, F_PPO, o["sscratch"].data_ptr() if stats else None, 0.0, None,
                                  o["sug_stats"].data_ptr(), F_SUG, self.ord.data_ptr(), self.hip.stream())
        self.hip.check(rc, "cadre_ppo_sug_loss")
        return self.collect(o, stats)

    def ord_loss(self, o, use_hp, stats, hp_over=None):
        c, L = self.case.base, self.hip.lib()
        hp = dict(c.hp, **(hp_over or {}))
        byval = [float(hp[k]) for k in ("clip", "value_coeff", "clip_coeff", "ent_coeff")]
        rc = L.cadre_ppo_loss_ord(*self.head(), c.B, c.C, c.Ks[0], c.Ks[1], self.block.data_ptr() if use_hp else None,
                                  *([DECOY] * 4 if use_hp else byval), float(hp["inv_b"]), o["losses"].data_ptr(), o["dl"].data_ptr(),
                                  o["dv"].data_ptr(), o["scratch"].data_ptr(), None, o["stats"].data_ptr() if stats else None, F_PPO,
                                  o["sscratch"].data_ptr() if stats else None, 0.0, None, self.ord.data_ptr(), self.hip.stream())
        self.hip.check(rc, "cadre_ppo_loss_ord")
        return self.collect(o, stats)

    def collect(self, o, stats):
        torch.cuda.synchronize()
        assert bool((o["losses"][3:] == float(SENT)).all()) and bool((o["sug_losses"][1:] == float(SENT)).all()), "a loss beyond its slot was written"
        assert bool((o["sug_stats"][2 * F_SUG:] == float(SENT)).all()) and bool((o["sug_scratch"][2 * self.nblk * 4:] == 11.0).all())
        assert int(o["scratch"][:1].view(torch.int32)[0].item()) == 0, "the arrival counter was not reset"
        got = dict(dlogits=host(o["dl"]), dvalues=host(o["dv"]), losses=host(o["losses"])[:3], sug_losses=host(o["sug_losses"])[:1],
                   sug_stats=host(o["sug_stats"])[:2 * F_SUG].reshape(2, F_SUG))
        if stats:
            got["stats"] = host(o["stats"])
        return got


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


GRID = [(0, "all", 1), (1, "alt", 8), (2, "all", 8), (3, "alt", 1), (4, "all", 8), (5, "alt", 8), (6, "alt", 8), (7, "all", 1),
        (8, "alt", 8), (9, "all", 8), (1, "none", 8), (6, "none", 1)]


@pytest.mark.parametrize("g", GRID, ids=lambda g: "case%d-%s-Z%d" % g)
def test_ppo_sug_loss_within_the_bound(hip, g):
    case = sp.SugCase(*g)
    ref = sp.run_sug(case, XVE)
    run = SugLaunch(hip, case)
    kind = dev(case.kind)
    first = None
    for use_hp, stats in ((False, True), (True, False), (True, True), (False, False)):
        got = run.sug(run.outputs(), kind, use_hp, stats)
        what = "cadre_ppo_sug_loss hp %s stats %d %s" % ("block" if use_hp else "NULL", stats, case.tag())
        _w, n_amb = sp.check_sug(case, got, ref, what, stats=stats)
        assert n_amb <= 1
        if first is None:
            first = got
        for k in ("dlogits", "dvalues", "losses", "sug_losses", "sug_stats"):      # the four forms and a second launch: equal bits
            assert np.array_equal(bits(got[k]), bits(first[k])), (what, k)
    marked = int((case.eff() != 0).sum())
    assert (marked == 0) == (g[1] == "none")
    if marked == 0:
        assert bits(first["sug_losses"])[0] == 0 and not first["sug_stats"].any()


@pytest.mark.parametrize("i", [1, 5, 6, 8])
def test_kind_zero_and_coefficient_zero_are_the_ppo_loss(hip, i):
    """Every kind 0 (also: only kinds outside 0 .. Z): bit-identical to cadre_ppo_loss_ord on the same buffers, with and without
    stats / the block, and sug_losses[0] is +0.  sug_coeff = 0 with rows marked: outputs compare equal."""
    case = sp.SugCase(i, "alt", 8)
    run = SugLaunch(hip, case)
    zero = torch.zeros(2, case.base.B, dtype=torch.int32, device="cuda")
    junk = zero.clone()
    junk[0, ::2], junk[1, 1::2] = -1, case.Z + 1
    for use_hp, stats in ((False, False), (False, True), (True, True)):
        want = run.ord_loss(run.outputs(), use_hp, stats)
        for kind in (zero, junk):
            got = run.sug(run.outputs(), kind, use_hp, stats)
            for k in ("dlogits", "dvalues", "losses") + (("stats",) if stats else ()):
                assert np.array_equal(bits(got[k]), bits(want[k])), (use_hp, stats, k)
            assert bits(got["sug_losses"])[0] == 0 and not got["sug_stats"].any()
    # coefficient 0, rows marked (by value; the block holds the case's coefficient, so hp stays NULL here)
    want = run.ord_loss(run.outputs(), False, True)
    got = run.sug(run.outputs(), dev(case.kind), False, True, sug_coeff=0.0)
    for k in ("dlogits", "dvalues", "losses", "stats"):
        assert (got[k] == want[k]).all(), k
    assert got["sug_losses"][0] == 0.0 and got["sug_stats"][:, 0].sum() > 0


def test_logits_equal_to_the_prior_row_give_exact_zeros(hip):
    """Categorical heads, clip_coeff = value_coeff = ent_coeff = 0: rows planted with raw logits bit-equal to their prior row have kl == 0
    and a dlogits row of (+-)0; the other marked rows do not."""
    case = sp.SugCase(1, "all", 8)                                   # B 15, K (33, 3), C 4, ldl 40, categorical
    c = case.base
    eff = case.eff()
    planted = []
    for h in range(2):
        for b in (0, 4, 8, 13):
            if c.row_ok(h, b) and eff[h, b] != 0:
                net = h * c.C + c.cmds[h, b]
                c.logits[net * c.l_ns + b * c.ldl: net * c.l_ns + b * c.ldl + c.Ks[h]] = case.prior[h, eff[h, b], :c.Ks[h]]
                planted.append((h, b))
    assert len(planted) >= 4
    run = SugLaunch(hip, case)
    zero_hp = dict(clip_coeff=F4(0.0), value_coeff=F4(0.0), ent_coeff=F4(0.0))
    # only the planted rows marked: kl of the launch is exactly 0
    only = np.zeros_like(case.kind)
    for h, b in planted:
        only[h, b] = case.kind[h, b]
    got = run.sug(run.outputs(), dev(only), False, False, hp_over=zero_hp)
    assert got["sug_losses"][0] == 0.0 and (got["sug_stats"][:, 1] == 0.0).all() and (got["sug_stats"][:, 2] == 0.0).all()
    assert got["sug_stats"][:, 0].sum() == len(planted)
    ml, _mv = lp.written(c)
    assert (got["dlogits"][ml] == 0.0).all()                         # every written element: (+-)0
    # every row marked: the planted rows still hold zeros, the others moved
    got = run.sug(run.outputs(), dev(case.kind), False, False, hp_over=zero_hp)
    for h in range(2):
        for b in range(c.B):
            if not c.row_ok(h, b):
                continue
            net = h * c.C + c.cmds[h, b]
            row = got["dlogits"][net * c.l_ns + b * c.ldl: net * c.l_ns + b * c.ldl + c.Ks[h]]
            if (h, b) in planted:
                assert (row == 0.0).all(), (h, b)
            elif eff[h, b] != 0 and c.Ks[h] > 1:
                assert np.abs(row).max() > 0.0, (h, b)
    assert got["sug_losses"][0] > 0.0


def test_poison_and_repeatability(hip):
    case = sp.SugCase(6, "alt", 8)
    run = SugLaunch(hip, case)
    kind = dev(case.kind)
    o = run.outputs()
    a = run.sug(o, kind, False, True)
    o2 = run.outputs()
    o2["scratch"] = o["scratch"]                                     # the scratch of the first launch, counter left at zero
    b = run.sug(o2, kind, False, True)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    p = run.sug(run.outputs(), kind, False, False, poison=flag.data_ptr())
    assert np.isnan(p["losses"]).all() and np.isnan(p["sug_losses"]).all()


# ----------------------------------------------------------------------------- end to end
def e2e_cfg(**kw):
    d = dict(use_adv_norm=True, ppo_epoch=1, max_grad_norm=250.0, lr=3e-4)
    d.update(kw)
    return d


def e2e_suggestions(agent, coeff=0.5, horizon=(3, 4)):
    from cadre_amd.suggest import Suggestions, peaked_prior, uniform_prior
    cfg = dict(coeff=coeff, events=dict(blocked=dict(head="throttle", prior=peaked_prior(3, 1, 0.8), horizon=horizon[1]),
                                        route_deviation=dict(head="steer", prior=uniform_prior(33), horizon=horizon[0])))
    return Suggestions(cfg, agent.arena.n_out, agent.device)


def event_rollouts(T, mbn, seed, sug, n_env=2):
    """Synthetic storages (tests/test_ppo_stats_gpu.storages) with a few recorded events on both heads."""
    from tests.test_ppo_stats_gpu import storages
    out = []
    for w in range(n_env):
        pair = storages(T, mbn, seed + w)
        for h, s in enumerate(pair):
            ev = s._event_tensors()
            for t in range(3 + w + 2 * h, T, 7):
                ev[t] = sug.code["route_deviation" if h == 0 else "blocked"]
        out.append(pair)
    return out


def test_section_gradient_equals_autograd_of_the_mixed_loss(tmp_path):
    """(a) One step of learner_section_multi over N = 2 environments (T = 32, one minibatch per epoch: B = 64, the row-sorted form)
    against float64 autograd through the oracle's nets of the PPO loss + the suggestion term on the rows the numpy scan marks, per
    parameter within 2e-4 of the model's max |g| (the bar of tests/test_learner_gpu.py for the PPO gradient)."""
    from cadre_amd import synth
    from oracle import ppo_ref
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section_multi
    from tests.test_imitation_gpu import make_agent
    T, N, C, SC = 32, 2, 4, 0.5
    agent = make_agent(tmp_path)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    sug = e2e_suggestions(agent)
    agent.learner.set_loss("ppo+suggest", suggest_coeff=SC)
    agent.learner.set_loss("ppo")
    rollouts = event_rollouts(T, 1, 900, sug, N)
    assert agent.learner.sorted_rows(N * T)
    torch.manual_seed(5)
    st = {}
    learner_section_multi(agent, rollouts, [False, False], e2e_cfg(max_grad_norm=1e9, lr=1e-9), shared, stats=st, suggest=sug)
    torch.cuda.synchronize()
    assert agent.learner.loss_mode == "ppo" and st["suggest"]["marked_rows"][0] > 0 and st["suggest"]["marked_rows"][1] > 0
    ring = agent._gather_idx
    idx = ring["slots"][(ring["pos"] - 1) % len(ring["slots"])][0].numpy()            # [2N][T]: the step's index vectors
    hz = host(sug.horizon)
    params = {m: {k: p.double().requires_grad_(True) for k, p in d.items()} for m, d in ppo_ref.to_torch_params(synth.ppo_state(11)).items()}
    B = N * T
    f = lambda t: host(t).reshape(t.shape[0], -1)
    cols = {k: np.zeros((2, B), np.float64) for k in ("act", "cmd", "ov", "ret", "olp", "adv", "kind")}
    xs, h0s, c0s = [], [], []
    for hd in range(2):
        xo, hh, cc_ = [], [], []
        for w in range(N):
            s = rollouts[w][hd]
            t = idx[2 * w + hd]
            marks = suggest_ref.mark_scan(host(s.events), f(s.masks)[:, 0], f(s.time_limits)[:, 0] if s._tl_used else None, hd, T, sug.Z, hz)
            assert np.array_equal(marks, host(s.suggest))
            sl = slice(w * T, (w + 1) * T)
            for k, src in (("act", s.action), ("cmd", s.command), ("ov", s.value_preds), ("ret", s.returns), ("olp", s.action_log_probs),
                           ("adv", s.advantages)):
                cols[k][hd, sl] = f(src)[t, 0]
            cols["kind"][hd, sl] = marks[t]
            xo.append(host(s._obs)[t][:, :, :530]); hh.append(host(s._hn)[t][:, :530]); cc_.append(host(s._cn)[t][:, :530])
        xs.append(np.concatenate(xo)); h0s.append(np.concatenate(hh)); c0s.append(np.concatenate(cc_))
    lg_rows, v_rows = [], []
    for hd, (head, K) in enumerate((("steer", 33), ("throttle", 3))):
        x = torch.from_numpy(xs[hd]).double().permute(1, 0, 2).reshape(-1, 530)        # time-major [S * B, 530]
        hid = (torch.from_numpy(h0s[hd]).double(), torch.from_numpy(c0s[hd]).double())
        for c in range(C):
            h, _ = ppo_ref.lstm_forward(x, hid, params["%s_lstm_%d" % (head, c)])
            lg_rows.append(torch.nn.functional.pad(ppo_ref.mlp3(h, params["%s_ppo_%d" % (head, c)], "control.linear"), (0, 64 - K)))
            v_rows.append(ppo_ref.mlp3(h, params["%s_ppo_%d" % (head, c)], "critic").view(-1))
    tt = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    lrn = agent.learner
    out = suggest_ref.suggest_loss(torch.stack(lg_rows), torch.stack(v_rows), tt(cols["act"], torch.int64), tt(cols["cmd"], torch.int64),
                                   tt(cols["ov"], torch.float64), tt(cols["ret"], torch.float64), tt(cols["olp"], torch.float64),
                                   tt(cols["adv"], torch.float64), cols["kind"].astype(np.int64), host(sug.prior), sug.Z, (33, 3), (None, None),
                                   C, lrn.clip, lrn.vc, lrn.cc, lrn.ec, 1.0 / T, SC)
    out["total"].backward()
    assert float(out["sug_loss"].detach()) > 0
    worst = 0.0
    for mn, d in params.items():
        gv = agent.arena.views(agent.arena.grads, mn)
        scale = max(float(p.grad.abs().max()) for p in d.values() if p.grad is not None)
        for k, p in d.items():
            g64 = torch.zeros_like(p) if p.grad is None else p.grad
            err = float((gv[k].cpu().double() - g64).abs().max()) / scale
            worst = max(worst, err)
            assert err < 2e-4, (mn, k, err)
    print("section gradient with suggestions: worst per-parameter error (rel. to model max |g|) %.2e; marked rows %s"
          % (worst, st["suggest"]["marked_rows"]))
    got_sug = float(agent.learner.workspace(B)["sug_losses"][0])
    want_sug = float(out["sug_loss"].detach())
    assert abs(got_sug - want_sug) < 1e-4 * max(1.0, abs(want_sug))


def test_suggestion_term_alone_lowers_the_kl(tmp_path):
    """(c) PPO coefficients 0 (advantages untouched), 5 epochs of 4 minibatches = 20 optimiser steps on the same rollouts: the KL
    towards the priors, summed over an epoch's four steps (every row once), is lower in the last epoch than in the first.  A direction
    check: no bar."""
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section_multi
    from tests.test_imitation_gpu import make_agent
    agent = make_agent(tmp_path)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    sug = e2e_suggestions(agent)
    lrn = agent.learner
    lrn.vc, lrn.cc, lrn.ec = 0.0, 0.0, 0.0
    lrn.set_loss("ppo+suggest", suggest_coeff=1.0)
    lrn.set_loss("ppo")
    rollouts = event_rollouts(16, 4, 700, sug)
    torch.manual_seed(9)
    st = {}
    learner_section_multi(agent, rollouts, [False, False], e2e_cfg(ppo_epoch=5, lr=1e-3), shared, stats=st, suggest=sug)
    torch.cuda.synchronize()
    kl = sug._rows[:20, :, 1].double().cpu().numpy().sum(-1)          # per step: sum over the heads of the minibatch mean kl
    first, last = kl[:4].sum(), kl[16:].sum()
    print("suggestion term alone: epoch kl %.6f -> %.6f over 20 steps" % (first, last))
    assert st["suggest"]["steps"] == 20 and first > 0 and last < first


class BlockedEnv(object):
    """tests.helpers.SyntheticEnv that reports "blocked" on every third step."""

    def __new__(cls, cfg):
        from tests.helpers import SyntheticEnv

        class _Env(SyntheticEnv):
            def step(self, action):
                obs, reward, done, info = SyntheticEnv.step(self, action)
                self.n_steps = getattr(self, "n_steps", 0) + 1
                if self.n_steps % 3 == 0:
                    info["suggest_event"] = "blocked"
                return obs, reward, done, info
        return _Env(cfg)


def run_train_vec(tmp, env_cls, episodes=3, logger=None, **extra):
    from ppo_agent.train import train_vec
    from tests.helpers import topology_cfgs
    train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp), T=8, episodes=episodes)
    train_cfg.update(save_interval=10 ** 6, **extra)
    os.makedirs(str(tmp), exist_ok=True)
    agent = train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, 1, env_cls=env_cls, logger=logger)
    torch.cuda.synchronize()
    return agent


def suggest_key():
    from cadre_amd.suggest import peaked_prior
    return dict(coeff=("linear", 0.5, 0.1), events=dict(blocked=dict(head="throttle", prior=peaked_prior(3, 1, 0.8), horizon=2)))


def test_train_vec_with_and_without_the_key(tmp_path):
    """(b) Three episodes on a synthetic env that reports "blocked" every third step."""
    from tests.helpers import SyntheticEnv
    lines = []
    logger = types.SimpleNamespace(log=lines.append)
    absent = run_train_vec(tmp_path / "a", SyntheticEnv)
    none = run_train_vec(tmp_path / "b", BlockedEnv, suggest=None)              # the env's extra info key alone changes nothing
    assert torch.equal(absent.arena.params, none.arena.params) and absent.arena.step == none.arena.step
    assert not any(k and "suggest" in str(k) for k in none.learner._graphs)
    agent = run_train_vec(tmp_path / "c", BlockedEnv, logger=logger, log_stats=True, suggest=suggest_key())
    assert agent.arena.step == absent.arena.step and agent.learner.loss_mode == "ppo"
    assert not torch.equal(agent.arena.params, absent.arena.params) and bool(torch.isfinite(agent.arena.params).all())
    stat_lines = [s for s in lines if "approx kl" in s]
    assert len(stat_lines) == 3
    for s in stat_lines:
        rows = s.split("suggest rows: ")[1].split(",")[0].split("/")
        assert float(rows[0]) == 0 and float(rows[1]) > 0, s
    assert agent.learner.hyper("suggest_coeff") == 0.5 + (0.1 - 0.5) * 2.0 / 3.0      # the schedule's value at the last episode


def test_refused_combinations(tmp_path):
    """(d)"""
    from tests.helpers import SyntheticEnv
    with pytest.raises(ValueError, match="demo_mix"):
        run_train_vec(tmp_path / "a", SyntheticEnv, suggest=suggest_key(), demo_mix=dict(episodes="nowhere"))
    with pytest.raises(ValueError, match="not part of a checkpoint"):
        run_train_vec(tmp_path / "b", SyntheticEnv, suggest=suggest_key(), checkpoint_interval=2)
    with pytest.raises(ValueError, match="suggest"):
        run_train_vec(tmp_path / "c", SyntheticEnv, suggest=dict(coeff=0.1, events=dict(e=dict(head="steer", prior=[1.0, 0.0], horizon=1))))
    with pytest.raises(ValueError, match="33"):                                    # a prior of the wrong length for its head
        run_train_vec(tmp_path / "d", SyntheticEnv, suggest=dict(coeff=0.1, events=dict(e=dict(head="steer", prior=[0.5, 0.5], horizon=1))))


def test_learner_refusals(tmp_path):
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section, learner_section_multi
    from tests.test_imitation_gpu import make_agent
    agent = make_agent(tmp_path)
    lrn = agent.learner
    with pytest.raises(ValueError, match="set_loss"):
        lrn.set_loss("ppo+suggest", suggest_coeff=float("nan"))
    with pytest.raises(ValueError, match="set_suggest_tables"):
        lrn.set_suggest_tables(torch.zeros(2, 10, 64, device="cuda"))
    with pytest.raises(ValueError, match="set_suggest_tables"):
        lrn.set_suggest_tables(torch.zeros(2, 3, 64))
    sug = e2e_suggestions(agent)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    rollouts = event_rollouts(16, 4, 300, sug)
    mixer = types.SimpleNamespace(label_smoothing=0.0, entries=lambda *a: [])
    with pytest.raises(ValueError, match="demo"):
        learner_section_multi(agent, rollouts, [False, False], e2e_cfg(), shared, demo=mixer, suggest=sug)
    with pytest.raises(ValueError, match="fused_gather"):
        learner_section(agent, rollouts[0][0], rollouts[0][1], False, e2e_cfg(), shared, fused_gather=False, suggest=sug)
    assert lrn.loss_mode == "ppo"
    # the single-environment section runs the same chain
    st = {}
    learner_section(agent, rollouts[0][0], rollouts[0][1], False, e2e_cfg(), shared, stats=st, suggest=sug)
    torch.cuda.synchronize()
    assert lrn.loss_mode == "ppo" and st["suggest"]["marked_rows"][0] > 0 and st["suggest"]["marked_rows"][1] > 0


def test_key_absent_keeps_the_launch_lists(tmp_path):
    """With no suggestions the update's launches are the parent's: the launch census of a section (the C-ABI calls the existing tests
    read) is the same before and after a section that ran WITH suggestions, and that section adds exactly the mark launch and one rows
    launch per step (the loss launch replaces the PPO loss launch one for one)."""
    from cadre_amd import hip
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section_multi
    from tests.test_imitation_gpu import make_agent
    agent = make_agent(tmp_path)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    sug = e2e_suggestions(agent)

    def section(**kw):
        rollouts = event_rollouts(16, 4, 300, sug)
        n0 = hip.N_CALLS
        learner_section_multi(agent, rollouts, [False, False], e2e_cfg(), shared, **kw)
        return hip.N_CALLS - n0, dict(agent.learner.launches)
    section()                                                         # eager run, then the warm-up that captures
    section()
    plain_calls, plain_launches = section()
    keys_before = set(agent.learner._graphs)
    section(suggest=sug)
    section(suggest=sug)
    sug_calls, sug_launches = section(suggest=sug)
    again_calls, again_launches = section()
    assert again_calls == plain_calls and again_launches == plain_launches
    assert keys_before <= set(agent.learner._graphs)
    assert all(any(isinstance(p, tuple) and p and p[0] == "suggest" for p in k) for k in set(agent.learner._graphs) - keys_before)
    assert sug_launches == plain_launches                             # per part of the step: the same number of launches
    assert sug_calls == plain_calls + 1 + 4                           # + the mark launch + one rows launch per minibatch step


def test_stale_reuse_rows_get_kind_zero(tmp_path):
    """sample_reuse beside suggestions: the entries of a ReuseWindow have no marks (source pointer 0), so their rows carry kind 0 and
    only the live rows are marked."""
    from cadre_amd.reuse import ReuseWindow
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section_multi
    from tests.test_imitation_gpu import make_agent
    T, MBN, N = 16, 4, 2
    agent = make_agent(tmp_path)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    sug = e2e_suggestions(agent)
    win = ReuseWindow(agent, 1, N, T)
    win.append(event_rollouts(T, MBN, 300, sug), [False, False])
    st = {}
    live = event_rollouts(T, MBN, 400, sug)
    losses = learner_section_multi(agent, live, [False, False], e2e_cfg(), shared, stats=st, suggest=sug, reuse=win)
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for col in losses for v in col) and st["reuse"]["filled"] == 1
    Bw = T // MBN
    B = 2 * N * Bw                                                    # live and stale entries
    w = agent.learner.workspace(B)
    kind = w["sug_kind"].cpu()
    pos = w["pos"].cpu().long() if agent.learner.sorted_rows(B) else None
    for hd in range(2):
        at = torch.arange(B) if pos is None else pos[hd]
        assert int(kind[hd][at[N * Bw:]].abs().sum()) == 0            # the stale rows of the last step
    want = sum(float((s.suggest != 0).sum()) for pair in live for s in pair)
    assert sum(st["suggest"]["marked_rows"]) == want > 0              # every live marked row was counted once (one epoch)
