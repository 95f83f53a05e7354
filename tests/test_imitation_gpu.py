"""GPU: the behaviour-cloning warm start — cadre_bc_loss against float64 autograd (tests/imitation_ref.py),
cadre_demo_rows, DemoSet end to end at 84 x 84, one imitation step per parameter, and pretrain."""
import functools
import os

import numpy as np
import pytest
import torch

from cadre_amd import synth
from tests import imitation_ref
from tests.test_ordinal_cpu import shipped_steer

pytestmark = pytest.mark.gpu
BC, VC, EC = 1.0, 0.1, 0.01
ADAM_EPS = 1e-8
F = imitation_ref.BC_STATS_FIELDS
# (B, C, K_steer, K_throttle): one row; an odd count; a second workgroup holding one row; the full-width row with a single
# command; thirteen workgroups per head
CASES = [(1, 4, 33, 3), (7, 3, 33, 3), (17, 4, 33, 3), (64, 1, 64, 2), (200, 4, 33, 3)]


def rel(a, b):
    a = np.asarray(torch.as_tensor(a).detach().cpu(), np.float64)
    b = np.asarray(torch.as_tensor(b).detach().cpu(), np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def steer_rank(K, g):
    """The non-monotone shipped steer table's ranks for 33 bins; a random permutation for any other width."""
    if K == 33:
        from ppo_agent.agent import ordinal_rank
        return ordinal_rank(shipped_steer())
    return torch.randperm(K, generator=g).tolist()


def ord_table(ranks):
    t = torch.zeros(2, 64, dtype=torch.int32)
    for h, r in enumerate(ranks):
        if r is None:
            t[h, 0] = -1
        else:
            t[h, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return t.cuda()


@functools.lru_cache(maxsize=None)
def bc_case(B, C, nS, nT, scale, weighted, special=None):
    """Inputs (ldl = 64) shared by every variant of a case.  special: "idle" — the last command owns no row;
    "unlabelled" — action -1 in a third of the rows of each head (other thirds), one out-of-range command."""
    g = torch.Generator().manual_seed(1000 * B + nS + (7 if weighted else 0) + int(scale))
    logits = torch.zeros(2 * C, B, 64)
    logits[:C, :, :nS] = torch.randn(C, B, nS, generator=g) * scale
    logits[C:, :, :nT] = torch.randn(C, B, nT, generator=g) * scale
    values = torch.randn(2 * C, B, generator=g)
    actions = torch.stack([torch.randint(0, nS, (B,), generator=g), torch.randint(0, nT, (B,), generator=g)])
    cmds = torch.randint(0, C - 1 if special == "idle" else C, (2, B), generator=g, dtype=torch.int32)
    if special == "unlabelled":
        actions[0, 0::3] = -1
        actions[1, 1::3] = -1
        actions[1, 2] = nT                                  # one past the head's bins: skipped like -1
        cmds[0, 1], cmds[1, 3] = C, -1
    rets = torch.randn(2, B, generator=g)
    w = (torch.rand(2, B, generator=g) * 3.75 + 0.25) if weighted else None
    ranks = (steer_rank(nS, g), torch.randperm(nT, generator=g).tolist())
    return dict(logits=logits, values=values, actions=actions, cmds=cmds, rets=rets, w=w), ranks


@functools.lru_cache(maxsize=None)
def bc_ref(B, C, nS, nT, scale, weighted, eps, ordmode, special=None):
    """(losses[3], d total / d raw, d total / d value, stats [2][6]) in float64, once per variant."""
    inp, ranks = bc_case(B, C, nS, nT, scale, weighted, special)
    rk = {"cat": (None, None), "both": ranks, "steer": (ranks[0], None)}[ordmode]
    lg = inp["logits"].double().requires_grad_(True)
    vv = inp["values"].double().requires_grad_(True)
    tv, tb, te, total, stats = imitation_ref.bc_loss(lg, vv, inp["actions"], inp["cmds"], inp["rets"], inp["w"], (nS, nT), rk, C,
                                                     eps, BC, VC, EC, 1.0 / B)
    total.backward()
    return torch.tensor([float(tv.detach()), float(tb.detach()), float(te.detach())]), lg.grad, vv.grad, stats


def new_outputs(B, C):
    out = dict(losses=torch.zeros(3, device="cuda"), dl=torch.full((2 * C, B, 64), 9.0, device="cuda"),
               dv=torch.full((2 * C, B), 9.0, device="cuda"), scratch=torch.full((4 + 6 * ((B + 15) // 16),), 3.0, device="cuda"),
               stats=torch.full((2, F), 5.0, device="cuda"), sscr=torch.full((12 * ((B + 15) // 16),), 3.0, device="cuda"))
    out["scratch"][0] = 0.0                                # the arrival counter: zero on first use, reset by every launch
    return out


def run_bc(d, o, B, C, nS, nT, eps, table=None, grad=True, stats=True, poison=None, coeffs=(BC, VC, EC)):
    from cadre_amd import hip
    w = d.get("w")
    hip.check(hip.lib().cadre_bc_loss(
        d["logits"].data_ptr(), 64, B * 64, d["values"].data_ptr(), 1, B, d["actions"].data_ptr(), d["cmds"].data_ptr(),
        d["rets"].data_ptr(), None if w is None else w.data_ptr(), B, C, nS, nT, eps, coeffs[0], coeffs[1], coeffs[2], 1.0 / B,
        o["losses"].data_ptr(), o["dl"].data_ptr() if grad else None, o["dv"].data_ptr() if grad else None,
        o["scratch"].data_ptr(), None if poison is None else poison.data_ptr(), o["stats"].data_ptr() if stats else None, F,
        o["sscr"].data_ptr() if stats else None, None if table is None else table.data_ptr(), hip.stream()), "cadre_bc_loss")
    assert float(o["scratch"][0]) == 0.0                   # the counter is left zero


def dev_inputs(inp):
    return {k: v.cuda() for k, v in inp.items() if v is not None}


def check_against_ref(case, scale, weighted, eps, ordmode, special=None):
    B, C, nS, nT = case
    inp, ranks = bc_case(B, C, nS, nT, scale, weighted, special)
    want_l, want_dl, want_dv, want_st = bc_ref(B, C, nS, nT, scale, weighted, eps, ordmode, special)
    table = {"cat": None, "both": ord_table(ranks), "steer": ord_table((ranks[0], None))}[ordmode]
    d, o = dev_inputs(inp), new_outputs(B, C)
    run_bc(d, o, B, C, nS, nT, eps, table)
    e_l, e_dv, e_dl = rel(o["losses"], want_l), rel(o["dv"], want_dv), rel(o["dl"], want_dl)
    e_st = float((o["stats"].double().cpu() - want_st).abs().max())
    print("case %s scale %g weighted %s eps %g %s %s: losses %.2e dvalues %.2e dlogits %.2e stats %.2e"
          % (case, scale, weighted, eps, ordmode, special, e_l, e_dv, e_dl, e_st))
    assert e_l < 1e-5 and e_dv < 1e-5 and e_dl < 2e-5, (e_l, e_dv, e_dl)
    assert e_st < 1e-5 and torch.equal((o["stats"][:, 0].double().cpu() * B).round(), (want_st[:, 0] * B).round())   # accuracy: exact counts
    assert float(o["dl"][:C, :, nS:].abs().max() if nS < 64 else 0.0) == 0.0 and float(o["dl"][C:, :, nT:].abs().max()) == 0.0
    # exact zeros everywhere but a counted row's own net: the other nets of a head, skipped rows, an idle command
    zero_l, zero_v = torch.ones(2 * C, B, 64, dtype=torch.bool), torch.ones(2 * C, B, dtype=torch.bool)
    for hd, K in enumerate((nS, nT)):
        a_, c_ = inp["actions"][hd], inp["cmds"][hd].long()
        rows = torch.nonzero((c_ >= 0) & (c_ < C) & (a_ >= 0) & (a_ < K)).view(-1)
        zero_l[hd * C + c_[rows], rows, :K] = False
        zero_v[hd * C + c_[rows], rows] = False
    assert float(o["dl"].cpu()[zero_l].abs().max()) == 0.0 and float(want_dl[zero_l].abs().max()) == 0.0
    assert float(o["dv"].cpu()[zero_v].abs().max() if zero_v.any() else 0.0) == 0.0
    return inp, d, o, table


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("case", CASES)
def test_bc_loss_fwd_bwd(case, eps, weighted, scale):
    """Losses 1e-5, dvalues 1e-5, dlogits 2e-5 (relative to the largest reference magnitude: the bars of the categorical loss
    kernel) and the statistics 1e-5 absolute against float64 autograd; zero columns >= K; three repeated launches
    bit-identical; poison; the evaluation form."""
    B, C, nS, nT = case
    inp, d, o, table = check_against_ref(case, scale, weighted, eps, "cat")
    first = {k: o[k].clone() for k in ("losses", "dl", "dv", "stats")}
    for _ in range(3):                                     # partials combined in workgroup order
        run_bc(d, o, B, C, nS, nT, eps, table)
        assert all(torch.equal(o[k], first[k]) for k in first)
    o2 = new_outputs(B, C)                                 # the -1 marker and no stats row: the same bits
    run_bc(d, o2, B, C, nS, nT, eps, ord_table((None, None)), stats=False)
    assert all(torch.equal(o2[k], first[k]) for k in ("losses", "dl", "dv")) and float((o2["stats"] - 5.0).abs().max()) == 0.0
    ev = new_outputs(B, C)                                 # evaluation form: sentinel-filled gradient buffers stay
    run_bc(d, ev, B, C, nS, nT, eps, table, grad=False)
    assert torch.equal(ev["losses"], first["losses"]) and torch.equal(ev["stats"], first["stats"])
    assert float((ev["dl"] - 9.0).abs().max()) == 0.0 and float((ev["dv"] - 9.0).abs().max()) == 0.0
    poison = torch.ones(1, dtype=torch.int32, device="cuda")   # a reported forward-pass timeout: NaN losses
    run_bc(d, o, B, C, nS, nT, eps, table, poison=poison)
    assert bool(torch.isnan(o["losses"]).all()) and torch.equal(o["dl"], first["dl"]) and torch.equal(o["dv"], first["dv"])


@pytest.mark.parametrize("ordmode", ["both", "steer"])
@pytest.mark.parametrize("case", CASES)
def test_bc_loss_ordinal_heads(case, ordmode):
    """Both heads ordinal (the non-monotone shipped steer table at 33 bins) and steer-only ordinal, smoothed and weighted,
    saturating logits; the categorical throttle head of the mix is the categorical launch's, bit for bit."""
    B, C, nS, nT = case
    inp, d, o, table = check_against_ref(case, 4.0, True, 0.1, ordmode)
    first = {k: o[k].clone() for k in ("losses", "dl", "dv", "stats")}
    for _ in range(3):
        run_bc(d, o, B, C, nS, nT, 0.1, table)
        assert all(torch.equal(o[k], first[k]) for k in first)
    if ordmode == "steer":
        cat = new_outputs(B, C)
        run_bc(d, cat, B, C, nS, nT, 0.1, None)
        assert torch.equal(cat["dl"][C:], first["dl"][C:]) and torch.equal(cat["dv"], first["dv"])
        assert torch.equal(cat["stats"][1], first["stats"][1])


def test_bc_loss_idle_command_gets_exact_zeros():
    case = (7, 3, 33, 3)
    B, C, nS, nT = case
    inp, d, o, _t = check_against_ref(case, 1.0, True, 0.1, "cat", special="idle")
    assert int(inp["cmds"].max()) == C - 2
    for hd in range(2):
        assert float(o["dl"][hd * C + C - 1].abs().max()) == 0.0 and float(o["dv"][hd * C + C - 1].abs().max()) == 0.0


@pytest.mark.parametrize("ordmode", ["cat", "both"])
def test_bc_loss_unlabelled_rows_and_bad_commands_count_out(ordmode):
    case = (17, 4, 33, 3)
    B, C, nS, nT = case
    inp, d, o, _t = check_against_ref(case, 1.0, True, 0.1, ordmode, special="unlabelled")
    skipped = [(inp["actions"][0] < 0) | (inp["cmds"][0] >= C), (inp["actions"][1] < 0) | (inp["actions"][1] >= nT) | (inp["cmds"][1] < 0)]
    for hd in range(2):
        assert int(skipped[hd].sum()) >= B // 3
        assert abs(float(o["stats"][hd, 5]) - float((~skipped[hd]).sum()) / B) < 1e-6          # field 5 counts them out
        rows = torch.nonzero(skipped[hd]).view(-1).cuda()
        assert float(o["dl"][hd * C:(hd + 1) * C][:, rows].abs().max()) == 0.0
        assert float(o["dv"][hd * C:(hd + 1) * C][:, rows].abs().max()) == 0.0


@pytest.mark.parametrize("case", [(17, 4, 33, 3), (64, 1, 64, 2)])
def test_bc_gradient_equals_the_ppo_kernel_on_policy(case):
    """Both are -w inv_b grad log p(a): cadre_ppo_loss with old_logp = the row's own log-prob (cadre_categorical_eval),
    adv = w > 0 and the value and entropy coefficients 0 against cadre_bc_loss at eps = 0, within the 2e-5 bar."""
    from cadre_amd import hip
    B, C, nS, nT = case
    inp, _r = bc_case(B, C, nS, nT, 1.0, True)
    d = dev_inputs(inp)
    L = hip.lib()
    old_lp = torch.zeros(2, B, device="cuda")
    ent = torch.zeros(B, device="cuda")
    for hd, K in enumerate((nS, nT)):
        own = d["logits"][hd * C + d["cmds"][hd].long(), torch.arange(B, device="cuda")].contiguous()
        hip.check(L.cadre_categorical_eval(own.data_ptr(), 64, d["actions"][hd].contiguous().data_ptr(), B, K,
                                           old_lp[hd].data_ptr(), ent.data_ptr(), hip.stream()), "cadre_categorical_eval")
    ppo, bc = new_outputs(B, C), new_outputs(B, C)
    zeros = torch.zeros(2, B, device="cuda")
    hip.check(L.cadre_ppo_loss(d["logits"].data_ptr(), 64, B * 64, d["values"].data_ptr(), 1, B, d["actions"].data_ptr(),
                               d["cmds"].data_ptr(), zeros.data_ptr(), d["rets"].data_ptr(), old_lp.data_ptr(), d["w"].data_ptr(),
                               B, C, nS, nT, 0.1, 0.0, 1.0, 0.0, 1.0 / B, ppo["losses"].data_ptr(), ppo["dl"].data_ptr(),
                               ppo["dv"].data_ptr(), ppo["scratch"].data_ptr(), None, hip.stream()), "cadre_ppo_loss")
    run_bc(d, bc, B, C, nS, nT, 0.0, None, coeffs=(1.0, 0.0, 0.0))
    e = rel(bc["dl"], ppo["dl"])
    print("case %s: bc vs ppo dlogits %.2e" % (case, e))
    assert e < 2e-5 and float(ppo["dl"].abs().max()) > 0 and float(bc["dv"].abs().max()) == 0.0


# ----------------------------------------------------------------------------- cadre_demo_rows
def test_demo_rows():
    from cadre_amd import hip
    from ppo_agent.storage import RolloutStorage
    T, S, n = 5, 8, 12
    r = np.random.RandomState(3)
    stor = RolloutStorage(T, 1, 530, S, 530, True, 0.99, 0.95)
    stor.to("cuda:0")
    ldo = stor._ldo
    latent = r.standard_normal((n, 512)).astype(np.float32)
    meas = r.rand(n, 3)
    window = r.randint(0, n, (T, S)).astype(np.int32)
    want = imitation_ref.window_rows(latent, window, meas, ldo)
    stor._obs.fill_(-7.0)
    lat_d, win_d, meas_d = torch.from_numpy(latent).cuda(), torch.from_numpy(window).cuda(), torch.from_numpy(meas).cuda()

    def run(win):
        hip.check(hip.lib().cadre_demo_rows(lat_d.data_ptr(), 512, n, win.data_ptr(), meas_d.data_ptr(), T, S, stor._obs.data_ptr(),
                                            ldo, hip.stream()), "cadre_demo_rows")
    run(win_d)
    got = stor._obs.cpu().numpy()
    assert np.array_equal(got[:T], want)                                  # bit-identical, pad columns zero
    assert ldo > 530 and float(np.abs(got[:T, :, 530:]).max()) == 0.0
    assert float(np.abs(got[T] + 7.0).max()) == 0.0                       # the sentinel-filled row T is untouched
    bad = window.copy()
    bad[2, 3], bad[4, 7] = n, -1
    run(torch.from_numpy(bad).cuda())
    got2 = stor._obs.cpu().numpy()
    for t, s in ((2, 3), (4, 7)):
        assert np.isnan(got2[t, s, :530]).all() and float(np.abs(got2[t, s, 530:]).max()) == 0.0
    keep = np.ones((T, S), bool)
    keep[2, 3] = keep[4, 7] = False
    assert np.array_equal(got2[:T][keep], want[keep]) and float(np.abs(got2[T] + 7.0).max()) == 0.0   # neighbours untouched
    # a latent table with a pitch of its own (a view of wider rows)
    wide = torch.zeros(n, 544, device="cuda")
    wide[:, :512] = lat_d
    hip.check(hip.lib().cadre_demo_rows(wide.data_ptr(), 544, n, win_d.data_ptr(), meas_d.data_ptr(), T, S, stor._obs.data_ptr(),
                                        ldo, hip.stream()), "cadre_demo_rows")
    assert np.array_equal(stor._obs.cpu().numpy()[:T], want)


# ----------------------------------------------------------------------------- DemoSet end to end
def make_agent(tmp, ppo_seed=11):
    from ppo_agent.agent import CadreAgent
    from tests.helpers import topology_cfgs
    _tc, agent_cfg, _ec, _rc = topology_cfgs(str(tmp))
    agent = CadreAgent(**agent_cfg)
    agent.arena.load_numpy_state(synth.ppo_state(ppo_seed))
    return agent


def record_episodes(directory, lengths=(12, 9), seed=40):
    """Synthetic episodes written with RolloutRecorder; a `done` inside the first, the second truncated; some -1 labels."""
    from cadre_amd import replay
    rec = replay.RolloutRecorder(str(directory))
    paths = []
    for e, n in enumerate(lengths):
        steps = synth.synth_rollout(n, 84, 84, seed=seed + e)
        for i, td in enumerate(steps):
            done = [e == 0 and i == 4, False]
            act = (-1 if i % 5 == 3 else (7 * i + e) % 33, (i + e) % 3)
            rec.step(dict(rgb=td["rgb"], route_fig=td["route_fig"], measurements=td["measurements"], command=td["command"]),
                     act, (-0.5, -0.1), (0.0, 0.0), td["reward"], done)
        paths.append(rec.end_episode())
    return paths


def test_demo_set_end_to_end(tmp_path):
    from cadre_amd import replay
    from ppo_agent.imitation import DemoSet
    agent = make_agent(tmp_path)
    paths = record_episodes(tmp_path / "demos")
    eps = [replay.load_episode(p) for p in paths]
    demo = DemoSet.from_episodes(agent, paths, gamma=0.99, balance="command")
    assert demo.T == 21 and demo.episodes == [(0, 12), (12, 21)] and demo.throttle._obs is demo.steer._obs
    t = 0
    for ep in eps:
        for i in range(ep["window"].shape[0]):
            feat = agent.get_latent_feature(replay.windows(ep, i))            # the encoder is batch-invariant: equal bits
            assert torch.equal(demo.steer.obs[t], feat), (t,)
            assert float(demo.steer._obs[t, :, 530:].abs().max()) == 0.0
            t += 1
    cmd = np.concatenate([ep["command"] for ep in eps])
    act = np.concatenate([ep["action"] for ep in eps])
    rew = np.concatenate([ep["reward"] for ep in eps])
    done = np.concatenate([ep["done"] for ep in eps])
    assert int((act[:, 0] == -1).sum()) == 4
    for hd, st in enumerate((demo.steer, demo.throttle)):
        assert np.array_equal(st.command[:21, 0].cpu().numpy(), cmd) and np.array_equal(st.action[:21, 0].cpu().numpy(), act[:, hd])
        m = 1.0 - done[:, hd].astype(np.float32)
        m[11] = m[20] = 0.0                                                   # a record that ends without done is ended
        assert np.array_equal(st.masks[:21, 0].cpu().numpy(), m)
        want = imitation_ref.mc_returns(rew[:, hd], m, 0.99)
        assert np.array_equal(st.returns[:21, 0].cpu().numpy(), want)         # the strict fp32 scan, bit for bit
        assert float(st.value_preds.abs().max()) == 0.0 and float(st._hn.abs().max()) == 0.0
    assert np.abs(demo.weights[:, 0].cpu().numpy() - imitation_ref.balance_weights(cmd)).max() < 1e-6
    scaled = DemoSet.from_episodes(agent, eps, gamma=0.99, balance=None, return_scale=0.25)
    assert torch.equal(scaled.steer.returns, demo.steer.returns * 0.25) and float((scaled.weights - 1).abs().max()) == 0.0


def test_monte_carlo_returns_in_chunks_equal_one_scan():
    """Sets above 3000 rows are scanned in chunks from the back, each bootstrapping from the first return of the chunk behind
    it: 6001 rows (chunks of 3000, 2999 and 2 rows) of random rewards and 0 / 1 masks, no encoder, bit for bit against the
    numpy loop over the whole set; then with return_scale."""
    from ppo_agent import imitation
    from ppo_agent.imitation import DemoSet
    T = 6001
    chunks = imitation._gae_chunks(T)
    assert [hi - lo for lo, hi in chunks] == [2, 2999, 3000]
    r = np.random.RandomState(8)
    rew = r.rand(T, 2).astype(np.float32) - 0.3
    m = (r.rand(T, 2) >= 0.01).astype(np.float32)
    m[2999] = 1.0                                                             # a return that crosses both chunk borders
    m[5998] = 1.0
    m[T - 1] = 0.0
    steer, throttle = DemoSet._storages(T, 530, 1, 530, 0.99, "cuda:0")
    for hd, st in enumerate((steer, throttle)):
        st.rewards[:T, 0].copy_(torch.from_numpy(rew[:, hd].copy()))
        st.masks[:T, 0].copy_(torch.from_numpy(m[:, hd].copy()))
    DemoSet._mc_returns(steer, throttle, chunks, 0.99, 1.0)
    for hd, st in enumerate((steer, throttle)):
        want = imitation_ref.mc_returns(rew[:, hd], m[:, hd], 0.99)
        got = st.returns[:, 0].cpu().numpy()
        assert np.array_equal(got[:T], want) and got[T] == 0.0
        assert want[3000] != 0 and want[2999] != rew[2999, hd]                # (the border row does carry the chunk behind it)
        assert float(st.value_preds.abs().max()) == 0.0 and float(st.advantages.abs().max()) == 0.0
    DemoSet._mc_returns(steer, throttle, chunks, 0.99, 0.5)
    assert np.array_equal(steer.returns[:T, 0].cpu().numpy(), imitation_ref.mc_returns(rew[:, 0], m[:, 0], 0.99) * np.float32(0.5))


# ----------------------------------------------------------------------------- one imitation step, per parameter
def random_host(T, seed):
    """Random feature rows, labels, commands, returns and weights of a T-row demonstration set (host arrays)."""
    r = np.random.RandomState(seed)
    obs = (r.standard_normal((T, 8, 530)) * 0.5).astype(np.float32)
    cmd = r.randint(0, 4, T).astype(np.int32)
    act = np.stack([r.randint(0, 33, T), r.randint(0, 3, T)], 1).astype(np.int64)
    act[1, 0] = -1                                                            # one unlabelled steer row
    ret = r.standard_normal((T, 2)).astype(np.float32)
    w = (r.rand(T) * 3.75 + 0.25).astype(np.float32)
    return dict(obs=obs, cmd=cmd, act=act, ret=ret, w=w)


def random_demo(agent, T, seed):
    """A DemoSet of random feature rows (no encoder): what the float64 reference can be fed on the CPU."""
    from ppo_agent.imitation import DemoSet
    host = random_host(T, seed)
    obs, cmd, act, ret, w = (host[k] for k in ("obs", "cmd", "act", "ret", "w"))
    steer, throttle = DemoSet._storages(T, 530, 8, 530, 0.99, "cuda:0")
    steer.obs[:T].copy_(torch.from_numpy(obs))
    for hd, st in enumerate((steer, throttle)):
        st.command[:T, 0].copy_(torch.from_numpy(cmd))
        st.action[:T, 0].copy_(torch.from_numpy(act[:, hd].copy()))
        st.returns[:T, 0].copy_(torch.from_numpy(ret[:, hd].copy()))
    demo = DemoSet(steer, throttle, torch.from_numpy(w).cuda().view(T, 1), [(0, T)], cmd, 0.99, None, 1.0)
    return demo, host


def reference_step(host, idx, eps, params=None, C=4):
    """float64 autograd through the oracle's nets (oracle/ppo_ref.py) with the reference loss on rows idx.  Returns
    (params, losses[3], stats)."""
    from oracle import ppo_ref
    if params is None:
        params = {m: {k: p.double().requires_grad_(True) for k, p in d.items()}
                  for m, d in ppo_ref.to_torch_params(synth.ppo_state(11)).items()}
    B = len(idx)
    x = torch.from_numpy(host["obs"][idx]).double().permute(1, 0, 2).reshape(-1, 530)          # time-major [S * B, 530]
    zero = (torch.zeros(B, 530, dtype=torch.float64), torch.zeros(B, 530, dtype=torch.float64))
    lg_rows, v_rows = [], []
    for hd, (head, K) in enumerate((("steer", 33), ("throttle", 3))):
        for c in range(C):
            h, _ = ppo_ref.lstm_forward(x, zero, params["%s_lstm_%d" % (head, c)])
            raw = ppo_ref.mlp3(h, params["%s_ppo_%d" % (head, c)], "control.linear")
            lg_rows.append(torch.nn.functional.pad(raw, (0, 64 - K)))
            v_rows.append(ppo_ref.mlp3(h, params["%s_ppo_%d" % (head, c)], "critic").view(-1))
    logits, values = torch.stack(lg_rows), torch.stack(v_rows)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    tv, tb, te, total, stats = imitation_ref.bc_loss(logits, values, t(host["act"][idx].T), t(host["cmd"][idx]).view(1, -1).repeat(2, 1),
                                                     t(host["ret"][idx].T), t(host["w"][idx]).view(1, -1).repeat(2, 1), (33, 3),
                                                     (None, None), C, eps, BC, VC, EC, 1.0 / B)
    for d in params.values():
        for p in d.values():
            p.grad = None
    total.backward()
    for d in params.values():
        for p in d.values():
            if p.grad is None:
                p.grad = torch.zeros_like(p)
    return params, [float(tv.detach()), float(tb.detach()), float(te.detach())], stats


def ppo_samples(B, C=4, seed=9):
    r = np.random.RandomState(seed)
    out = []
    for K in (33, 3):
        tup = (torch.from_numpy((r.standard_normal((8 * B, 530)) * 0.5).astype(np.float32)),
               torch.from_numpy(r.randint(0, K, (B, 1)).astype(np.int64)),
               torch.from_numpy((0.3 * r.standard_normal((B, 1))).astype(np.float32)),
               torch.from_numpy(r.standard_normal((B, 1)).astype(np.float32)), torch.ones(B, 1),
               torch.from_numpy((-np.log(K) + 0.2 * r.standard_normal((B, 1))).astype(np.float32)),
               torch.from_numpy(r.standard_normal((B, 1)).astype(np.float32)),
               [torch.zeros(B, 530), torch.zeros(B, 530)], torch.from_numpy(r.randint(0, C, (B, 1)).astype(np.int32)))
        out.append(tuple(x.cuda() if not isinstance(x, list) else [y.cuda() for y in x] for x in tup))
    return out


@pytest.mark.parametrize("B,sort", [(24, False), (64, True), (64, False)])
def test_one_imitation_step_matches_float64_autograd_per_param(tmp_path, B, sort):
    """Gradients of one imitation step within 2e-4 of each model's max |g| (the project's gradient bar) of float64 autograd
    through the oracle's nets with the reference loss: eager (call 1), warm-up (call 2) and through the captured graph (call
    3), bit-identical to each other.  B = 24 is the masked (unsorted) form; the row-sorted form exists from B = 64 in
    multiples of 32, so B = 64 runs both forms.  A PPO step right after is bit-identical to the same step on an agent that
    never entered BC mode, through its own captured graph.
    Parameters after one clip + Adam step against the whole float64 chain (float64 autograd, then the oracle's step in
    float64), element by element within 1e-5 of the model's largest |parameter| wherever the step is well conditioned, and
    bounded element by element where it is not.  Adam's first step is lr g / (|g| + eps), eps = 1e-8: its derivative is
    lr eps / (|g| + eps)^2, at most lr / (121 eps) for |g| >= 10 eps and up to lr / eps = 3e4 below, where the fp32 rounding
    of a gradient (1e-10 .. 1e-9 here) moves its parameter by up to 3e-5 in any fp32 implementation (torch's own fp32 autograd
    of the same loss on the CPU: 1.5e-5 of max |p|).  So: every element with float64 |g| >= 10 eps = 1e-7 is held to 1e-5;
    the others must be few (below 1 % of the elements that have a gradient; 0.2 % for torch's fp32 autograd), must be exactly
    the ones below the threshold by construction, and each of them (with the elements that have no gradient at all) is held to
    the Lipschitz bound lr / eps |g_device - g_64|.  Beside it the two checks that do not depend on conditioning: every
    element against the oracle's step on the device's own gradients, and the per-model parameter sums (the measure of the
    learner section's replay test), both at 1e-5."""
    from oracle import ppo_ref
    agent, fresh = make_agent(tmp_path), make_agent(tmp_path)
    agent.learner.use_sorted = sort
    fresh.learner.use_sorted = sort
    assert agent.learner.sorted_rows(B) == sort
    eps = 0.1
    demo, host = random_demo(agent, B + 8, seed=B)
    idx = torch.from_numpy(np.random.RandomState(1).permutation(B + 8)[:B].astype(np.int64))
    params, want_l, want_st = reference_step(host, idx.numpy(), eps)
    row = torch.zeros(2, F, device="cuda")
    calls = []
    for _ in range(3):
        got = agent.imitate_from_storages(demo.batch(idx), stats_row=row, label_smoothing=eps)
        calls.append((got, agent.arena.grads.clone(), row.clone()))
    assert agent.learner.loss_mode == "ppo"                                   # the mode is restored on exit
    assert any(k[0] == "all" and ("bc", eps, 1.0) in k for k in agent.learner._graphs if k[0] != "warm")
    for got, grads, st in calls[1:]:
        assert got == calls[0][0] and torch.equal(grads, calls[0][1]) and torch.equal(st, calls[0][2])
    assert rel(calls[0][0], want_l) < 1e-4
    assert float((calls[0][2].double().cpu() - want_st).abs().max()) < 1e-4
    worst = 0.0
    for mn, d in params.items():
        gv = agent.arena.views(calls[2][1], mn)
        scale = max(float(p.grad.abs().max()) for p in d.values())
        assert scale > 0
        for k, p in d.items():
            err = float((gv[k].cpu().double() - p.grad).abs().max()) / scale
            worst = max(worst, err)
            assert err < 2e-4, (mn, k, err)
    print("B %d sorted %s: worst per-parameter gradient error (rel. to model max |g|): %.2e" % (B, sort, worst))
    # a PPO step right after: the graphs of the two modes do not mix
    smp = ppo_samples(B)
    for _ in range(3):
        l_a, l_f = agent.update_policy(smp[0], smp[1]), fresh.update_policy(smp[0], smp[1])
        assert l_a == l_f and torch.equal(agent.arena.grads, fresh.arena.grads)
    # and the imitation step again (a replay of its own graph), then the optimiser step
    again = agent.imitate_from_storages(demo.batch(idx), stats_row=row, label_smoothing=eps)
    assert again == calls[0][0] and torch.equal(agent.arena.grads, calls[0][1])
    agent.learner.clip_adam(lr=3e-4, max_grad_norm=250.0)
    lr = 3e-4

    def oracle_step(grads):
        ps = {m: {k: p.detach().clone() for k, p in d.items()} for m, d in params.items()}
        adam = {m: {k: (torch.zeros_like(p), torch.zeros_like(p)) for k, p in d.items()} for m, d in ps.items()}
        ppo_ref.chief_step(ps, grads, adam, 1, lr=lr, max_grad_norm=250.0)
        return ps
    names = list(params)
    dev_p = {m: {k: v.cpu().double() for k, v in agent.arena.views(agent.arena.params, m).items()} for m in names}
    dev_g = {m: {k: v.cpu().double() for k, v in agent.arena.views(calls[0][1], m).items()} for m in names}
    same_g, chain = oracle_step(dev_g), oracle_step({m: {k: p.grad for k, p in d.items()} for m, d in params.items()})
    thr = 10 * ADAM_EPS
    worst_s = worst_k = worst_x = 0.0
    n_all = n_out = 0
    for mn in names:
        scale = max(float(p.abs().max()) for p in chain[mn].values())
        for k, p in params[mn].items():
            g64 = p.grad
            diff = (dev_p[mn][k] - chain[mn][k]).abs()
            worst_s = max(worst_s, float((dev_p[mn][k] - same_g[mn][k]).abs().max()) / scale)
            keep = g64.abs() >= thr
            out = ~keep                                   # (with the elements that have no float64 gradient at all)
            n_all += int((g64 != 0).sum())
            n_out += int((out & (g64 != 0)).sum())
            if keep.any():
                worst_k = max(worst_k, float(diff[keep].max()) / scale)
            if out.any():
                # the step lr g / (|g| + eps) is Lipschitz with constant lr / eps: the two steps differ by no more than that
                # times the difference of the gradients (+ the fp32 rounding of the parameter itself, 2^-24 |p|)
                room = lr / ADAM_EPS * (dev_g[mn][k] - g64).abs()[out] * (1 + 1e-3) + 2.0 ** -23 * scale
                worst_x = max(worst_x, float((diff[out] / room).max()))
    e_sum = rel([float(sum(t.sum() for t in dev_p[m].values())) for m in names],
                [float(sum(t.sum() for t in chain[m].values())) for m in names])
    print("B %d sorted %s: parameters after clip + Adam against the float64 chain: %.2e of max |p| on the elements with |g| >= %.0e, "
          "%d of %d elements with a gradient below that (%.3f %%), those at %.2f of their Lipschitz room; per-model sums %.2e; "
          "against the oracle's step on the device's gradients %.2e"
          % (B, sort, worst_k, thr, n_out, n_all, 100.0 * n_out / n_all, worst_x, e_sum, worst_s))
    assert worst_k < 1e-5 and worst_s < 1e-5 and e_sum < 1e-5
    assert n_out < 0.01 * n_all and worst_x <= 1.0


def test_bc_mode_refuses_the_device_hyper_block(tmp_path):
    from cadre_amd import hip
    agent = make_agent(tmp_path)
    agent.learner.set_device_hyper(True)
    with pytest.raises(hip.CadreHipError, match="device-hyper"):
        agent.learner.set_loss("bc")
    agent.learner.set_device_hyper(False)
    agent.learner.set_loss("bc", label_smoothing=0.1)
    assert ("bc", 0.1, 1.0) in agent.learner._mode_key()
    agent.learner.set_loss("ppo")
    assert agent.learner._mode_key() == ()
    with pytest.raises(ValueError):
        agent.learner.set_loss("bc", label_smoothing=1.0)


# ----------------------------------------------------------------------------- pretrain
def test_pretrain_overfits_one_minibatch(tmp_path):
    """16 rows, 30 steps, lr 1e-3: the NLL (field 1) of both heads after the last step is below its value at step 0 — the
    sign of the change only.  The float64 reference (reference_step + the oracle's chief_step, the same rows, seed 16) was
    run for the same 30 steps on the CPU and itself decreases: steer 3.2866 -> 2.9e-5, throttle 1.1284 -> 2.2e-7."""
    from ppo_agent.imitation import evaluate, pretrain
    agent = make_agent(tmp_path)
    demo, _host = random_demo(agent, 16, seed=16)
    before = evaluate(agent, demo, 16)
    assert agent.learner.loss_mode == "ppo"
    torch.manual_seed(3)
    log = []
    rec = pretrain(agent, demo, None, epochs=30, minibatch=16, lr=1e-3, max_grad_norm=250.0, validation=demo, log=log.append)
    assert len(rec) == 30 and len(log) == 30 and all(r["steps"] == 1 for r in rec)
    for hd in range(2):
        print("head %d: NLL %.4f -> %.4f (accuracy %.3f -> %.3f)" % (hd, rec[0]["train_nll"][hd], rec[-1]["val_nll"][hd],
                                                                     rec[0]["train_accuracy"][hd], rec[-1]["val_accuracy"][hd]))
        assert rec[-1]["val_nll"][hd] < rec[0]["train_nll"][hd]
        assert abs(rec[0]["train_nll"][hd] - before[hd][1]) < 1e-5          # step 0 sees the untouched nets
    a = agent.arena                                                           # reset_optimizer: a fresh optimiser for PPO
    assert a.step == 0 and int(a.step_dev.item()) == 0
    assert float(a.exp_avg.abs().max()) == 0.0 and float(a.exp_avg_sq.abs().max()) == 0.0
    assert agent.learner.loss_mode == "ppo"
    # the validation form reports the training form's numbers on the same rows (same order, same kernels before the loss)
    idx = torch.randperm(16)
    r_eval, r_train = torch.zeros(2, F, device="cuda"), torch.zeros(2, F, device="cuda")
    l_eval = agent.imitate_from_storages(demo.batch(idx), stats_row=r_eval, evaluate=True)
    p0 = a.params.clone()
    l_train = agent.imitate_from_storages(demo.batch(idx), stats_row=r_train)
    assert l_eval == l_train and torch.equal(r_eval, r_train) and torch.equal(a.params, p0)
    kept = pretrain(agent, demo, None, epochs=1, minibatch=16, lr=1e-3, max_grad_norm=250.0, reset_optimizer=False)
    assert a.step == 1 and float(a.exp_avg.abs().max()) > 0 and "val_nll" not in kept[0]


def run_train_vec(tmp, **extra):
    from ppo_agent.train import train_vec
    from tests.helpers import SyntheticEnv, topology_cfgs
    train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp), T=8, episodes=1)
    train_cfg.update(extra)
    os.makedirs(str(tmp), exist_ok=True)
    agent = train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, 1, env_cls=SyntheticEnv, logger=None)
    torch.cuda.synchronize()
    return agent


def test_train_vec_with_and_without_a_pretrain_key(tmp_path):
    paths = record_episodes(tmp_path / "demos")
    absent = run_train_vec(tmp_path / "a")
    none = run_train_vec(tmp_path / "b", pretrain=None)
    assert torch.equal(absent.arena.params, none.arena.params) and absent.arena.step == none.arena.step == 2
    lines = []

    class Logger(object):
        def log(self, s):
            lines.append(s)
    from ppo_agent import train as train_mod
    from tests.helpers import SyntheticEnv, topology_cfgs
    train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path / "c"), T=8, episodes=1)
    train_cfg["pretrain"] = dict(episodes=os.path.dirname(paths[0]), epochs=2, minibatch=8, lr=1e-3, label_smoothing=0.1,
                                 balance="command", validation_fraction=0.5)
    os.makedirs(str(tmp_path / "c"), exist_ok=True)
    agent = train_mod.train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, 1, env_cls=SyntheticEnv, logger=Logger())
    torch.cuda.synchronize()
    assert sum(s.startswith("Pretrain epoch") for s in lines) == 2 and any("validation nll" in s for s in lines)
    assert agent.arena.step == 2                                              # PPO's own two steps: the warm start left no count
    assert not torch.equal(agent.arena.params, absent.arena.params) and bool(torch.isfinite(agent.arena.params).all())
