"""GPU: ordinal policy heads — cadre_ppo_loss_ord, the `_ord` sampling / eval / dist kernels and the agent-level paths
against the float64 statement of tests/ordinal_ref.py (never against the kernels themselves), plus the bit-identity of
the -1 marker and of `ordinal_policy` off with the existing entry points."""
import functools
import math

import numpy as np
import pytest
import torch

from cadre_amd import synth
from tests import ordinal_ref
from tests.test_ordinal_cpu import THROTTLE, shipped_steer

pytestmark = pytest.mark.gpu
CLIP, VC, CC, EC = 0.1, 0.1, 1.0, 0.01
# (B, C, K_steer, K_throttle, scale): B = 17 crosses the 16-rows-per-workgroup boundary, K = 64 fills the wave, K = 1 / 2 are
# the degenerate scans, scale = 4 saturates the sigmoids
CASES = [(1, 1, 1, 2, 1.0), (7, 4, 33, 3, 2.0), (16, 4, 33, 3, 1.0), (17, 4, 64, 3, 4.0), (200, 4, 33, 3, 4.0)]


def rel(a, b):
    a = np.asarray(torch.as_tensor(a).detach().cpu(), np.float64)
    b = np.asarray(torch.as_tensor(b).detach().cpu(), np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def random_rank(K, g):
    """A random non-identity permutation (K = 1 has only the identity)."""
    while True:
        r = torch.randperm(K, generator=g).tolist()
        if K == 1 or r != list(range(K)):
            return r


def ord_table(ranks):
    """[steer, throttle] rank lists (None: the -1 marker) -> device int32 [2][64]."""
    t = torch.zeros(2, 64, dtype=torch.int32)
    for h, r in enumerate(ranks):
        if r is None:
            t[h, 0] = -1
        else:
            t[h, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return t.cuda()


@functools.lru_cache(maxsize=None)
def loss_case(B, C, nS, nT, scale):
    """Inputs built like test_ppo_loss_fwd_bwd (ldl = 64) with a random non-identity rank per head, and the float64
    reference (losses, d total / d raw, d total / d value), computed once per case.  Old log-probs: even rows sit around the
    head's own log-prob (ratios near 1: both clip branches), odd rows around -log K as in test_ppo_loss_fwd_bwd (an
    ordinal head's log-probs spread with sqrt(K) * scale, so those ratios are far from 1)."""
    g = torch.Generator().manual_seed(1000 * B + nS)
    ldl, K = 64, (nS, nT)
    ranks = (random_rank(nS, g), random_rank(nT, g))
    logits = torch.zeros(2 * C, B, ldl)
    values = torch.randn(2 * C, B, generator=g)
    logits[:C, :, :nS] = torch.randn(C, B, nS, generator=g) * scale
    logits[C:, :, :nT] = torch.randn(C, B, nT, generator=g) * scale
    actions = torch.stack([torch.randint(0, nS, (B,), generator=g), torch.randint(0, nT, (B,), generator=g)])
    cmds = torch.randint(0, C, (2, B), generator=g, dtype=torch.int32)
    old_v = torch.randn(2, B, generator=g); rets = torch.randn(2, B, generator=g); adv = torch.randn(2, B, generator=g)
    old_lp = torch.zeros(2, B)
    for hd in range(2):
        own = logits[hd * C + cmds[hd].long(), torch.arange(B), :K[hd]]
        lp = ordinal_ref.normalised_logits(own, ranks[hd]).gather(1, actions[hd].view(-1, 1)).view(-1).float()
        flat = torch.full((B,), -math.log(K[hd]))
        old_lp[hd] = torch.where(torch.arange(B) % 2 == 0, lp, flat) + 0.3 * torch.randn(B, generator=g)
    inp = dict(logits=logits, values=values, actions=actions, cmds=cmds, old_v=old_v, rets=rets, old_lp=old_lp, adv=adv)
    ref = {}
    for name, rk in (("ord", ranks), ("steer_only", (ranks[0], None))):
        lg = logits.double().requires_grad_(True); vv = values.double().requires_grad_(True)
        tv, ta, te, total = ordinal_ref.ppo_loss(lg, vv, actions, cmds, old_v.double(), rets.double(), old_lp.double(),
                                                 adv.double(), K, rk, C, CLIP, VC, CC, EC)
        total.backward()
        ref[name] = (torch.tensor([float(tv.detach()), float(ta.detach()), float(te.detach())]), lg.grad, vv.grad)
    return inp, ranks, ref


def dev_inputs(inp):
    return {k: v.cuda() for k, v in inp.items()}


def hp_block():
    from cadre_amd import hip
    hp = torch.zeros(hip.HP_FIELDS, dtype=torch.float64)
    hp[hip.HP["lr"]], hp[hip.HP["clip"]], hp[hip.HP["value_coeff"]] = 3e-4, CLIP, VC
    hp[hip.HP["clip_coeff"]], hp[hip.HP["ent_coeff"]], hp[hip.HP["max_grad_norm"]] = CC, EC, 250.0
    return hp.cuda()


def new_outputs(B, C):
    out = dict(losses=torch.zeros(3, device="cuda"), dl=torch.full((2 * C, B, 64), 9.0, device="cuda"),
               dv=torch.full((2 * C, B), 9.0, device="cuda"), scratch=torch.full((4 + 6 * ((B + 15) // 16),), 3.0, device="cuda"))
    out["scratch"][0] = 0.0                                # the arrival counter: zero on first use, reset by every launch
    return out


def loss_args(d, o, B, C, nS, nT):
    return (d["logits"].data_ptr(), 64, B * 64, d["values"].data_ptr(), 1, B, d["actions"].data_ptr(), d["cmds"].data_ptr(),
            d["old_v"].data_ptr(), d["rets"].data_ptr(), d["old_lp"].data_ptr(), d["adv"].data_ptr(), B, C, nS, nT)


def loss_tail(o):
    return (1.0 / o["dl"].shape[1], o["losses"].data_ptr(), o["dl"].data_ptr(), o["dv"].data_ptr(), o["scratch"].data_ptr())


def run_ord(d, o, case, table, hp=None, stats=None, poison=None):
    from cadre_amd import hip
    B, C, nS, nT, _s = case
    st = (None, 0, None) if stats is None else (stats[0].data_ptr(), stats[0].shape[1], stats[1].data_ptr())
    hip.check(hip.lib().cadre_ppo_loss_ord(*loss_args(d, o, B, C, nS, nT), None if hp is None else hp.data_ptr(), CLIP, VC, CC, EC,
                                           *loss_tail(o), None if poison is None else poison.data_ptr(), *st, 0.0, None,
                                           table.data_ptr(), hip.stream()), "cadre_ppo_loss_ord")


def stats_bufs(B):
    return torch.zeros(2, 8, device="cuda"), torch.zeros(12 * ((B + 15) // 16), device="cuda")


# ----------------------------------------------------------------------------- loss forward and backward
@pytest.mark.parametrize("case", CASES)
def test_loss_ord_fwd_bwd(case):
    """Losses 1e-5, dvalues 1e-5, dlogits 2e-5 (relative to the largest reference magnitude: the bars of the categorical
    loss kernel) against float64 autograd; zero columns >= K; repeated launches and the four modes bit-identical; poison."""
    B, C, nS, nT, _scale = case
    inp, ranks, ref = loss_case(*case)
    want_l, want_dl, want_dv = ref["ord"]
    d, o, table = dev_inputs(inp), new_outputs(B, C), ord_table(ranks)
    run_ord(d, o, case, table)
    e_l, e_dv, e_dl = rel(o["losses"], want_l), rel(o["dv"], want_dv), rel(o["dl"], want_dl)
    print("case %s: losses %.2e dvalues %.2e dlogits %.2e" % (case, e_l, e_dv, e_dl))
    assert e_l < 1e-5 and e_dv < 1e-5 and e_dl < 2e-5, (e_l, e_dv, e_dl)
    assert float(o["dl"][:C, :, nS:].abs().max() if nS < 64 else 0.0) == 0.0 and float(o["dl"][C:, :, nT:].abs().max()) == 0.0
    first = {k: o[k].clone() for k in ("losses", "dl", "dv")}
    for _ in range(3):                                     # fixed combination order of the scans and of the loss sums
        run_ord(d, o, case, table)
        assert all(torch.equal(o[k], first[k]) for k in first)
    # device hyper block at the same values + a stats row: the same bits
    o2, srow = new_outputs(B, C), stats_bufs(B)
    run_ord(d, o2, case, table, hp=hp_block(), stats=srow)
    assert torch.equal(o2["losses"], first["losses"]) and torch.equal(o2["dl"], first["dl"]) and torch.equal(o2["dv"], first["dv"])
    for hd, K in enumerate((nS, nT)):                      # the diagnostics see the ordinal log-probs
        own = inp["logits"][hd * C + inp["cmds"][hd].long(), torch.arange(B), :K]
        lp = ordinal_ref.normalised_logits(own, ranks[hd]).gather(1, inp["actions"][hd].view(-1, 1)).view(-1)
        lr = lp - inp["old_lp"][hd].double()
        assert abs(float((-lr).mean()) - float(srow[0][hd, 1])) < 1e-5 * max(1.0, float(lr.abs().max()))
    assert float(srow[0][0, 6]) == 1.0
    for hp, st in ((hp_block(), None), (None, stats_bufs(B))):
        o3 = new_outputs(B, C)
        run_ord(d, o3, case, table, hp=hp, stats=st)
        assert torch.equal(o3["losses"], first["losses"]) and torch.equal(o3["dl"], first["dl"])
    poison = torch.ones(1, dtype=torch.int32, device="cuda")   # a reported forward-pass timeout: NaN losses
    run_ord(d, o, case, table, poison=poison)
    assert bool(torch.isnan(o["losses"]).all()) and torch.equal(o["dl"], first["dl"])


@pytest.mark.parametrize("case", CASES)
def test_loss_marker_heads_equal_the_categorical_kernels(case):
    """Steer ordinal + throttle -1: the throttle rows of dlogits are cadre_ppo_loss's, bit for bit, and the whole result
    matches the float64 statement of that mix.  Both heads -1: every output of cadre_ppo_loss / cadre_ppo_loss_stats."""
    from cadre_amd import hip
    B, C, nS, nT, _scale = case
    inp, ranks, ref = loss_case(*case)
    d = dev_inputs(inp)
    L = hip.lib()
    cat = new_outputs(B, C)
    hip.check(L.cadre_ppo_loss(*loss_args(d, cat, B, C, nS, nT), CLIP, VC, CC, EC, *loss_tail(cat), None, hip.stream()), "loss")
    mix = new_outputs(B, C)
    run_ord(d, mix, case, ord_table((ranks[0], None)))
    assert torch.equal(mix["dl"][C:], cat["dl"][C:]) and torch.equal(mix["dv"], cat["dv"])
    want_l, want_dl, want_dv = ref["steer_only"]
    assert rel(mix["losses"], want_l) < 1e-5 and rel(mix["dl"], want_dl) < 2e-5 and rel(mix["dv"], want_dv) < 1e-5
    off = new_outputs(B, C)
    none = ord_table((None, None))
    run_ord(d, off, case, none)
    assert all(torch.equal(off[k], cat[k]) for k in ("losses", "dl", "dv"))
    cat_s, srow_c = new_outputs(B, C), stats_bufs(B)
    hip.check(L.cadre_ppo_loss_stats(*loss_args(d, cat_s, B, C, nS, nT), CLIP, VC, CC, EC, *loss_tail(cat_s), None,
                                     srow_c[0].data_ptr(), 8, srow_c[1].data_ptr(), 0.0, None, hip.stream()), "loss_stats")
    off_s, srow_o = new_outputs(B, C), stats_bufs(B)
    run_ord(d, off_s, case, none, stats=srow_o)
    assert all(torch.equal(off_s[k], cat_s[k]) for k in ("losses", "dl", "dv")) and torch.equal(srow_o[0], srow_c[0])
    assert torch.equal(cat_s["losses"], cat["losses"])


# ----------------------------------------------------------------------------- sampling, eval, dist
MARGIN = 1e-3


@functools.lru_cache(maxsize=None)
def rows_case(K, R=64, seed=1):
    """(seed 1: the float64 margin filter below keeps every row at all four K; with 64 rows one dropped row is 1.6 %)"""
    g = torch.Generator().manual_seed(100 * K + seed)
    rank = random_rank(K, g)
    raw = torch.zeros(R, 64)
    raw[:, :K] = torch.randn(R, K, generator=g) * 2
    q = torch.ones(R, 64)
    q[:, :K] = torch.empty(R, K).exponential_(1, generator=g)
    acts = torch.randint(0, K, (R,), generator=g)
    lgn = ordinal_ref.normalised_logits(raw[:, :K], rank)
    return rank, raw, q, acts, lgn


def single_table(rank):
    return ord_table((rank, None))[0]


@pytest.mark.parametrize("K", [33, 3])
def test_sample_ord(K):
    from cadre_amd import hip
    L, R = hip.lib(), 64
    rank, raw, q, _acts, lgn = rows_case(K)
    want, margin = ordinal_ref.sample(lgn, q[:, :K])
    keep = margin > MARGIN
    assert float(keep.double().mean()) >= 0.99
    raw_d, q_d = raw.cuda(), q.cuda()
    out = []
    for table in (single_table(rank), single_table(None)):
        act = torch.empty(R, dtype=torch.int64, device="cuda"); lp = torch.empty(R, device="cuda")
        hip.check(L.cadre_sample_ord(raw_d.data_ptr(), 64, q_d.data_ptr(), 64, R, K, act.data_ptr(), lp.data_ptr(),
                                     table.data_ptr(), hip.stream()), "sample_ord")
        out.append((act.cpu(), lp.cpu()))
    act, lp = out[0]
    assert torch.equal(act[keep], want[keep])
    assert bool(((act >= 0) & (act < K)).all())
    assert rel(lp, lgn.gather(1, act.view(-1, 1)).view(-1)) < 1e-5
    a0 = torch.empty(R, dtype=torch.int64, device="cuda"); l0 = torch.empty(R, device="cuda")
    hip.check(L.cadre_sample(raw_d.data_ptr(), 64, q_d.data_ptr(), 64, R, K, a0.data_ptr(), l0.data_ptr(), hip.stream()), "sample")
    assert torch.equal(out[1][0], a0.cpu()) and torch.equal(out[1][1], l0.cpu())
    assert not torch.equal(act, a0.cpu())                  # (the ordinal head is a different distribution on the same raw rows)


def test_sample_rows_ord():
    """N = 5 environments, commands spread over C = 4, a non-trivial pos (rows sorted by command)."""
    from cadre_amd import hip
    from ppo_agent.agent import command_rows
    L, N, C, K = hip.lib(), 5, 4, (33, 3)
    g = torch.Generator().manual_seed(7)
    ranks = (random_rank(33, g), random_rank(3, g))
    cmd = [2, 0, 3, 0, 1]
    pos, _seg = command_rows(cmd, C)
    assert pos.tolist() != list(range(N))
    O3 = torch.randn(4 * C, N, 64, generator=g) * 2
    q = torch.ones(N, 2, 64)
    for h in range(2):
        q[:, h, :K[h]] = torch.empty(N, K[h]).exponential_(1, generator=g)
    O3_d, q_d = O3.cuda(), q.cuda()
    pos_d, cmd_d = torch.from_numpy(pos).cuda(), torch.tensor(cmd, dtype=torch.int32).cuda()

    def run(table, fn=None):
        act = torch.zeros(N, 2, dtype=torch.int64, device="cuda"); lp = torch.zeros(N, 2, device="cuda"); v = torch.zeros(N, 2, device="cuda")
        args = (O3_d.data_ptr(), 64, N * 64, pos_d.data_ptr(), cmd_d.data_ptr(), N, C, q_d.data_ptr(), K[0], K[1],
                act.data_ptr(), lp.data_ptr(), v.data_ptr())
        if table is None:
            hip.check(L.cadre_sample_rows(*args, hip.stream()), "sample_rows")
        else:
            hip.check(L.cadre_sample_rows_ord(*args, table.data_ptr(), hip.stream()), "sample_rows_ord")
        return act.cpu(), lp.cpu(), v.cpu()
    act, lp, v = run(ord_table(ranks))
    kept = 0
    for e in range(N):
        for h in range(2):
            z = 2 * (h * C + cmd[e])
            lgn = ordinal_ref.normalised_logits(O3[z, pos[e], :K[h]].view(1, -1), ranks[h])
            want, margin = ordinal_ref.sample(lgn, q[e, h, :K[h]].view(1, -1))
            if float(margin) > MARGIN:
                kept += 1
                assert int(act[e, h]) == int(want), (e, h)
            assert abs(float(lp[e, h]) - float(lgn[0, act[e, h]])) < 1e-5 * max(1.0, float(lgn.abs().max()))
            assert float(v[e, h]) == float(O3[z + 1, pos[e], 0])
    assert kept >= math.ceil(0.99 * 2 * N)
    for x, y in zip(run(ord_table((None, None))), run(None)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("K", [33, 3, 64, 1])
def test_eval_and_dist_ord(K):
    from cadre_amd import hip
    L, R = hip.lib(), 64
    rank, raw, _q, acts, lgn = rows_case(K)
    raw_d, acts_d = raw.cuda(), acts.cuda()

    def run(table):
        lp = torch.empty(R, device="cuda"); ent = torch.empty(R, device="cuda")
        lo = torch.empty(R, K, device="cuda"); pr = torch.empty(R, K, device="cuda"); mode = torch.empty(R, dtype=torch.int64, device="cuda")
        if table is None:
            hip.check(L.cadre_categorical_eval(raw_d.data_ptr(), 64, acts_d.data_ptr(), R, K, lp.data_ptr(), ent.data_ptr(),
                                               hip.stream()), "eval")
            hip.check(L.cadre_categorical_dist(raw_d.data_ptr(), 64, R, K, lo.data_ptr(), pr.data_ptr(), mode.data_ptr(),
                                               hip.stream()), "dist")
        else:
            hip.check(L.cadre_categorical_eval_ord(raw_d.data_ptr(), 64, acts_d.data_ptr(), R, K, lp.data_ptr(), ent.data_ptr(),
                                                   table.data_ptr(), hip.stream()), "eval_ord")
            hip.check(L.cadre_categorical_dist_ord(raw_d.data_ptr(), 64, R, K, lo.data_ptr(), pr.data_ptr(), mode.data_ptr(),
                                                   table.data_ptr(), hip.stream()), "dist_ord")
        return lp.cpu(), ent.cpu(), lo.cpu(), pr.cpu(), mode.cpu()
    lp, ent, lo, pr, mode = run(single_table(rank))
    want_lp = lgn.gather(1, acts.view(-1, 1)).view(-1)
    assert float((lp.double() - want_lp).abs().max()) < 1e-5 * max(1.0, float(want_lp.abs().max()))
    assert float((ent.double() - ordinal_ref.entropy(lgn)).abs().max()) < 1e-5 * max(1.0, float(ordinal_ref.entropy(lgn).max()))
    assert float((lo.double() - lgn).abs().max()) < 1e-5 * max(1.0, float(lgn.abs().max()))
    assert float((pr.double() - lgn.exp()).abs().max()) < 1e-5
    want, margin = ordinal_ref.top2_margin(lgn.exp())
    keep = margin > MARGIN
    assert float(keep.double().mean()) >= 0.99 and torch.equal(mode[keep], want[keep])
    for x, y in zip(run(single_table(None)), run(None)):
        assert torch.equal(x, y)


# ----------------------------------------------------------------------------- agent level
def make_agent(ordinal="absent", enc_seed=7, ppo_seed=11, command_num=4, act_graph=False):
    from ppo_agent.agent import CadreAgent
    H = W = 84
    fh, fw = synth.feat_hw(H, W)
    cfg = dict(use_lstm=True, vae_device=0, device_num=0, vae_params="CoPM", measurement_dim=18,
               num_output=dict(steer=33, throttle=3), command_num=command_num, obs_hw=(H, W), weights_init="none",
               vae_state_dict=synth.encoder_state(fh, fw, enc_seed), act_graph=act_graph)
    if ordinal != "absent":
        cfg["ordinal_policy"] = ordinal
    agent = CadreAgent(rank=0, model_cfg=cfg, frame=8, STEER_CONTROL=shipped_steer(), THROTTLE_CONTROL=THROTTLE, ent_coeff=EC,
                       value_coeff=VC, clip_coeff=CC, clip=CLIP)
    agent.arena.load_numpy_state(synth.ppo_state(ppo_seed, command_num=command_num))
    return agent


def obs_of(td, command=None):
    return dict(rgb=td["rgb"], route_fig=td["route_fig"].copy(), measurements=td["measurements"],
                command=td["command"] if command is None else command)


def new_storages(T, mbn=2):
    from ppo_agent.storage import RolloutStorage
    pair = [RolloutStorage(T, mbn, 530, 8, 530, True, 0.99, 0.95) for _ in range(2)]
    for s in pair:
        s.to("cuda:0")
    return pair


def section_first_row(agent, pair, hyper):
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    if hyper:
        agent.learner.set_device_hyper(True)
    st = {}
    learner_section(agent, pair[0], pair[1], False, dict(use_adv_norm=True, ppo_epoch=1, max_grad_norm=250.0, lr=3e-4), shared,
                    stats=st)
    torch.cuda.synchronize()
    return st["rows"][0]


def assert_on_policy(row):
    for h in range(2):
        assert abs(row["ratio_mean"][h] - 1.0) < 1e-5 and row["approx_kl"][h] < 1e-8, row


@pytest.mark.parametrize("hyper", [False, True])
def test_act_then_update_is_on_policy(hyper):
    """The log-prob stored at act time is the one the update recomputes: first minibatch step ratio_mean = 1, approx_kl = 0
    (act-time and update-time heads agree on transform and permutation), by-value and device-hyper mode."""
    T = 16
    agent = make_agent(True)
    assert agent.ordinal_rank[1] == [1, 0, 2] and agent.ordinal_rank[0][17] == 25 and agent.ordinal_rank[0][32] == 0
    assert agent.arena.ord[0, :33].tolist() == agent.ordinal_rank[0] and agent.arena.ord[1, :3].tolist() == [1, 0, 2]
    pair = new_storages(T)
    steps = synth.synth_rollout(T + 1, 84, 84, seed=12)
    torch.manual_seed(5)
    for i in range(T + 1):
        cmd = i % 4
        feat, action, alp, values, hidden = agent.act(obs_of(steps[i], cmd))
        for h in range(2):
            pair[h].insert(feat, action[h], alp[h], values[h], 0.1 * (i % 3), torch.tensor([[1.0]]), hidden, cmd)
    assert_on_policy(section_first_row(agent, pair, hyper))


def test_act_batch_then_update_is_on_policy():
    """The same check through act_batch + insert_batch with 3 environments (cadre_sample_rows_ord)."""
    from ppo_agent.storage import RolloutStorage
    T, N = 16, 3
    agent = make_agent(True)
    rollouts = [new_storages(T) for _ in range(N)]
    steps = [synth.synth_rollout(T + 1, 84, 84, seed=20 + e) for e in range(N)]
    torch.manual_seed(6)
    for i in range(T + 1):
        cmds = [(i + e) % 4 for e in range(N)]
        outs = agent.act_batch([obs_of(steps[e][i], cmds[e]) for e in range(N)])
        RolloutStorage.insert_batch(rollouts, outs, [[0.1, 0.2]] * N, [[1.0, 1.0]] * N, cmds)
    # each environment's storages against the weights that acted: a section steps the optimiser, so the parameters are put
    # back before the next environment's section (what update_model does after a weight pull)
    p0 = agent.arena.params.clone()
    for e, pair in enumerate(rollouts):
        agent.arena.params.copy_(p0)
        agent.learner._wp_key = None
        row = section_first_row(agent, pair, False)
        print("environment %d: ratio_mean %r approx_kl %r" % (e, row["ratio_mean"], row["approx_kl"]))
        assert_on_policy(row)


def _acts(agent, steps, seed=3):
    torch.manual_seed(seed)
    res = []
    for i, td in enumerate(steps):
        feat, a, lp, v, _hid = agent.act(obs_of(td, i % 2))
        res.append((feat.cpu(), int(a[0]), int(a[1]), lp[0].cpu(), lp[1].cpu(), v[0].cpu(), v[1].cpu()))
    return res, torch.rand(1).item()


def _same(x, y):
    return x[1] == y[1] and all(all(torch.equal(u, w) if torch.is_tensor(u) else u == w for u, w in zip(p, q))
                                for p, q in zip(x[0], y[0]))


def test_act_graph_equals_eager_chain():
    """_act_graphed (first pass, warm-up, capture, replay per (window mode, command)) == the eager chain, bit for bit."""
    steps = synth.synth_rollout(8, 84, 84, seed=33)
    graphed = make_agent(True, act_graph=True)
    assert graphed.learner._mode_key() == (("ord",),)
    assert _same(_acts(make_agent(True), steps), _acts(graphed, steps))
    assert len(graphed._ag["graphs"]) >= 1


def test_off_means_off():
    """An agent built with ordinal_policy=False == one built without the key: act() outputs and update losses / gradients
    from the same seeds, bit for bit, with the plain entry points and graph keys."""
    from tests.test_ppo_stats_gpu import dev, samples
    steps = synth.synth_rollout(4, 84, 84, seed=33)
    absent, off = make_agent(), make_agent(False)
    assert absent.ordinal_rank is None and off.ordinal_rank is None and off.arena.ord is None
    assert _same(_acts(absent, steps), _acts(off, steps))
    smp = samples(24, 4, 3)
    la = absent.update_policy(dev(smp[0]), dev(smp[1]))
    lo = off.update_policy(dev(smp[0]), dev(smp[1]))
    assert la == lo and torch.equal(absent.arena.grads, off.arena.grads)
    assert absent.learner._mode_key() == () and off.learner._mode_key() == ()


def test_ensemble_act_of_ordinal_agents():
    """ensemble_act of two ordinal agents (different nets, one encoder checkpoint) == the per-agent loop."""
    from ppo_agent.agent import CadreAgent
    group = [make_agent(True, ppo_seed=11), make_agent(True, ppo_seed=12)]
    td = synth.synth_rollout(1, 84, 84, seed=33)[0]
    torch.manual_seed(9)
    ens = CadreAgent.ensemble_act(group, obs_of(td))
    torch.manual_seed(9)
    loop = [a.act(obs_of(td)) for a in group]
    for x, y in zip(ens, loop):
        assert int(x[1][0]) == int(y[1][0]) and int(x[1][1]) == int(y[1][1])
        assert torch.equal(x[2][0], y[2][0]) and torch.equal(x[2][1], y[2][1]) and torch.equal(x[3][0], y[3][0])


def test_update_policy_matches_module_autograd_per_param():
    """Parameter gradients of one fused update_policy against the module-level autograd path (LSTM.forward +
    Model.evaluate_actions with the ordinal tail in torch: an independent implementation of the same head), at the bar of
    test_update_policy_matches_oracle_autograd_per_param (2e-4 of the model's largest |g|)."""
    from tests.test_ppo_stats_gpu import dev, samples
    B, C = 24, 4
    agent = make_agent(True)
    smp = [dev(s) for s in samples(B, C, 4)]
    # old log-probs near the ordinal head's own, so that the ratios exercise both clip branches
    with torch.no_grad():
        for hd, head in enumerate(("steer", "throttle")):
            obs, act, _ov, _ret, _m, old_lp, _adv, hidden, cmd = smp[hd]
            for c in range(C):
                h, _ = agent.model_dict["%s_lstm_%d" % (head, c)](obs, (hidden[0], hidden[1]))
                _v, lp, _e = agent.model_dict["%s_ppo_%d" % (head, c)].evaluate_actions(h, act)
                m = (cmd == c).view(-1, 1)
                old_lp[m] = (lp + (old_lp + math.log((33, 3)[hd])))[m]
    got = agent.update_policy(smp[0], smp[1])
    fused = agent.arena.grads.clone()
    agent.arena.grads.zero_()
    tot_v = tot_a = tot_e = 0
    for hd, head in enumerate(("steer", "throttle")):
        obs, act, old_v, ret, _m, old_lp, adv, hidden, cmd = smp[hd]
        cur_v = cur_lp = ent = 0
        for c in range(C):
            h, _ = agent.model_dict["%s_lstm_%d" % (head, c)](obs, (hidden[0], hidden[1]))
            v, lp, e = agent.model_dict["%s_ppo_%d" % (head, c)].evaluate_actions(h, act)
            m = (cmd == c).view(-1, 1).float()
            cur_v, cur_lp, ent = cur_v + v * m, cur_lp + lp * m, ent + e * m
        ratio = torch.exp(cur_lp - old_lp)
        tot_a = tot_a - torch.min(ratio * adv, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * adv).mean()
        vpc = old_v + (cur_v - old_v).clamp(-CLIP, CLIP)
        tot_v = tot_v + 0.5 * torch.max((cur_v - ret).pow(2), (vpc - ret).pow(2)).mean()
        tot_e = tot_e + ent.mean()
    (tot_v * VC + tot_a * CC - tot_e * EC).backward()
    assert rel(got, [float(tot_v * VC), float(tot_a * CC), float(tot_e * EC)]) < 1e-4
    a, worst = agent.arena, 0.0
    for mn in a.model_names():
        gf, gm = a.views(fused, mn), a.views(a.grads, mn)
        scale = max(float(t.abs().max()) for t in gm.values())
        assert scale > 0
        for k in gm:
            err = float((gf[k] - gm[k]).abs().max()) / max(scale, 1e-12)
            worst = max(worst, err)
            assert err < 2e-4, (mn, k, err)
    print("worst per-parameter gradient error (rel. to model max |g|): %.2e" % worst)
