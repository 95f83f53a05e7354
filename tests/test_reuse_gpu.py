"""GPU: sample reuse — cadre_vtrace_multi against cadre_gae_multi (on-policy: bit for bit) and against the fp32 emulation of
tests/reuse_ref.py run from the kernel's own stored ratio (off-policy: bit for bit; expf itself against float64 at
update_parity.T_EXP ulps), cadre_reuse_record at the running bound of tests/loss_parity.py and its exact statement with
cadre_ppo_loss_stats, the window through learner_section_multi, and train_cfg["sample_reuse"] in train_vec."""
import os
import types

import numpy as np
import pytest
import torch

from tests import loss_parity as lp
from tests import reuse_ref as rr
from tests import update_parity

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
GAMMA, TAU = 0.99, 0.95
G32, GT32 = float(f32(GAMMA)), float(f32(GAMMA * TAU))
SENT = 7.25                                        # what no launch addressed keeps this bit pattern
SCALES, CLIP_R = (0.37, 1.9), 0.8                  # a reward-scaler state: (steer, throttle) scales, clip


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ----------------------------------------------------------------------------- cadre_vtrace_multi
class Scan(object):
    """n storages of T rows as both kernels' tables address them.  lr: fp32 [n][T] log-ratio to plant (None: on-policy)."""

    def __init__(self, n, T, seed, flags, lr=None, mu=None):
        r = np.random.RandomState(seed)
        self.n, self.T = n, T
        self.rew = (r.rand(n, T + 1) * 2.0 - 0.5).astype(f32)
        self.V = (r.randn(n, T + 1) * 0.3).astype(f32)
        self.m = (r.rand(n, T + 1) >= 0.1).astype(f32)
        self.tl = {"none": None, "zeros": np.zeros((n, T + 1), f32), "random": (r.rand(n, T + 1) < 0.2).astype(f32)}[flags]
        self.boot = (np.arange(n) % 2 == 0).astype(f32)               # boot_keep 1, 0, 1, ...
        self.V[n - 1, T] = f32(-0.75)                                 # the last storage: a negative value_now[T] ...
        self.boot[n - 1] = 0.0                                        # ... of a finished rollout
        self.mu = (r.randn(n, T) * 0.7 - 1.0).astype(f32) if mu is None else mu
        self.logp = self.mu.copy() if lr is None else (self.mu + lr).astype(f32)
        self.state = np.zeros(8 + 2 * n, f64)
        self.state[6:8] = SCALES

    def gae(self, normalise, scaled):
        """cadre_gae_multi on value_preds = value_now, next_value = the select: (returns, adv, value_preds[T]) per storage."""
        from cadre_amd import hip
        n, T = self.n, self.T
        d = dict(rew=dev(self.rew), V=dev(self.V), m=dev(self.m), nv=dev(np.where(self.boot != 0, self.V[:, T], f32(0.0)).astype(f32)),
                 ret=torch.full((n, T + 1), SENT, device="cuda"), adv=torch.full((n, T), SENT, device="cuda"))
        tl = None if self.tl is None else dev(self.tl)
        rows = [[d["rew"][k].data_ptr(), d["V"][k].data_ptr(), d["m"][k].data_ptr(), d["nv"][k:].data_ptr(), d["ret"][k].data_ptr(),
                 d["adv"][k].data_ptr(), 0 if tl is None else tl[k].data_ptr()] for k in range(n)]
        table = torch.tensor(rows, dtype=torch.int64).cuda()
        state = dev(self.state) if scaled else None
        hip.check(hip.lib().cadre_gae_multi(table.data_ptr(), n, T, G32, GT32, int(normalise), None if state is None else state.data_ptr(),
                                            CLIP_R if scaled else 0.0, hip.stream()), "cadre_gae_multi")
        return host(d["ret"])[:, :T], host(d["adv"]), host(d["V"])[:, T]

    def vtrace(self, normalise, scaled, rho_bar, c_bar):
        from cadre_amd import hip
        n, T = self.n, self.T
        d = dict(rew=dev(self.rew), V=dev(self.V), m=dev(self.m), boot=dev(self.boot), mu=dev(self.mu), logp=dev(self.logp),
                 ret=torch.full((n, T + 3), SENT, device="cuda"), adv=torch.full((n, T + 3), SENT, device="cuda"),
                 ratio=torch.full((n, T + 3), SENT, device="cuda"), diag=torch.full((n, 4 + 2), SENT, device="cuda"))
        tl = None if self.tl is None else dev(self.tl)
        rows = [[d["rew"][k].data_ptr(), d["m"][k].data_ptr(), 0 if tl is None else tl[k].data_ptr(), d["V"][k].data_ptr(),
                 d["boot"][k:].data_ptr(), d["mu"][k].data_ptr(), d["logp"][k].data_ptr(), d["ret"][k].data_ptr(),
                 d["adv"][k].data_ptr(), d["ratio"][k].data_ptr(), d["diag"][k].data_ptr()] for k in range(n)]
        table = torch.tensor(rows, dtype=torch.int64).cuda()
        state = dev(self.state) if scaled else None
        hip.check(hip.lib().cadre_vtrace_multi(table.data_ptr(), n, T, G32, GT32, int(normalise),
                                               None if state is None else state.data_ptr(), CLIP_R if scaled else 0.0,
                                               rho_bar, c_bar, hip.stream()), "cadre_vtrace_multi")
        out = {k: host(d[k]) for k in ("ret", "adv", "ratio", "diag", "V")}
        for k in ("ret", "adv", "ratio"):                             # the guard band behind the T rows is untouched
            assert (out[k][:, T:] == f32(SENT)).all(), k
            out[k] = out[k][:, :T]
        assert (out["diag"][:, 4:] == f32(SENT)).all()
        out["diag"] = out["diag"][:, :4]
        for k, src in (("rew", self.rew), ("m", self.m), ("mu", self.mu), ("logp", self.logp), ("boot", self.boot)):
            assert np.array_equal(bits(host(d[k])), bits(src)), k     # the inputs are not written
        assert np.array_equal(bits(out["V"][:, :T]), bits(self.V[:, :T]))
        return out


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("T", [2, 3, 63, 64, 65, 130])
def test_vtrace_multi_on_policy_is_gae_multi_bit_for_bit(n, T):
    for flags in ("none", "zeros", "random"):
        c = Scan(n, T, 1000 * n + T, flags)
        for normalise in (0, 1):
            for scaled in (False, True):
                ret, adv, vT = c.gae(normalise, scaled)
                for bars in ((1.0, 1.0), (2.5, 1.5)):
                    o = c.vtrace(normalise, scaled, *bars)
                    tag = (flags, normalise, scaled, bars)
                    assert np.array_equal(bits(o["ret"]), bits(ret)), tag
                    assert np.array_equal(bits(o["adv"]), bits(adv)), tag
                    assert np.array_equal(bits(o["V"][:, T]), bits(vT)), tag
                    assert (bits(o["ratio"]) == bits(np.ones(1, f32))[0]).all(), tag
                    assert np.array_equal(bits(o["diag"]), bits(np.tile(np.array([1, 0, 0, 1], f32), (n, 1)))), tag
        assert o["V"][n - 1, T] == 0 and bits(o["V"][n - 1:, T])[0] == 0              # the select: +0, not -0
    # the all-zero flag array gives the bits of NULL
    a, b = Scan(n, T, 1000 * n + T, "none").vtrace(1, False, 1.0, 1.0), Scan(n, T, 1000 * n + T, "zeros").vtrace(1, False, 1.0, 1.0)
    assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


@pytest.mark.parametrize("bars", [(1.0, 1.0), (2.0, 0.5), (1e6, 1e6)])
@pytest.mark.parametrize("T", [8, 65, 130])
def test_vtrace_multi_off_policy_against_the_emulation(T, bars):
    """Stage by stage: the stored ratio against float64 exp of the fp32 difference, then returns / advantages bit for bit
    against the emulation run from that stored ratio, then the diagnostics within 2 fp32 ulps of float64."""
    n = 3
    r = np.random.RandomState(T)
    lr = (r.randn(n, T) * 0.5).astype(f32)
    mu = (r.randn(n, T) * 0.7 - 1.0).astype(f32)
    for k in range(n):                                                 # planted rows: mu = 0, so the difference is the plant itself
        plant = np.array([20.0, -20.0, 0.0, -0.0, np.log(f64(f32(bars[0])))], f64).astype(f32)
        at = r.permutation(T)[:5]
        mu[k, at], lr[k, at] = 0.0, plant
    worst = 0.0
    for flags, scaled in (("random", True), ("none", False)):
        c = Scan(n, T, 77 + T, flags, lr=lr, mu=mu)
        d = (c.logp - c.mu).astype(f32)                                # the kernel's one fp32 subtraction
        for normalise in (0, 1):
            o = c.vtrace(normalise, scaled, *bars)
            u = rr.ulps32(o["ratio"], np.exp(d.astype(f64)))
            worst = max(worst, float(u.max()))
            assert u.max() <= update_parity.T_EXP, (flags, normalise, float(u.max()))
            assert (o["ratio"][d == 0] == 1).all()
            for k in range(n):
                keep = None if c.tl is None else (f32(1.0) - c.tl[k]).astype(f32)
                ret, adv, vT = rr.vtrace32(c.rew[k], c.V[k], c.m[k], keep, o["ratio"][k], c.boot[k], f32(G32), f32(GT32), bars[0],
                                           bars[1], normalise, scale=SCALES[k & 1] if scaled else None, clip=CLIP_R if scaled else None)
                assert np.isfinite(o["ret"][k]).all() and np.isfinite(o["adv"][k]).all()
                assert np.array_equal(bits(o["ret"][k]), bits(ret)), (flags, normalise, k)
                assert np.array_equal(bits(o["adv"][k]), bits(adv)), (flags, normalise, k)
                assert bits(o["V"][k, T:])[0] == bits(np.array([vT], f32))[0]
                du = rr.ulps32(o["diag"][k], rr.diag64(d[k], o["ratio"][k], bars[0]))
                assert du.max() <= 2.0, (flags, normalise, k, du)
    print("T %d bars %s: stored ratio worst %.2f ulps of float64 exp (bound %g)" % (T, bars, worst, update_parity.T_EXP))


# ----------------------------------------------------------------------------- cadre_reuse_record
class Record(object):
    def __init__(self, B, C, K, ldl, ordinal, sorted_pos, seed):
        r = np.random.RandomState(seed)
        self.B, self.C, self.K, self.ldl, self.ordinal = B, C, K, ldl, ordinal
        self.R = 2 * B + 3
        self.logits = np.full((2 * C, B, ldl), 3.25, f32)              # (columns K .. ldl - 1 hold junk no lane may read)
        for hd in range(2):
            for c in range(C):
                self.logits[hd * C + c, :, :K[hd]] = lp.raw_rows(r, B, K[hd], 4.0, ordinal)
        self.values = r.randn(2 * C, B).astype(f32)
        self.cmds = r.randint(0, C, (2, B)).astype(np.int32)
        self.actions = np.stack([r.randint(0, K[hd], B) for hd in range(2)]).astype(np.int64)
        self.pos = np.stack([r.permutation(B) for _ in range(2)]).astype(np.int32) if sorted_pos else None
        self.row_id = np.stack([r.permutation(self.R)[:B] for _ in range(2)]).astype(np.int64)
        self.ord = np.stack([lp.rank_table(K[hd], ordinal) for hd in range(2)]).astype(np.int32)

    def launch(self, cmds=None, actions=None, pos=None, row_id=None):
        from cadre_amd import hip
        B, C, K, R = self.B, self.C, self.K, self.R
        d = dict(logits=dev(self.logits), values=dev(self.values), cmds=dev(self.cmds if cmds is None else cmds),
                 actions=dev(self.actions if actions is None else actions), row_id=dev(self.row_id if row_id is None else row_id))
        pos = self.pos if pos is None else pos
        pos_d = None if pos is None else dev(pos)
        ord_d = dev(self.ord) if self.ordinal else None
        logp = torch.full((2 * R + 16,), SENT, device="cuda")
        value = torch.full((2 * R + 16,), SENT, device="cuda")
        hip.check(hip.lib().cadre_reuse_record(
            d["logits"].data_ptr(), self.ldl, B * self.ldl, d["values"].data_ptr(), 1, B, d["cmds"].data_ptr(), d["actions"].data_ptr(),
            None if pos_d is None else pos_d.data_ptr(), d["row_id"].data_ptr(), B, C, K[0], K[1],
            None if ord_d is None else ord_d.data_ptr(), logp.data_ptr(), value.data_ptr(), R, hip.stream()), "cadre_reuse_record")
        lo, vo = host(logp), host(value)
        assert (lo[2 * R:] == f32(SENT)).all() and (vo[2 * R:] == f32(SENT)).all()              # the guard band
        return lo[:2 * R].reshape(2, R), vo[:2 * R].reshape(2, R), d, ord_d

    def rows(self, hd):
        """(unsorted row u, workspace position b, command c, table row r) of head hd."""
        u = np.arange(self.B)
        b = u if self.pos is None else self.pos[hd]
        return u, b, self.cmds[hd][b], self.row_id[hd]


RECORD_CASES = [(B, C, K, ldl, ordinal, srt)
                for B in (1, 15, 16, 17, 33) for C in (1, 4) for K, ldl in (((33, 3), 64), ((33, 3), 40), ((1, 64), 64))
                for ordinal, srt in ((False, False), (True, True), (False, True) if B == 17 else (True, False))]


@pytest.mark.parametrize("B,C,K,ldl,ordinal,srt", RECORD_CASES)
def test_reuse_record(B, C, K, ldl, ordinal, srt):
    from cadre_amd import hip
    c = Record(B, C, K, ldl, ordinal, srt, seed=100 * B + 10 * C + K[0] + ldl)
    logp, value, d, ord_d = c.launch()
    R = c.R
    rep = lp.Report("cadre_reuse_record B %d C %d K %s ldl %d %s %s" % (B, C, K, ldl, "ordinal" if ordinal else "categorical",
                                                                        "sorted" if srt else "identity"))
    old_lp = np.zeros((2, B), f32)
    for hd in range(2):
        u, b, cm, rid = c.rows(hd)
        x = c.logits[hd * C + cm, b, :K[hd]]
        rk = c.ord[hd, :K[hd]].astype(np.int64) if ordinal else None
        _X, lg, _pk, _H = lp.front_reference(x, rk)
        a = c.actions[hd][b]
        want = lp.VE(np.zeros(R), np.zeros(R))
        want.v[rid], want.e[rid] = lg.v[u, a], lg.e[u, a]
        mask = np.zeros(R, bool)
        mask[rid] = True
        rep.check("logp_now[%d]" % hd, logp[hd], want, mask, f32(SENT))
        assert np.array_equal(bits(value[hd][rid]), bits(c.values[hd * C + cm, b]))             # the same bits
        assert (value[hd][~mask] == f32(SENT)).all()
        old_lp[hd, b] = logp[hd][rid]
    rep.finish()
    # the exact statement: the same logits, old_logp := logp_now -> ratio == expf(0) == 1 in every row
    r = np.random.RandomState(B)
    nblk = (B + 15) // 16
    o = dict(old_v=dev(r.randn(2, B).astype(f32)), rets=dev(r.randn(2, B).astype(f32)), adv=dev(r.randn(2, B).astype(f32)),
             old_lp=dev(old_lp), losses=torch.zeros(3, device="cuda"), dl=torch.zeros(2 * C, B, ldl, device="cuda"),
             dv=torch.zeros(2 * C, B, device="cuda"), scratch=torch.zeros(4 + 6 * nblk, device="cuda"),
             poison=torch.zeros(1, dtype=torch.int32, device="cuda"), stats=torch.full((2, 8), SENT, device="cuda"),
             sscr=torch.zeros(12 * nblk, device="cuda"))
    head = (d["logits"].data_ptr(), ldl, B * ldl, d["values"].data_ptr(), 1, B, d["actions"].data_ptr(), d["cmds"].data_ptr(),
            o["old_v"].data_ptr(), o["rets"].data_ptr(), o["old_lp"].data_ptr(), o["adv"].data_ptr(), B, C, K[0], K[1])
    tail = (0.1, 0.1, 1.0, 0.01, 1.0 / B, o["losses"].data_ptr(), o["dl"].data_ptr(), o["dv"].data_ptr(), o["scratch"].data_ptr(),
            o["poison"].data_ptr(), o["stats"].data_ptr(), 8, o["sscr"].data_ptr(), 0.0, None)
    if ordinal:
        hip.check(hip.lib().cadre_ppo_loss_ord(*head, None, *tail, ord_d.data_ptr(), hip.stream()), "cadre_ppo_loss_ord")
    else:
        hip.check(hip.lib().cadre_ppo_loss_stats(*head, *tail, hip.stream()), "cadre_ppo_loss_stats")
    st = host(o["stats"])
    assert (st[:, 4] == 1.0).all() and (st[:, 0] == 0.0).all() and (st[:, 5] == 0.0).all() and (st[:, 2] == 0.0).all(), st
    # rows with a bad command, position, row id or action leave their elements at the sentinel
    if B < 15:
        return
    u0, u1, u2, u3 = 0, 3, 7, 11
    cmds, actions, row_id = c.cmds.copy(), c.actions.copy(), c.row_id.copy()
    pos = None if c.pos is None else c.pos.copy()
    skip = [set(), set()]                                               # table rows that stay at the sentinel
    for hd in range(2):
        _u, b, _cm, rid = c.rows(hd)
        cmds[hd, b[u0]] = C if hd == 0 else -1
        skip[hd].add(rid[u0])
        if pos is not None:
            pos[hd, u1] = B if hd == 0 else -1
            skip[hd].add(rid[u1])
        row_id[hd, u2] = R if hd == 0 else -1
        skip[hd].add(rid[u2])
        actions[hd, b[u3]] = K[hd] if hd == 0 else -1
    logp2, value2, _d, _o = c.launch(cmds=cmds, actions=actions, pos=pos, row_id=row_id)
    for hd in range(2):
        _u, b, _cm, rid = c.rows(hd)
        for rrow in range(R):
            if rrow in skip[hd]:
                assert logp2[hd, rrow] == f32(SENT) and value2[hd, rrow] == f32(SENT), (hd, rrow)
            elif rrow == rid[u3]:                                       # no action: the value only
                assert logp2[hd, rrow] == f32(SENT) and bits(value2[hd, rrow:])[0] == bits(value[hd, rrow:])[0]
            else:
                assert bits(logp2[hd, rrow:])[0] == bits(logp[hd, rrow:])[0] and bits(value2[hd, rrow:])[0] == bits(value[hd, rrow:])[0]


# ----------------------------------------------------------------------------- the window through learner_section_multi
T_E2E, MBN, N_ENV, M_WIN = 16, 4, 2, 2


def e2e_cfg(**kw):
    d = dict(use_adv_norm=True, ppo_epoch=1, max_grad_norm=250.0, lr=3e-4)
    d.update(kw)
    return d


def section_rollouts(section):
    from tests.test_ppo_stats_gpu import storages
    return [storages(T_E2E, MBN, 500 + 10 * section + w) for w in range(N_ENV)]


def run_sections(tmp, with_window, sections=3):
    """`sections` learner sections of a fresh agent on fixed synthetic rollouts; per section (losses, parameters, the global
    generator's state, stats, C-ABI calls of the section)."""
    from cadre_amd import hip
    from cadre_amd.reuse import ReuseWindow
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section_multi
    from tests.test_imitation_gpu import make_agent
    agent = make_agent(tmp)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    win = ReuseWindow(agent, M_WIN, N_ENV, T_E2E, seed=3) if with_window else None
    torch.manual_seed(77)
    out, last = [], None
    for e in range(sections):
        rollouts, dones = section_rollouts(e), [False, e == 1]
        st = {}
        kw = dict(reuse=win) if with_window else {}
        n0 = hip.N_CALLS
        losses = learner_section_multi(agent, rollouts, dones, e2e_cfg(), shared, stats=st, episode=e, **kw)
        out.append((losses, agent.arena.params.clone(), torch.get_rng_state().clone(), st, hip.N_CALLS - n0))
        if win is not None:
            win.append(rollouts, dones)
        last = rollouts
    torch.cuda.synchronize()
    return agent, win, out, last


def test_window_through_learner_section_multi(tmp_path):
    agent, win, with_w, last = run_sections(tmp_path / "a", True)
    _agent0, _none, plain, _l = run_sections(tmp_path / "b", False)
    _agent2, _win2, again, _l2 = run_sections(tmp_path / "c", True)
    # (a) window empty: losses, parameters and the global generator are those of the call without `reuse`
    assert with_w[0][0] == plain[0][0] and torch.equal(with_w[0][1], plain[0][1]) and with_w[0][3]["reuse"] == dict(filled=0)
    assert "reuse" not in plain[0][3]
    assert with_w[0][4] == plain[0][4] and with_w[1][4] > plain[1][4]   # the launch census: an empty window adds no call
    for e in range(3):                                                 # the window never draws from the global generator
        assert torch.equal(with_w[e][2], plain[e][2]), e
    # (c) after three sections
    Bw = T_E2E // MBN
    assert [s[3]["reuse"]["filled"] for s in with_w] == [0, 1, 2]
    for B in (1, 2, 3):                                                 # the steps ran (1 + filled) N entries
        assert (B * N_ENV * Bw, agent.arena.Z, agent.learner.S) in agent.learner._ws
    assert (4 * N_ENV * Bw, agent.arena.Z, agent.learner.S) not in agent.learner._ws
    assert not torch.equal(with_w[2][1], plain[2][1]) and bool(torch.isfinite(with_w[2][1]).all())
    assert not torch.equal(with_w[1][1], plain[1][1])
    r = with_w[2][3]["reuse"]
    print("section 2 reuse stats: %s" % (r,))
    for k in ("ratio_mean", "truncated", "max_abs_log_ratio", "effective_sample_share"):
        assert len(r[k]) == 2 and all(np.isfinite(v) for v in r[k]), k
    assert all(0.0 <= v <= 1.0 for v in r["truncated"] + r["effective_sample_share"])
    assert (win.filled, win.next) == (2, 1)                             # the oldest slot was overwritten by the third section
    P = T_E2E + 1
    for e_, (s, t) in enumerate(last):
        lo = win.base(0, e_)
        assert torch.equal(win.steer._obs[lo:lo + P], s._obs) and torch.equal(win.mu[1, lo:lo + P], t.action_log_probs)
        assert torch.equal(win.steer.rewards[lo:lo + P], s.rewards) and torch.equal(win.throttle.action[lo:lo + P], t.action)
    assert win.boot_keep.tolist() == [1.0, 1.0, 1.0, 0.0]               # slot 0: section 2 (no done), slot 1: section 1 (done, env 1)
    # (e) determinism
    for e in range(3):
        assert again[e][0] == with_w[e][0] and torch.equal(again[e][1], with_w[e][1]), e


def test_refresh_then_the_same_pass_finds_ratio_one_and_the_float64_targets(tmp_path):
    """After one append, before any optimiser step.  The record pass and an update over the record pass's own index vectors
    are the same chain on the same inputs: max |log ratio| == 0 and approx_kl == 0 for the stale rows.  The stale returns /
    advantages: bit-equal to the fp32 emulation run on the recorded tables (what the rollout-finish tests hold their scans to),
    and within the fp32 error bound of tests/test_reuse_cpu.py (12 T 2^-24 of the largest magnitude) of the float64 V-trace."""
    from cadre_amd.reuse import ReuseWindow
    from tests.test_imitation_gpu import make_agent
    agent = make_agent(tmp_path)
    rho_bar, c_bar = 1.5, 0.8
    win = ReuseWindow(agent, M_WIN, N_ENV, T_E2E, rho_bar=rho_bar, c_bar=c_bar)
    rollouts, dones = section_rollouts(0), [False, True]
    win.append(rollouts, dones)
    win.refresh(True)
    lrn = agent.learner
    lrn.set_update_modes(stats=True)
    try:
        for idx in win.record_batches():
            row = torch.zeros(2, lrn.stats_fields(), device="cuda")
            agent.update_policy_from_storages(win.entry(idx), sync=False, stats_row=row)
            st = row.cpu()
            assert float(st[:, 5].abs().max()) == 0.0 and float(st[:, 0].abs().max()) == 0.0, st[:, :6]
    finally:
        lrn.set_update_modes()
    T, P = T_E2E, T_E2E + 1
    diag = host(win.stats()).reshape(N_ENV, 2, 4)
    for e, pair in enumerate(rollouts):
        lo = win.base(0, e)
        for h, (src, big) in enumerate(zip(pair, (win.steer, win.throttle))):
            g = lambda t: host(t[lo:lo + P].reshape(-1))
            V, logp, mu, ratio = g(win.value_now[h]), g(win.logp_now[h])[:T], g(win.mu[h])[:T], g(win.ratio[h])[:T]
            rew, m = host(src.rewards[:, 0]), host(src.masks[:, 0])
            keep_boot = 0.0 if dones[e] else 1.0
            assert V[T] == 0.0 if dones[e] else V[T] != 0.0
            d = (logp - mu).astype(f32)
            assert rr.ulps32(ratio, np.exp(d.astype(f64))).max() <= update_parity.T_EXP
            V_in = V.copy()                                             # (V[T] was overwritten with the bootstrap: the select is idempotent)
            ret, adv, _vT = rr.vtrace32(rew, V_in, m, None, ratio, keep_boot, f32(G32), f32(GT32), rho_bar, c_bar, True)
            got_ret, got_adv = g(big.returns)[:T], host(big.advantages[lo:lo + T, 0])
            assert np.array_equal(bits(got_ret), bits(ret)) and np.array_equal(bits(got_adv), bits(adv)), (e, h)
            vs, A, rho = rr.vtrace64(rew, V_in, m, None, ratio, keep_boot, G32, GT32 / G32, rho_bar, c_bar)
            want = rr.finish64(A, rho, True)
            mag = max(1.0, np.abs(V_in).max(), np.abs(vs - V_in[:T]).max(), np.abs(A).max(), rho.max() * 4.0)
            tol = 12 * T * 2.0 ** -24 * mag
            assert np.abs(got_ret - vs).max() <= tol and np.abs(got_adv - want).max() <= tol * rho.max() * 3.0 / A.std(ddof=1)
            assert rr.ulps32(diag[e, h], rr.diag64(d, ratio, rho_bar)).max() <= 2.0
    print("synthetic behaviour log-probabilities: max |log ratio| per stale storage %s" % diag[:, :, 2].tolist())


def test_demo_mix_composes_and_n_ppo_counts_the_stale_rows(tmp_path):
    from cadre_amd.reuse import ReuseWindow
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section_multi
    from tests.test_imitation_gpu import make_agent, random_demo
    agent = make_agent(tmp_path)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    win = ReuseWindow(agent, M_WIN, N_ENV, T_E2E)
    win.append(section_rollouts(0), [False, False])
    demo_set, _host = random_demo(agent, 40, seed=3)
    Bw = T_E2E // MBN
    mixer = types.SimpleNamespace(label_smoothing=0.0, entries=lambda rows, episode, step: demo_set.batch(torch.arange(rows) + step))
    st = {}
    losses = learner_section_multi(agent, section_rollouts(1), [False, False], e2e_cfg(), shared, stats=st, demo=mixer, episode=1,
                                   reuse=win)
    assert len(losses[0]) == MBN and all(np.isfinite(v) for col in losses for v in col)
    n_ppo = (1 + 1) * N_ENV * Bw                                        # live and stale rows are PPO rows, the demonstration rows follow
    w = agent.learner.workspace(n_ppo + Bw)
    kind = w["row_kind"].cpu()
    assert int(kind.sum()) == 2 * Bw and st["reuse"]["filled"] == 1 and "demo" in st
    pos = None if not agent.learner.sorted_rows(n_ppo + Bw) else w["pos"].cpu()
    for hd in range(2):
        at = torch.arange(n_ppo + Bw) if pos is None else pos[hd].long()
        assert int(kind[hd][at[:n_ppo]].sum()) == 0 and int(kind[hd][at[n_ppo:]].sum()) == Bw
    assert agent.learner.loss_mode == "ppo"


# ----------------------------------------------------------------------------- train_vec
def run_train_vec(tmp, episodes=3, logger=None, callback=None, num_envs=1, **extra):
    from ppo_agent.train import train_vec
    from tests.helpers import SyntheticEnv, topology_cfgs
    train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp), T=8, episodes=episodes)
    for k in ("port", "routes", "scenarios", "town"):
        env_cfg[k] = env_cfg[k] * num_envs
    train_cfg.update(save_interval=10 ** 6, **extra)
    os.makedirs(str(tmp), exist_ok=True)
    agent = train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, num_envs, env_cls=SyntheticEnv, logger=logger, callback=callback)
    torch.cuda.synchronize()
    return agent


def test_train_vec_with_a_sample_reuse_key(tmp_path):
    from cadre_amd.reuse import ReuseWindow
    lines, seen = [], {}
    logger = types.SimpleNamespace(log=lines.append)

    def cb(event, **st):
        # the first rollout, before any optimiser step: the record pass against the act-time behaviour log-probabilities
        if event == "rollout" and st["episode"] == 0:
            w = ReuseWindow(st["agent"], 1, len(st["rollouts"]), 8)
            w.append(st["rollouts"], st["dones"])
            w.refresh(True)
            seen["act_vs_update"] = w.stats()[:, 2].cpu().tolist()
    absent = run_train_vec(tmp_path / "a")
    none = run_train_vec(tmp_path / "b", sample_reuse=None)
    assert torch.equal(absent.arena.params, none.arena.params) and absent.arena.step == none.arena.step == 6
    agent = run_train_vec(tmp_path / "c", logger=logger, callback=cb, log_stats=True, sample_reuse={"rollouts": 2})
    print("act-time against update-time kernels, no optimiser step between: max |log ratio| (steer, throttle) %s" % seen["act_vs_update"])
    assert all(np.isfinite(v) for v in seen["act_vs_update"])
    assert agent.arena.step == 6 and agent.learner.loss_mode == "ppo"
    assert not torch.equal(agent.arena.params, absent.arena.params) and bool(torch.isfinite(agent.arena.params).all())
    stat_lines = [s for s in lines if "approx kl" in s]
    assert len(stat_lines) == 3 and stat_lines[0].endswith("reuse: 0 rollouts")
    assert "reuse: 1 rollouts, ratio: " in stat_lines[1] and "reuse: 2 rollouts, ratio: " in stat_lines[2]
    assert "effective samples: " in stat_lines[2] and "max |log ratio|: " in stat_lines[2]
    with pytest.raises(ValueError, match="checkpoint"):
        run_train_vec(tmp_path / "d", sample_reuse={"rollouts": 2}, checkpoint_interval=2)
    with pytest.raises(ValueError, match="sample_reuse"):
        run_train_vec(tmp_path / "e", sample_reuse={"rollouts": 0})
