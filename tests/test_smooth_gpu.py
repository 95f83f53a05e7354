"""GPU: the temporal smoothness term (csrc/smooth.hip, cadre_amd/smooth.py).

  1  every mate -1 and every row of kind 0: cadre_ppo_smooth_loss is cadre_ppo_loss_ord bit for bit
  2  layouts "prefix" and "random": unpaired rows are the PPO kernel's, the bit-equal pair stores d == 0, invalid successor rows zeros, the
     two d of a pair exact negatives, equal inputs equal bits
  3  every stored element against float64 at the running bound of tests/loss_parity.py (tests/smooth_parity.py); every mutant rejected
  4  the KL gate, the PPO diagnostics and the adaptive lr do not see the pairs
  5  cadre_smooth_mates against its numpy statement
  6  cadre_action_jitter against numpy float64
  7  one mixed step through update_policy_from_storages(smooth=) against float64 autograd
  8  device-hyper mode: field 15 moves the step without a new graph
  9  coeff = 0 with the key present leaves the parameters of a run without the key
 10  train_vec / train with the key
 11  a checkpointed run with the key continues with the bits of the uninterrupted one"""
import os
import types

import numpy as np
import pytest
import torch

from tests import demo_mix_ref
from tests import smooth_parity as sp
from tests import smooth_ref as ref
from tests.loss_parity import F4, SENT, XVE
from tests.test_loss_parity_gpu import DECOY, F_PPO, Launch, dev, host

pytestmark = pytest.mark.gpu
FS = 4
IDS = [sp.case_id(kw) for kw in sp.SMOOTH_CASES]


@pytest.fixture(scope="module")
def hip():
    from cadre_amd import hip as h
    h.lib()
    return h


class SmoothLaunch(Launch):
    def __init__(self, hip, c):
        Launch.__init__(self, hip, c)
        self.ctrl = dev(c.ctrl)
        self.kind, self.mate = dev(c.kindrow), dev(c.mate)

    def outputs(self):
        o = Launch.outputs(self)
        c = self.c
        o.update(smooth_losses=torch.full((8,), float(SENT), device="cuda"), smooth_d=torch.full((2, c.B), float(SENT), device="cuda"),
                 smooth_stats=torch.zeros(2, FS, device="cuda"), smooth_scratch=torch.full((2 * self.nblk * FS,), 3.0, device="cuda"),
                 stop=torch.zeros(1, dtype=torch.int32, device="cuda"))
        return o

    def smooth_block(self, **over):
        block = self.block().clone()
        block[self.hip.HP_SMOOTH_COEFF] = float(self.c.hp["smooth_coeff"])
        for k, v in over.items():
            block[self.hip.HP[k]] = v
        return block

    def smooth(self, o, use_hp, stats, kind=None, mate=None, target_kl=0.0, block=None):
        c, L, hp = self.c, self.hip.lib(), self.c.hp
        byval = [float(hp[k]) for k in ("clip", "value_coeff", "clip_coeff", "ent_coeff")]
        block = self.smooth_block() if block is None else block
        kind, mate = self.kind if kind is None else kind, self.mate if mate is None else mate
        rc = L.cadre_ppo_smooth_loss(*self.head(), kind.data_ptr(), mate.data_ptr(), self.ctrl.data_ptr(), c.B, c.C, c.Ks[0], c.Ks[1],
                                     block.data_ptr() if use_hp else None, *([DECOY] * 4 if use_hp else byval), float(hp["inv_b"]),
                                     DECOY if use_hp else float(hp["smooth_coeff"]), float(hp["scale_steer"]), float(hp["scale_throttle"]),
                                     float(hp["inv_bp"]), o["losses"].data_ptr(), o["smooth_losses"].data_ptr(), o["smooth_d"].data_ptr(),
                                     o["dl"].data_ptr(), o["dv"].data_ptr(), o["scratch"].data_ptr(), o["smooth_scratch"].data_ptr(), None,
                                     o["stats"].data_ptr() if stats else None, F_PPO, o["sscratch"].data_ptr() if stats else None, target_kl,
                                     o["stop"].data_ptr() if (stats and target_kl > 0) else None,
                                     o["smooth_stats"].data_ptr() if stats else None, FS,
                                     self.ord.data_ptr() if any(c.ordinal) else None, self.hip.stream())
        self.hip.check(rc, "cadre_ppo_smooth_loss")
        got = self.collect(o, stats)
        assert bool((o["smooth_losses"][1:] == float(SENT)).all()), "a smoothness loss beyond its slot was written"
        got.update(smooth_losses=host(o["smooth_losses"])[:1], smooth_d=host(o["smooth_d"]), stop=int(o["stop"]))
        if stats:
            got["smooth_stats"] = host(o["smooth_stats"])
        return got

    def ppo_ord(self, o, use_hp, stats, target_kl=0.0, block=None, cmds=None):
        """cadre_ppo_loss_ord on the case's operands (an all-categorical case passes the marker table)."""
        c, L, hp = self.c, self.hip.lib(), self.c.hp
        byval = [float(hp[k]) for k in ("clip", "value_coeff", "clip_coeff", "ent_coeff")]
        block = self.smooth_block() if block is None else block
        head = self.head()
        if cmds is not None:
            head[7] = cmds.data_ptr()
        table = self.ord if any(c.ordinal) else self.marker
        rc = L.cadre_ppo_loss_ord(*head, c.B, c.C, c.Ks[0], c.Ks[1], block.data_ptr() if use_hp else None,
                                  *([DECOY] * 4 if use_hp else byval), float(hp["inv_b"]), o["losses"].data_ptr(), o["dl"].data_ptr(),
                                  o["dv"].data_ptr(), o["scratch"].data_ptr(), None, o["stats"].data_ptr() if stats else None,
                                  F_PPO if stats else 0, o["sscratch"].data_ptr() if stats else None, target_kl,
                                  o["stop"].data_ptr() if (stats and target_kl > 0) else None, table.data_ptr(), self.hip.stream())
        self.hip.check(rc, "cadre_ppo_loss_ord")
        got = self.collect(o, stats)
        got["stop"] = int(o["stop"])
        return got


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F4)).view(np.uint32)


# ----------------------------------------------------------------------------- 1. no pairs: the PPO kernel
@pytest.mark.parametrize("i", [0, 2, 4, 7], ids=[IDS[i] for i in (0, 2, 4, 7)])
def test_no_pairs_is_the_ppo_kernel(hip, i):
    """Every mate -1 and every row of kind 0: losses, dlogits, dvalues and the stats row carry the bits of cadre_ppo_loss_ord, in the four
    variants (stats x hp); smooth_losses and smooth_d are zeros."""
    c = sp.smooth_case(sp.SMOOTH_CASES[i])
    run = SmoothLaunch(hip, c)
    kind = torch.zeros(2, c.B, dtype=torch.int32, device="cuda")
    mate = torch.full((2, c.B), -1, dtype=torch.int32, device="cuda")
    for use_hp in (False, True):
        for stats in (False, True):
            got = run.smooth(run.outputs(), use_hp, stats, kind, mate)
            want = run.ppo_ord(run.outputs(), use_hp, stats)
            for k in ("losses", "dlogits", "dvalues") + (("stats",) if stats else ()):
                assert np.array_equal(bits(got[k]), bits(want[k])), (k, use_hp, stats)
            assert float(np.abs(got["smooth_losses"]).max()) == 0.0 and float(np.abs(got["smooth_d"]).max()) == 0.0
            if stats:
                assert float(np.abs(got["smooth_stats"]).max()) == 0.0


# ----------------------------------------------------------------------------- 2. the pairs, two layouts
@pytest.mark.parametrize("layout", ["prefix", "random"])
@pytest.mark.parametrize("i", [0, 1, 2, 5, 6], ids=[IDS[i] for i in (0, 1, 2, 5, 6)])
def test_pairs_in_two_layouts(hip, i, layout):
    c = sp.smooth_case(sp.SMOOTH_CASES[i], layout)
    run = SmoothLaunch(hip, c)
    o = run.outputs()
    got = run.smooth(o, False, True)
    ppo = run.ppo_ord(run.outputs(), False, False)
    C, ldl = c.C, c.ldl
    gl, pl = got["dlogits"], ppo["dlogits"]
    allnets = lambda buf, h, b: np.stack([buf[(h * C + cc) * c.l_ns + b * ldl: (h * C + cc) * c.l_ns + (b + 1) * ldl] for cc in range(C)])
    vals = lambda buf, h, b: np.array([buf[(h * C + cc) * c.v_ns + b * c.ldv] for cc in range(C)])
    n_pairs = 0
    for h in range(2):
        paired0, paired1 = sp.paired_rows(c, h, False), sp.paired_rows(c, h, True)
        n_pairs += paired0.size
        for b in range(c.B):
            if c.kindrow[h, b] == 0 and b not in paired0:
                # rows without a partner are cadre_ppo_loss_ord bit for bit
                assert np.array_equal(bits(allnets(gl, h, b)), bits(allnets(pl, h, b))), (h, b)
                assert np.array_equal(bits(vals(got["dvalues"], h, b)), bits(vals(ppo["dvalues"], h, b))) and got["smooth_d"][h, b] == 0
            if c.kindrow[h, b] == 1 and b not in paired1:
                # invalid successor rows store zeros
                assert not allnets(gl, h, b).any() and not vals(got["dvalues"], h, b).any() and got["smooth_d"][h, b] == 0, (h, b)
            if c.kindrow[h, b] == 1:
                assert not vals(got["dvalues"], h, b).any()
            elif b in paired0:                         # the critic does not see the pair
                assert np.array_equal(bits(vals(got["dvalues"], h, b)), bits(vals(ppo["dvalues"], h, b)))
        # the bit-equal pair: d == 0, the PPO gradient on the kind-0 partner, zeros on the successor
        b = c.plant[h]["equal"]
        m = c.mate[h, b]
        assert m >= 0 and got["smooth_d"][h, b] == 0 and got["smooth_d"][h, m] == 0
        assert np.array_equal(allnets(gl, h, b), allnets(pl, h, b)) and not allnets(gl, h, m).any()
        # exact negatives
        j = c.mate[h, paired0]
        assert np.array_equal(got["smooth_d"][h, paired0], -got["smooth_d"][h, j])
        assert np.array_equal(bits(np.abs(got["smooth_d"][h, paired0])), bits(np.abs(got["smooth_d"][h, j])))
        assert np.abs(got["smooth_d"][h, paired0]).max() > 0
        assert got["smooth_stats"][h, 0] == paired0.size
        # paired successor rows carry a gradient (a saturated ordinal row, every threshold unit at 0 or 1, has none to give)
        far = [b2 for b2 in paired1 if abs(got["smooth_d"][h, b2]) > 1e-3]
        assert far and any(np.abs(sp.head_grad(c, gl, h, np.array([b2]))).max() > 0 for b2 in far)
    assert n_pairs >= 6 and got["smooth_losses"][0] > 0
    first = {k: np.array(got[k]) for k in ("losses", "smooth_losses", "smooth_d", "dlogits", "dvalues", "stats", "smooth_stats")}
    for _ in range(2):                                 # partials combine in workgroup order: equal inputs give equal bits
        again = run.smooth(o, False, True)
        assert all(np.array_equal(bits(again[k]), bits(first[k])) for k in first)


# ----------------------------------------------------------------------------- 3. every stored element against float64
WORST = {}


@pytest.mark.parametrize("i", range(len(sp.SMOOTH_CASES)), ids=IDS)
def test_every_stored_element_against_float64(hip, i):
    """dlogits, dvalues, smooth_d, the PPO and smoothness losses and both statistics rows within the running first-order bound (T_EXP,
    T_LOG of tests/loss_parity.py; no other tolerance) — by value and with the block, with and without statistics, the kinds and partners
    from cadre_smooth_mates on the case's storages.  Every mutant of the pair statements is rejected by the same check."""
    c = sp.smooth_case(sp.SMOOTH_CASES[i])
    run = SmoothLaunch(hip, c)
    kind, mate = mates_launch(hip, c.src, c.idx, c.nW, c.E, c.Bw, c.T, c.C, c.rotation, c.pos, c.B)
    assert np.array_equal(kind, c.kindrow) and np.array_equal(mate, c.mate)
    want = sp.run_smooth(c, XVE)
    worst = 0.0
    for use_hp, stats in ((False, False), (False, True), (True, False), (True, True)):
        got = run.smooth(run.outputs(), use_hp, stats, dev(kind), dev(mate))
        w, n_amb = sp.check_smooth(c, got, want, "cadre_ppo_smooth_loss hp %s stats %d %s" % ("block" if use_hp else "NULL", stats, c.tag()),
                                   stats=stats)
        worst = max(worst, w)
        assert n_amb <= 1
    WORST[i] = worst
    print("worst err / bound over the cases so far: %.3f" % max(WORST.values()))
    for m in ref.MUTANTS:
        if m == "mate_wrong_net" and c.C == 1:
            continue
        with pytest.raises(AssertionError):
            sp.check_smooth(c, sp.emulate_smooth(c, mut={m}), want, m, quiet=True)


# ----------------------------------------------------------------------------- 4. the gate does not see the pairs
@pytest.mark.parametrize("i", [0, 4], ids=[IDS[0], IDS[4]])
def test_kl_gate_diagnostics_and_adaptive_lr_do_not_see_the_pairs(hip, i):
    """Against cadre_ppo_loss_ord on the same kind-0 rows (the successor rows' commands out of range there): losses, the stats row, the
    stop flag and the block after the KL-adaptive rule are equal bit for bit, with a gate that fires and one that does not; old_logp /
    old_values / adv / returns of the successor rows are not read (NaN there changes nothing)."""
    c = sp.smooth_case(sp.SMOOTH_CASES[i])
    run = SmoothLaunch(hip, c)
    cmds_ppo = dev(np.where(c.kindrow == 1, -1, c.cmds).astype(np.int32))
    nan = lambda a: dev(np.where(c.kindrow == 1, np.nan, a).astype(F4))
    for tkl in (1e-6, 1e3):
        blocks = [run.smooth_block(desired_kl=1e-5, lr_min=1e-5, lr_max=1e-2, lr_factor=1.5) for _ in range(3)]
        got = run.smooth(run.outputs(), True, True, target_kl=tkl, block=blocks[0])
        want = run.ppo_ord(run.outputs(), True, True, target_kl=tkl, block=blocks[1], cmds=cmds_ppo)
        assert np.array_equal(bits(got["losses"]), bits(want["losses"])) and got["stop"] == want["stop"] == (1 if tkl < 1 else 0)
        assert np.array_equal(bits(got["stats"][:, :7]), bits(want["stats"][:, :7]))
        assert torch.equal(blocks[0], blocks[1]) and (float(blocks[0][hip.HP["lr"]]) == 3e-4) == (tkl < 1)
        assert got["smooth_losses"][0] > 0
        saved = {k: run.d[k] for k in ("old_v", "rets", "old_lp", "adv")}
        try:
            for k in saved:
                run.d[k] = nan(getattr(c, k))
            poisoned = run.smooth(run.outputs(), True, True, target_kl=tkl, block=blocks[2])
        finally:
            run.d.update(saved)
        for k in ("losses", "smooth_losses", "smooth_d", "dlogits", "dvalues", "stats", "smooth_stats"):
            assert np.array_equal(bits(poisoned[k]), bits(got[k])), k


def test_refusals_come_before_any_launch(hip):
    c = sp.smooth_case(sp.SMOOTH_CASES[0])
    run = SmoothLaunch(hip, c)
    o = run.outputs()
    for patch, why in ((dict(scale_steer=F4(-1.0)), "scale"), (dict(inv_bp=F4(0.0)), "inv_bp"), (dict(smooth_coeff=F4(np.inf)), "finite")):
        old = {k: c.hp[k] for k in patch}
        c.hp.update(patch)
        try:
            with pytest.raises(hip.CadreHipError, match=why):
                run.smooth(o, False, False)
        finally:
            c.hp.update(old)
    assert bool((o["dl"] == float(SENT)).all())
    L = hip.lib()
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    for args in ((1, 2, 4, 9, 2, 0, None, 12), (2, 1, 4, 9, 2, -1, None, 12), (2, 1, 4, 9, 2, 0, None, 13), (2, 1, 4, 1, 2, 0, None, 12)):
        assert L.cadre_smooth_mates(t.data_ptr(), t.data_ptr(), *args, t.data_ptr(), t.data_ptr(), hip.stream()) != 0
    assert L.cadre_action_jitter(t.data_ptr(), 0, 9, 2, 33, 3, t.data_ptr(), t.data_ptr(), hip.stream()) != 0


# ----------------------------------------------------------------------------- 5. cadre_smooth_mates
def mates_launch(hip, src, idx, nW, E, Bw, T, C, rotation, pos, B):
    keep = []
    rows = []
    for masks, tl, cmd in src:
        t = [dev(masks.copy()), None if tl is None else dev(tl.copy()), dev(cmd.copy())]
        keep.append(t)
        rows.append([t[0].data_ptr(), 0 if t[1] is None else t[1].data_ptr(), t[2].data_ptr()])
    table, idx_d = dev(np.array(rows, np.int64)), dev(idx)
    kind = torch.full((2, B), 9, dtype=torch.int32, device="cuda")
    mate = torch.full((2, B), 9, dtype=torch.int32, device="cuda")
    pos_d = None if pos is None else dev(pos)
    hip.check(hip.lib().cadre_smooth_mates(table.data_ptr(), idx_d.data_ptr(), nW, E, Bw, T, C, rotation,
                                           None if pos_d is None else pos_d.data_ptr(), B, kind.data_ptr(), mate.data_ptr(), hip.stream()),
              "cadre_smooth_mates")
    return host(kind), host(mate)


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("shape", sp.SHAPES, ids=lambda s: "Bw%d-nW%d-E%d" % s)
def test_mates_against_the_numpy_statement(hip, shape, with_pos):
    """Random storages (ends, time limits with and without the pointer, command runs, commands out of range) and random index vectors with
    the host's successor rule, one of them broken (an index that is not t + 1), at two step numbers."""
    Bw, nW, E = shape
    B, C, T = (nW + E) * Bw, 3, Bw + 7
    for step in (0, 5):
        r = np.random.RandomState(17 * Bw + step + with_pos)
        src = []
        for k in range(2 * nW):
            masks = (r.random_sample(T + 1) > 0.15).astype(F4)
            tl = (r.random_sample(T + 1) < 0.1).astype(F4) if k % 3 else None
            cmd = np.repeat(r.randint(-1, C + 1, T + 1), 3)[:T + 1].astype(np.int32)
            src.append((masks, tl, cmd))
        idx = np.zeros((2 * (nW + E), Bw), np.int64)
        for k in range(2 * nW):
            idx[k] = r.permutation(T)[:Bw]
            idx[k, 0] = T - 1
        rot = step * E
        for k in range(E):
            for h in range(2):
                idx[2 * (nW + k) + h] = np.minimum(idx[2 * ((rot + k) % nW) + h] + 1, T - 1)
        idx[2 * nW, 1] += 1                                                   # not the successor of its worker row
        pos = np.stack([r.permutation(B) for _ in range(2)]).astype(np.int32) if with_pos else None
        want = ref.smooth_mates(src, idx, nW, E, Bw, T, C, rot, pos, B)
        got = mates_launch(hip, src, idx, nW, E, Bw, T, C, rot, pos, B)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        n_valid = int((want[1] >= 0).sum()) // 2
        assert 0 < n_valid < 2 * E * Bw


# ----------------------------------------------------------------------------- 6. cadre_action_jitter
@pytest.mark.parametrize("with_tl", [False, True])
@pytest.mark.parametrize("T", [2, 65, 300])
def test_jitter_against_numpy_float64(hip, T, with_tl):
    """Count and max exact; the sum within 1e-12 relative: the terms are exact fp32 differences widened to double, and reordering <= 3000
    doubles moves the sum by less than 3000 * 2^-53 relative."""
    n, C, Ks = 6, 3, (33, 3)
    r = np.random.RandomState(T + with_tl)
    ctrl = sp.ctrl_table(Ks)
    keep, rows, want = [], [], []
    for k in range(n):
        K = Ks[k & 1]
        a = r.randint(0, K, T + 1).astype(np.int64)
        if T > 2:
            a[r.randint(T)] = K
            a[r.randint(T)] = -1
        masks = (r.random_sample(T + 1) > 0.1).astype(F4)
        tl = (r.random_sample(T + 1) < 0.1).astype(F4) if with_tl else None
        cmd = np.repeat(r.randint(0, C + 1, T + 1), 5)[:T + 1].astype(np.int32)
        if T == 2:
            masks[:], cmd[:] = 1, 1
            if tl is not None:
                tl[:] = 0
        t = [dev(a), dev(masks), None if tl is None else dev(tl), dev(cmd)]
        keep.append(t)
        rows.append([0 if x is None else x.data_ptr() for x in t])
        want.append(ref.action_jitter(a, masks, tl, cmd, T, C, K, ctrl[k & 1]))
    out = torch.full((n, 3), -1.0, dtype=torch.float64, device="cuda")
    table, ctrl_d = dev(np.array(rows, np.int64)), dev(ctrl)          # (named: both must outlive the launch)
    hip.check(hip.lib().cadre_action_jitter(table.data_ptr(), n, T, C, Ks[0], Ks[1], ctrl_d.data_ptr(), out.data_ptr(), hip.stream()),
              "cadre_action_jitter")
    got, want = host(out), np.array(want)
    worst = float(np.max(np.abs(got[:, 1] - want[:, 1]) / np.maximum(want[:, 1], 1e-300)))
    print("jitter T %d: worst relative error of the sum %.2e" % (T, worst))
    assert np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 2], want[:, 2]) and worst <= 1e-12
    assert want[:, 0].sum() > 0


# ----------------------------------------------------------------------------- 7 .. 9. through the agent
T_E, MBN, N_ENV = 16, 2, 2
BW = T_E // MBN
COEFF, HEAD_SCALE = 0.8, (1.0, 0.5)


def e2e_cfg(**kw):
    d = dict(use_adv_norm=True, ppo_epoch=1, max_grad_norm=250.0, lr=3e-4)
    d.update(kw)
    return d


def section_rollouts(section):
    """Synthetic storages with the cursor at T: an end and a command change inside the rollout of every storage, a time limit in one."""
    from tests.test_ppo_stats_gpu import storages
    out = []
    for w in range(N_ENV):
        pair = storages(T_E, MBN, 900 + 10 * section + w)
        for h, s in enumerate(pair):
            s.masks.fill_(1.0)
            s.masks[5 + w + h] = 0.0
            s.command.copy_(torch.tensor([((t + h) // 7 + w) % 4 for t in range(T_E + 1)], dtype=torch.int32).view(-1, 1))
            if w == 1:
                s.time_limits[11] = 1.0
                s._tl_used = True
            s.step = T_E
        out.append(pair)
    return out


def make(tmp):
    from ppo_agent.models import Shared_grad_buffers
    from tests.test_imitation_gpu import make_agent
    agent = make_agent(tmp)
    return agent, Shared_grad_buffers(agent.model_dict, agent.device)


def test_step_gradient_against_autograd(tmp_path, hip):
    """One mixed step with E = 1 < nW = 2 at step number 1 (worker 1 is paired, worker 0 is not): the gradient of all 16 nets within 2e-4
    of its model's max |g| of float64 autograd of the PPO loss on the workers' rows + coeff * head_scale * mean over the pair slots of d^2
    (the bar of the same test of the self-imitation step); pairs and kinds are the numpy statement's, the term is the stated one."""
    from cadre_amd import synth
    from cadre_amd.smooth import Smoothness
    from oracle import ppo_ref
    agent, _shared = make(tmp_path)
    lrn, C = agent.learner, 4
    sm = Smoothness(agent, COEFF, entries=1, head_scale=HEAD_SCALE)
    lrn.set_loss("ppo+smooth", smooth_coeff=COEFF)
    lrn.set_loss("ppo")
    live = section_rollouts(1)
    advs = []
    for pair in live:
        for s in pair:
            s.returns.copy_(s.value_preds + 0.5 * torch.randn(s.returns.shape, generator=torch.Generator().manual_seed(3)).cuda())
            advs.append(torch.randn(T_E, 1, generator=torch.Generator().manual_seed(len(advs))).cuda())
    r = np.random.RandomState(4)
    idx = [torch.from_numpy(r.permutation(T_E)[:BW].astype(np.int64)) for _ in range(2 * N_ENV)]
    batches = [(live[w][0], idx[2 * w], advs[2 * w], live[w][1], idx[2 * w + 1], advs[2 * w + 1]) for w in range(N_ENV)]
    sm.begin_section(live, 1)
    sm.step_no = 1
    entries, rotation = sm.step(batches)
    assert rotation == 1 and len(entries) == 1 and entries[0][0] is live[1][0] and not entries[0][1].is_cuda
    assert entries[0][1].tolist() == [min(t + 1, T_E - 1) for t in idx[2].tolist()]
    srow = sm.next_stats_row()
    agent.update_policy_from_storages(batches, smooth=(entries, rotation), smooth_stats_row=srow)
    E = 1
    B_ppo, B = N_ENV * BW, (N_ENV + E) * BW
    assert lrn.loss_mode == "ppo" and lrn._smooth_rows is None
    w = lrn.workspace(B)
    srt = lrn.sorted_rows(B)
    pos = host(w["pos"]) if srt else None
    f1 = lambda t: host(t).reshape(-1)
    src = [(f1(s.masks), f1(s.time_limits) if s._tl_used else None, f1(s.command)) for pair in live for s in pair]
    idx_all = np.stack([x.numpy() for x in idx] + [entries[0][1].numpy(), entries[0][4].numpy()])
    kind_w, mate_w = ref.smooth_mates(src, idx_all, N_ENV, E, BW, T_E, C, rotation, pos, B)
    assert np.array_equal(host(w["row_kind"]), kind_w) and np.array_equal(host(w["mate"]), mate_w)
    kind_u, mate_u = ref.smooth_mates(src, idx_all, N_ENV, E, BW, T_E, C, rotation, None, B)
    n_valid = [(mate_u[h, :B_ppo] >= 0).sum() for h in range(2)]
    print("sorted rows %s; valid pairs %s of %d slots" % (srt, n_valid, BW))
    assert min(n_valid) >= 2 and max(n_valid) < BW and (mate_u[:, :BW] == -1).all()
    # float64 autograd on the unsorted layout
    params = {m: {k: p.double().requires_grad_(True) for k, p in d.items()} for m, d in ppo_ref.to_torch_params(synth.ppo_state(11)).items()}
    f2 = lambda t: host(t).reshape(t.shape[0], -1)
    cols = {k: np.zeros((2, B), np.float64) for k in ("act", "cmd", "ov", "ret", "olp", "adv")}
    xs, h0s, c0s = [], [], []
    for hd in range(2):
        xo, hh, cc_ = [], [], []
        srcs = [(live[wk][hd], idx[2 * wk + hd].numpy(), advs[2 * wk + hd]) for wk in range(N_ENV)]
        srcs.append((live[1][hd], entries[0][1 + 3 * hd].numpy(), advs[2 + hd]))
        for k_, (s, t, adv) in enumerate(srcs):
            sl = slice(k_ * BW, (k_ + 1) * BW)
            for k, src_ in (("act", s.action), ("cmd", s.command), ("ov", s.value_preds), ("ret", s.returns), ("olp", s.action_log_probs),
                            ("adv", adv)):
                cols[k][hd, sl] = f2(src_)[t, 0]
            xo.append(host(s._obs)[t][:, :, :530]); hh.append(host(s._hn)[t][:, :530]); cc_.append(host(s._cn)[t][:, :530])
        xs.append(np.concatenate(xo)); h0s.append(np.concatenate(hh)); c0s.append(np.concatenate(cc_))
    lg_rows, v_rows = [], []
    for hd, (head, K) in enumerate((("steer", 33), ("throttle", 3))):
        x = torch.from_numpy(xs[hd]).double().permute(1, 0, 2).reshape(-1, 530)        # time-major [S * B, 530]
        hid = (torch.from_numpy(h0s[hd]).double(), torch.from_numpy(c0s[hd]).double())
        for c in range(C):
            hh_, _ = ppo_ref.lstm_forward(x, hid, params["%s_lstm_%d" % (head, c)])
            lg_rows.append(torch.nn.functional.pad(ppo_ref.mlp3(hh_, params["%s_ppo_%d" % (head, c)], "control.linear"), (0, 64 - K)))
            v_rows.append(ppo_ref.mlp3(hh_, params["%s_ppo_%d" % (head, c)], "critic").view(-1))
    tt = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    lgs, vs = torch.stack(lg_rows), torch.stack(v_rows)
    cmd = tt(cols["cmd"], torch.int64)
    ppo = demo_mix_ref.ppo_rows_loss(lgs, vs, tt(cols["act"], torch.int64), cmd, tt(cols["ov"], torch.float64), tt(cols["ret"], torch.float64),
                                     tt(cols["olp"], torch.float64), tt(cols["adv"], torch.float64), torch.from_numpy(kind_u), (33, 3),
                                     (None, None), C, lrn.clip, lrn.vc, lrn.cc, lrn.ec, 1.0 / BW)
    total, want_term = ppo[3], 0.0
    ctrl = sm.ctrl.double().cpu()
    for hd, K in enumerate((33, 3)):
        i = torch.from_numpy(np.flatnonzero(mate_u[hd, :B_ppo] >= 0))
        j = torch.from_numpy(mate_u[hd, :B_ppo][i.numpy()].astype(np.int64))
        term = ref.smooth_loss_torch(lgs[hd * C + cmd[hd, i], i, :K], lgs[hd * C + cmd[hd, j], j, :K], ctrl[hd, :K],
                                     COEFF * HEAD_SCALE[hd] / (E * BW))
        total = total + term
        want_term += float(term.detach())
    total.backward()
    worst = 0.0
    for mn, dct in params.items():
        gv = agent.arena.views(agent.arena.grads, mn)
        scale = max(float(p.grad.abs().max()) for p in dct.values() if p.grad is not None)
        if scale == 0.0:                               # a command net without a row in this step: exact zeros
            assert all(float(gv[k].abs().max()) == 0.0 for k in dct), mn
            continue
        for k, p in dct.items():
            g64 = torch.zeros_like(p) if p.grad is None else p.grad
            err = float((gv[k].cpu().double() - g64).abs().max()) / scale
            worst = max(worst, err)
            assert err < 2e-4, (mn, k, err)
    got_term = float(w["smooth_losses"][0])
    print("mixed step with successor rows: worst per-parameter error (rel. to model max |g|) %.2e; smoothness term %.6e (float64 %.6e)"
          % (worst, got_term, want_term))
    assert want_term > 1e-5 and abs(got_term - want_term) < 1e-5 * max(1.0, want_term)
    assert [float(srow[h, 0]) for h in range(2)] == [float(n) for n in n_valid]
    s = sm.summary()
    assert s["pairs"] == tuple(float(n) for n in n_valid) and min(s["max_abs_d"]) > 0 and min(s["jitter"]["pairs"]) > 0
    # what is refused
    with pytest.raises(ValueError, match="successor entry"):
        agent.update_policy_from_storages(batches, smooth=(entries, 0))
    with pytest.raises(ValueError, match="rotation"):
        agent.update_policy_from_storages(batches, smooth=(entries * 3, 0))
    live[0][0].step = 3
    with pytest.raises(ValueError, match="cursor"):
        sm.begin_section(live, 0)
    assert lrn.loss_mode == "ppo"


def test_device_hyper_mode_follows_the_block_without_a_new_graph(tmp_path):
    """After set_hyper(smooth_coeff = 2 x) the replayed graph writes exactly twice the successor rows' dlogits and the smoothness term
    (a power of two), the critic gradients stay, and no graph is added."""
    from cadre_amd.smooth import Smoothness
    agent, _shared = make(tmp_path)
    lrn = agent.learner
    sm = Smoothness(agent, 0.5, head_scale=HEAD_SCALE)
    live = section_rollouts(1)
    idx = torch.arange(T_E)                              # B = 64: the rows are sorted by command, the pairs go through `pos`
    batches = [(s, idx, s.advantages, t, idx, t.advantages) for s, t in live]
    lrn.set_device_hyper(True)
    lrn.set_hyper(smooth_coeff=0.5)
    sm.begin_section(live, 0)
    step = sm.step(batches)
    for _ in range(3):
        agent.update_policy_from_storages(batches, smooth=step)
    B_ppo, B = N_ENV * T_E, 2 * N_ENV * T_E
    w = lrn.workspace(B)
    assert lrn.sorted_rows(B)
    f1 = lambda t: host(t).reshape(-1)
    src = [(f1(s.masks), f1(s.time_limits) if s._tl_used else None, f1(s.command)) for pair in live for s in pair]
    idx_all = np.stack([idx.numpy()] * (2 * N_ENV) + [e[k].numpy() for e in step[0] for k in (1, 4)])
    kind_w, mate_w = ref.smooth_mates(src, idx_all, N_ENV, N_ENV, T_E, T_E, agent.arena.C, step[1], host(w["pos"]), B)
    assert np.array_equal(host(w["row_kind"]), kind_w) and np.array_equal(host(w["mate"]), mate_w) and (mate_w >= 0).sum() >= 16
    n_graphs = len(lrn._graphs)
    assert any(k[0] == "all" and any(isinstance(x, tuple) and x[:2] == ("smooth", B_ppo) for x in k) and ("hp",) in k
               for k in lrn._graphs if k[0] != "warm")
    before, sl_before, kind = w["dO3"].clone(), w["smooth_losses"].clone(), w["row_kind"].clone()
    lrn.set_hyper(smooth_coeff=1.0)
    agent.update_policy_from_storages(batches, smooth=step)
    assert len(lrn._graphs) == n_graphs and lrn.hyper("smooth_coeff") == 1.0
    assert float(lrn._hp[15]) == 1.0
    after, C = w["dO3"], agent.arena.C
    for hd in range(2):
        succ = torch.nonzero(kind[hd] != 0).view(-1)
        own = torch.nonzero(kind[hd] == 0).view(-1)
        act_b, act_a = before[2 * hd * C:2 * (hd + 1) * C:2], after[2 * hd * C:2 * (hd + 1) * C:2]
        crit_b, crit_a = before[2 * hd * C + 1:2 * (hd + 1) * C:2], after[2 * hd * C + 1:2 * (hd + 1) * C:2]
        assert succ.numel() == B_ppo and torch.equal(act_a[:, succ], 2.0 * act_b[:, succ]) and float(act_b[:, succ].abs().max()) > 0
        assert torch.equal(crit_a, crit_b) and not torch.equal(act_a[:, own], act_b[:, own])
    assert float(w["smooth_losses"][0]) == 2.0 * float(sl_before[0]) > 0
    assert lrn.loss_mode == "ppo"


def run_sections(tmp, coeff, sections=2):
    """coeff None: no term; else a Smoothness with that coefficient.  Per section (losses, parameters, generator state, stats)."""
    from cadre_amd.smooth import Smoothness
    from ppo_agent.train import learner_section_multi
    agent, shared = make(tmp)
    sm = None
    if coeff is not None:
        sm = Smoothness(agent, coeff, head_scale=HEAD_SCALE)
        agent.learner.set_loss("ppo+smooth", smooth_coeff=coeff)
        agent.learner.set_loss("ppo")
    torch.manual_seed(77)
    out = []
    for e in range(sections):
        rollouts, dones = section_rollouts(e), [False, e == 1]
        st = {}
        losses = learner_section_multi(agent, rollouts, dones, e2e_cfg(), shared, stats=st, episode=e,
                                       **({} if sm is None else dict(smooth=sm)))
        out.append((losses, agent.arena.params.clone(), torch.get_rng_state().clone(), st))
    torch.cuda.synchronize()
    return agent, out


def test_zero_coefficient_leaves_the_run_without_the_key(tmp_path):
    """coeff = 0 with the term present: the parameters after every section are array_equal to a run without it on the same seeds (the
    successor rows' gradients are exact zeros, the PPO rows' bits do not depend on their neighbours).  The generator streams are the same —
    the term draws nothing — so the comparison is on the parameters themselves, not on the PPO rows' gradients.  With coeff > 0 the
    parameters move and the section's stats carry pairs, mean |d|, max |d| and the realised jitter."""
    agent, zero = run_sections(tmp_path / "a", 0.0)
    _a, plain = run_sections(tmp_path / "b", None)
    for e in range(2):
        assert torch.equal(zero[e][2], plain[e][2]) and zero[e][0] == plain[e][0], e
        assert torch.equal(zero[e][1], plain[e][1]), e
        assert "smooth" in zero[e][3] and "smooth" not in plain[e][3]
    assert agent.learner.loss_mode == "ppo"
    _b, on = run_sections(tmp_path / "c", COEFF, sections=1)
    s = on[0][3]["smooth"]
    print("section stats with the term: %s" % (s,))
    assert not torch.equal(on[0][1], plain[0][1]) and bool(torch.isfinite(on[0][1]).all())
    assert s["steps"] == MBN and min(s["pairs"]) > 0 and min(s["mean_abs_d"]) > 0 and all(m >= a for m, a in zip(s["max_abs_d"], s["mean_abs_d"]))
    assert min(s["jitter"]["pairs"]) > 0 and min(s["jitter"]["mean"]) > 0
    from ppo_agent.train import stats_line
    assert "smooth: pairs" in stats_line(0, on[0][3])


# ----------------------------------------------------------------------------- 10. train_vec / train with the key
def test_train_vec_and_train_with_the_key(tmp_path):
    """Two episodes of train_vec (the sizes of test_train_vec_with_a_self_imitation_key) and of train() with one environment: the run
    goes through, the loss mode is "ppo" again, the log line carries pairs, mean |d|, max |d| and the realised jitter, the coefficient
    schedule is in block field 15; the key absent and the key None are the same run; what is refused at start-up raises."""
    from cadre_amd import hip as h
    from cadre_amd.ppo_agent import train as T_
    from ppo_agent import train as train_mod
    from tests.helpers import SyntheticEnv, topology_cfgs

    def run(tag, **extra):
        lines = []
        train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path / tag), T=8, episodes=2)
        train_cfg.update(save_interval=10 ** 6, **extra)
        os.makedirs(str(tmp_path / tag), exist_ok=True)
        agent = train_mod.train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, 1, env_cls=SyntheticEnv,
                                    logger=types.SimpleNamespace(log=lines.append))
        torch.cuda.synchronize()
        return agent, lines
    absent, _l = run("a", log_stats=True)
    none, plain_lines = run("b", log_stats=True, smoothness=None)
    assert torch.equal(absent.arena.params, none.arena.params) and not none.learner.device_hyper
    agent, lines = run("c", log_stats=True, smoothness=dict(coeff=("linear", 1.0, 0.0), head_scale=(1.0, 0.5)))
    lrn = agent.learner
    stat_lines = [s for s in lines if "approx kl" in s]
    print(stat_lines[-1])
    assert len(stat_lines) == 2 and all("smooth: pairs" in s and "|d|:" in s and "max |d|:" in s and "jitter:" in s for s in stat_lines)
    assert not any("smooth:" in s for s in plain_lines)
    assert lrn.loss_mode == "ppo" and lrn.device_hyper and float(lrn._hp[h.HP_SMOOTH_COEFF]) == 0.5
    assert agent.arena.step == absent.arena.step and bool(torch.isfinite(agent.arena.params).all())
    assert not torch.equal(agent.arena.params, absent.arena.params)
    for key, why in ((dict(sample_reuse=dict(rollouts=2)), "sample_reuse"), (dict(self_imitation=dict(rollouts=2, coeff=0.1)), "one kind array"),
                     (dict(smoothness=dict(coeff=0.1, tau=1)), "unknown")):
        with pytest.raises(ValueError, match=why):
            run("d", **dict(dict(smoothness=dict(coeff=0.1)), **key))
    # train(): one environment
    made, lines1 = [], []
    Base = T_.CadreAgent

    class Agent(Base):
        def __init__(self, *a, **kw):
            Base.__init__(self, *a, **kw)
            made.append(self)
    train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path / "one"), T=8, episodes=2)
    train_cfg.update(save_interval=10 ** 6, log_stats=True, smoothness=dict(coeff=0.25))
    os.makedirs(str(tmp_path / "one"), exist_ok=True)
    orig, T_.CadreAgent = T_.CadreAgent, Agent
    try:
        T_.train(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, env_cls=SyntheticEnv, logger=types.SimpleNamespace(log=lines1.append))
    finally:
        T_.CadreAgent = orig
    torch.cuda.synchronize()
    one = [s for s in lines1 if "approx kl" in s]
    assert len(one) == 2 and all("smooth: pairs" in s and "jitter:" in s for s in one)
    assert made[-1].learner.loss_mode == "ppo" and float(made[-1].learner._hp[h.HP_SMOOTH_COEFF]) == 0.25
    assert bool(torch.isfinite(made[-1].arena.params).all())


# ----------------------------------------------------------------------------- 11. resume
def test_resume_with_the_key_is_bit_exact(tmp_path):
    """The sizes and helpers of tests/test_checkpoint_gpu.py::test_train_vec_resume_is_bit_exact, with the key: a checkpoint after every
    episode perturbs nothing, and a fresh call from another seed resumed from episode 1 continues with the bits of the straight run."""
    from ppo_agent.train import train_vec
    from tests.helpers import topology_cfgs
    from tests.test_checkpoint_gpu import _assert_episode, _record, _resume_env
    N, T, EP = 2, 8, 4
    Env = _resume_env()

    def run(sub, callback, **kw):
        (tmp_path / sub).mkdir()
        train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path / sub), H=84, W=84, T=T, episodes=EP)
        env_cfg.update(num_processes=N, port=[2000 + i for i in range(N)], routes=["r%d" % i for i in range(N)],
                       scenarios=["s"] * N, town=["Town01"] * N)
        env_cfg.update({k: kw.pop(k) for k in ("start_step", "seed_base") if k in kw})
        train_cfg.update(save_interval=10 ** 6, reward_scaling=True, log_stats=True, ppo_epoch=1,
                         smoothness=dict(coeff=("linear", 0.6, 0.2), entries=1), **kw)
        return train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, N, env_cls=Env, callback=callback)
    straight, files, resumed = {}, {}, []

    def cb1(event, **kw):
        if event == "update":
            straight[kw["episode"]] = _record(kw["agent"], kw["rollouts"], kw["reward_scaler"], kw["losses"])
        if event == "checkpoint":
            files[kw["episode"]] = kw["path"]
    run("straight", cb1, checkpoint_interval=1)
    assert sorted(straight) == list(range(EP)) and sorted(files) == list(range(EP))
    assert all(c[0] == T for e in range(EP) for c in straight[e][1]["cursors"])          # every rollout starts at row 0

    def cb3(event, **kw):
        if event == "update":
            _assert_episode(_record(kw["agent"], kw["rollouts"], kw["reward_scaler"], kw["losses"]), straight[kw["episode"]],
                            "resumed, episode %d" % kw["episode"])
            resumed.append(kw["episode"])
    agent = run("resumed", cb3, resume_from=files[1], start_step=2 * T, seed_base=31337)
    assert resumed == [2, 3]
    assert torch.equal(torch.get_rng_state(), straight[EP - 1][1]["rng"]) and agent.arena.step == EP * 2
    assert float(agent.learner._hp[15]) == 0.6 + (0.2 - 0.6) * 3 / 4
