"""GPU: training checkpoints.  A: cadre_state_capture at the smallest shapes that can go wrong, against the numpy digest
(tests/checkpoint_ref.py); B: a capture is stream-ordered; C: a resumed train_vec continues with the bits of the straight
run; D: refusals leave the live state untouched; E: a checkpoint from before the first optimiser step."""
import numpy as np
import pytest
import torch

from tests import checkpoint_ref as ref

pytestmark = pytest.mark.gpu

WORDS = [0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 4097, 2 ** 20 + 3]
CANARY = np.uint32(0xA5C3A5C3)
GAP = 8                                   # canary words around every destination range (and junk around every source)


@pytest.fixture(scope="module")
def hip():
    from cadre_amd import hip as h
    h.lib()
    return h


def bits(t):
    return t.detach().contiguous().view(-1).view(torch.int32)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- A: the kernel
class Case(object):
    """Ranges of (words, source misalignment, staging misalignment) — bytes past a 16-byte boundary: 0, 4, 8 or 12 —
    laid out in one source buffer (junk between the ranges) and one staging buffer (canaries everywhere else)."""

    def __init__(self, hip, specs, seed):
        r = np.random.RandomState(seed)
        self.hip, self.specs = hip, specs
        so, do, self.src_at, self.dst_at = 4, 4, [], []
        for n, sm, dm in specs:
            so = (so + GAP + 3) // 4 * 4 + sm // 4
            do = (do + GAP + 3) // 4 * 4 + dm // 4
            self.src_at.append(so)
            self.dst_at.append(do)
            so, do = so + n, do + n
        self.src_h = r.randint(0, 2 ** 32, size=so + GAP, dtype=np.uint64).astype(np.uint32)
        for (n, _sm, _dm), at in zip(specs, self.src_at):
            self.src_h[at:at + n] = ref.random_words(r, n)
        self.src = torch.from_numpy(self.src_h.view(np.int32).copy()).cuda()
        self.n_dst = do + GAP
        base = self.src.data_ptr()
        assert base % 16 == 0
        self.table = hip.capture_table([(base + 4 * at if n else 0, 4 * dt, 4 * n)
                                        for (n, _s, _d), at, dt in zip(specs, self.src_at, self.dst_at)], "cuda")
        for (n, sm, dm), at, dt in zip(specs, self.src_at, self.dst_at):
            assert (4 * at) % 16 == sm and (4 * dt) % 16 == dm

    def words(self, k):
        n, at = self.specs[k][0], self.src_at[k]
        return self.src_h[at:at + n]

    def want(self):
        return [ref.digest(self.words(k)) for k in range(len(self.specs))]

    def launch(self, copy):
        """One launch; returns (digests as Python ints, staging as uint32 or None).  The digest slots start as junk (the
        entry point zeroes them) and sit between two guard slots."""
        R = len(self.specs)
        stg = torch.from_numpy(np.full(self.n_dst, CANARY, np.uint32).view(np.int32)).cuda() if copy else None
        assert stg is None or stg.data_ptr() % 16 == 0
        dig = torch.full((R + 2,), 0x1234567, dtype=torch.int64, device="cuda")
        self.hip.state_capture(self.table, R, stg, dig[1:R + 1])
        d = dig.cpu().numpy()
        assert d[0] == 0x1234567 and d[-1] == 0x1234567
        return [int(x) for x in d[1:R + 1].view(np.uint64)], None if stg is None else stg.cpu().numpy().view(np.uint32)

    def poke(self, k, j, value):
        at = self.src_at[k] + j
        self.src_h[at] = value
        self.src[at:at + 1].copy_(torch.from_numpy(self.src_h[at:at + 1].view(np.int32).copy()))

    def check(self):
        want = self.want()
        got, stg = self.launch(copy=True)
        expect = np.full(self.n_dst, CANARY, np.uint32)
        for k, ((n, _s, _d), dt) in enumerate(zip(self.specs, self.dst_at)):
            expect[dt:dt + n] = self.words(k)
        bad = np.nonzero(stg != expect)[0]
        assert bad.size == 0, (self.specs, bad[:8], self.dst_at)          # the copies, and every canary word around them
        assert got == want, (self.specs, got, want)
        only, none = self.launch(copy=False)
        assert none is None and only == want                              # digest-only mode
        again, stg2 = self.launch(copy=True)
        assert again == want and np.array_equal(stg2, expect)             # a second launch: the same bits
        for k, (n, _s, _d) in enumerate(self.specs):
            if n == 0:
                assert want[k] == 0
                continue
            for j in sorted({0, n - 1}):                                  # one bit of the first / of the last word
                old = self.src_h[self.src_at[k] + j]
                self.poke(k, j, old ^ np.uint32(1 << ((7 * k + 13 * j + 31) % 32)))
                flipped, _ = self.launch(copy=False)
                assert flipped[k] != want[k] and flipped[k] == ref.digest(self.words(k)), (self.specs, k, j)
                assert flipped[:k] == want[:k] and flipped[k + 1:] == want[k + 1:], (self.specs, k, j)
                self.poke(k, j, old)


@pytest.mark.parametrize("src_mis", [0, 4, 8, 12])
def test_capture_one_range_every_size_and_alignment(hip, src_mis):
    """Every word count with the source 16-, 4-, 8- and 12-bytes past a 16-byte boundary and the staging side likewise:
    equal misalignment takes the 16-byte stores, a difference of 8 the 8-byte ones, else 4-byte ones."""
    for dst_mis in (0, 4, 8, 12):
        for n in WORDS:
            Case(hip, [(n, src_mis, dst_mis)], seed=n + src_mis + 100 * dst_mis).check()


MULTI = [
    [(257, 4, 4), (0, 0, 0), (65, 8, 0)],
    [(1, 12, 8), (0, 4, 12), (2 ** 20 + 3, 8, 8)],
    [(4097, 0, 4), (0, 8, 8), (3, 4, 0)],
    [(0, 0, 0), (1, 4, 8), (2, 8, 4), (0, 12, 0), (3, 0, 12), (4, 4, 4), (63, 12, 12)],
    [(64, 8, 0), (65, 0, 8), (255, 4, 12), (0, 0, 4), (256, 12, 4), (257, 8, 8), (4097, 4, 0)],
    [(2 ** 20 + 3, 4, 4), (0, 8, 0), (4, 12, 12), (63, 0, 0), (0, 4, 4), (1, 8, 12), (255, 0, 8)],
]


@pytest.mark.parametrize("k", range(len(MULTI)))
def test_capture_three_and_seven_ranges(hip, k):
    """3 and 7 ranges per launch with a zero-length one in the middle, mixed sizes and alignments."""
    assert len(MULTI[k]) in (3, 7) and any(n == 0 for n, _s, _d in MULTI[k][1:-1])
    Case(hip, MULTI[k], seed=50 + k).check()


def test_malformed_record_is_marked_not_copied(hip):
    """A record the host wrapper refuses, handed to the launch anyway: nothing of it is copied, its slot holds
    CADRE_CAPTURE_BAD_RANGE, and the ranges beside it are done as usual."""
    c = Case(hip, [(65, 0, 0), (64, 4, 4), (3, 8, 8)], seed=9)
    tab = c.table.clone()
    tab[1, 2] = 6                                          # bytes no multiple of 4
    c.table = tab
    got, stg = c.launch(copy=True)
    want = c.want()
    assert got[0] == want[0] and got[2] == want[2] and got[1] == hip.CAPTURE_BAD_RANGE
    dt = c.dst_at[1]
    assert (stg[dt - GAP:dt + 64 + GAP] == CANARY).all()
    assert np.array_equal(stg[c.dst_at[0]:c.dst_at[0] + 65], c.words(0))


# ----------------------------------------------------------------------------- agents for B, D, E
def _agent(command_num=4, ppo_seed=11):
    from tests.test_act_batch_gpu import build_agent
    return build_agent(84, 84, command_num=command_num, ppo_seed=ppo_seed)


def _step(agent, smp, lr=1e-3):
    from tests.test_ppo_stats_gpu import dev
    agent.update_policy(dev(smp[0]), dev(smp[1]))
    agent.learner.clip_adam(lr=lr, max_grad_norm=250.0)


def _arena_state(agent):
    a = agent.arena
    out = dict(params=a.params.clone(), step_dev=a.step_dev.clone())
    if a.exp_avg is not None:
        out.update(exp_avg=a.exp_avg.clone(), exp_avg_sq=a.exp_avg_sq.clone())
    if agent.learner._hp is not None:
        out["hp"] = agent.learner._hp.clone()
    return out


def _file_verifies(state):
    for n, d in zip(state["names"], state["digests"].tolist()):
        assert ref.as_i64(ref.digest(state["tensors"][n].numpy())) == d, n


# ----------------------------------------------------------------------------- B: stream order
def test_capture_is_stream_ordered(tmp_path):
    """capture, then WITHOUT any sync an optimiser step that moves the parameters, then save / load: the file holds the
    state from before the step, and its digests verify."""
    from cadre_amd import checkpoint
    from tests.test_ppo_stats_gpu import samples, storages
    agent = _agent()
    agent.learner.set_device_hyper()
    pair = storages(16, 2, 21)
    smp = samples(64, 4, 1)
    for _ in range(3):                                   # (the optimiser step's graph exists: the next one is a replay)
        _step(agent, smp)
    torch.cuda.synchronize()
    before = _arena_state(agent)
    stor_before = {k: getattr(pair[1], k).clone() for k in checkpoint.STORAGE_TENSORS}
    rng = torch.get_rng_state()
    cap = checkpoint.capture(agent, [pair], None, episode=5, extra={"tag": "b"})
    agent.learner.clip_adam(lr=1e-3, max_grad_norm=250.0)               # enqueued behind the capture, nothing waited for
    assert torch.equal(torch.get_rng_state(), rng)                      # capture draws nothing
    path = cap.save(tmp_path / "ckpt_5.pt")
    state = checkpoint.load(path)
    torch.cuda.synchronize()
    assert not same(agent.arena.params, before["params"])               # the step did move them
    for k, v in before.items():
        assert same(state["tensors"][k], v.cpu()), k
    for k, v in stor_before.items():
        assert same(state["tensors"]["storage0.throttle." + k], v.cpu()), k
    _file_verifies(state)
    assert state["step"] == 3 and int(state["tensors"]["step_dev"][0]) == 3 and state["episode"] == 5
    assert state["extra"] == {"tag": "b"} and state["device_hyper"] is True and torch.equal(state["rng_state"], rng)
    assert state["layout"] == dict(D=530, C=4, n_out=[33, 3], hid=128, total=agent.arena.total, ordinal_rank=None)
    assert state["storages"][0][0]["step"] == pair[0].step and state["storages"][0][0]["num_steps"] == 16
    # a second capture reuses the one staging buffer; the first capture, already saved, can no longer be saved again
    st = agent._ckpt_stager
    ptrs = (st.staging.data_ptr(), st.host.data_ptr())
    cap2 = checkpoint.capture(agent, [pair], None)
    assert (st.staging.data_ptr(), st.host.data_ptr()) == ptrs
    from cadre_amd.hip import CadreHipError
    with pytest.raises(CadreHipError, match="reused"):
        cap.state()
    s2 = cap2.state()
    assert same(s2["tensors"]["params"], agent.arena.params.cpu()) and s2["step"] == 4


# ----------------------------------------------------------------------------- D: refusals
def test_damaged_file_is_refused_and_nothing_moves(tmp_path):
    from cadre_amd import checkpoint
    from cadre_amd.hip import CadreHipError
    from tests.test_ppo_stats_gpu import samples
    agent = _agent()
    agent.learner.set_device_hyper()
    smp = samples(64, 4, 1)
    _step(agent, smp)
    path = checkpoint.capture(agent).save(tmp_path / "c.pt")
    _step(agent, smp)                                    # the live state moves on
    state = checkpoint.load(path)
    state["tensors"]["exp_avg"][12345] += 1.0            # one element changed after saving, the digests kept
    torch.cuda.synchronize()
    live, step, rng = _arena_state(agent), agent.arena.step, torch.get_rng_state()
    with pytest.raises(CadreHipError, match="range exp_avg does not verify"):
        checkpoint.restore(agent, state)
    torch.cuda.synchronize()
    for k, v in _arena_state(agent).items():
        assert same(v, live[k]), k
    assert agent.arena.step == step == 2 and torch.equal(torch.get_rng_state(), rng)
    good = checkpoint.load(path)                         # the undamaged file goes in
    checkpoint.restore(agent, good)
    assert agent.arena.step == 1 and int(agent.arena.step_dev.item()) == 1
    assert same(agent.arena.exp_avg.cpu(), good["tensors"]["exp_avg"])


def test_layout_mismatch_and_sharded_arena_are_refused(tmp_path):
    from cadre_amd import checkpoint
    from cadre_amd.hip import CadreHipError
    from tests.test_ppo_stats_gpu import samples, dev
    small = _agent(command_num=2)
    path = checkpoint.capture(small).save(tmp_path / "c2.pt")
    agent = _agent(command_num=4)
    p0 = agent.arena.params.clone()
    with pytest.raises(ValueError, match="layout mismatch in C"):
        checkpoint.restore(agent, checkpoint.load(path))
    assert same(agent.arena.params, p0)
    # a scaler in the call that the file lacks
    from ppo_agent.storage import ReturnScaler
    with pytest.raises(ValueError, match="reward_scaler"):
        checkpoint.restore(small, checkpoint.load(path), reward_scaler=ReturnScaler(1, 0.99, device="cuda:0"))
    # the sharded optimiser
    smp = samples(64, 4, 1)
    agent.update_policy(dev(smp[0]), dev(smp[1]))
    agent.learner.clip_adam_sharded(0, agent.arena.total, lambda t: None, lr=1e-3, max_grad_norm=0.5)
    with pytest.raises(CadreHipError, match="sharded"):
        checkpoint.capture(agent)


# ----------------------------------------------------------------------------- E: early checkpoint
def test_checkpoint_before_the_first_optimiser_step(tmp_path):
    """Taken before any step (no moments in the file), restored after two steps: two steps from there equal the first
    two, bit for bit — the arena is where ensure_adam() starts."""
    from cadre_amd import checkpoint
    from tests.test_ppo_stats_gpu import samples
    agent = _agent()
    smps = [samples(64, 4, 1), samples(64, 4, 2)]
    p0 = agent.arena.params.clone()
    path = checkpoint.capture(agent).save(tmp_path / "c0.pt")
    state = checkpoint.load(path)
    assert "exp_avg" not in state["tensors"] and state["step"] == 0
    for s in smps:
        _step(agent, s)
    torch.cuda.synchronize()
    first = _arena_state(agent)
    assert not same(first["params"], p0)
    checkpoint.restore(agent, state)
    assert same(agent.arena.params, p0) and agent.arena.step == 0 and int(agent.arena.step_dev.item()) == 0
    assert not agent.arena.exp_avg.any().item() and not agent.arena.exp_avg_sq.any().item()
    for s in smps:
        _step(agent, s)
    torch.cuda.synchronize()
    for k, v in _arena_state(agent).items():
        assert same(v, first[k]), k
    assert agent.arena.step == 2


# ----------------------------------------------------------------------------- C: bit-exact resume through train_vec
def _resume_env():
    from tests.helpers import SyntheticEnv

    class ResumeEnv(SyntheticEnv):
        """SyntheticEnv that starts at env_cfg["start_step"] and seeds the generator (the agent's initialisation draws
        from it) from env_cfg["seed_base"]."""

        def __init__(self, env_cfg):
            SyntheticEnv.__init__(self, env_cfg)
            self.i = int(env_cfg.get("start_step", 0))
            torch.manual_seed(int(env_cfg.get("seed_base", 999)) + int(env_cfg["rank"]))
    return ResumeEnv


def _record(agent, rollouts, reward_scaler, losses):
    from cadre_amd import checkpoint
    a = agent.arena
    rec = dict(params=a.params.clone(), exp_avg=a.exp_avg.clone(), exp_avg_sq=a.exp_avg_sq.clone(),
               step_dev=a.step_dev.clone(), hp=agent.learner._hp.clone(), scaler=reward_scaler.state.clone())
    for e, pair in enumerate(rollouts):
        for h, s in enumerate(pair):
            for k in checkpoint.STORAGE_TENSORS:
                rec["storage%d.%d.%s" % (e, h, k)] = getattr(s, k).clone()
    host = dict(step=a.step, losses=losses, cursors=[(s.step, s._tl_used) for p in rollouts for s in p],
                rng=torch.get_rng_state().clone(), adaptive=agent.learner._adaptive, hp_on=agent.learner.device_hyper)
    return rec, host


def _assert_episode(got, want, what):
    (rec, host), (rec0, host0) = got, want
    assert sorted(rec) == sorted(rec0)
    for k in rec0:
        assert same(rec[k], rec0[k]), (what, k)
    for k in host0:
        if k == "rng":
            assert torch.equal(host[k], host0[k]), (what, k)
        else:
            assert host[k] == host0[k], (what, k, host[k], host0[k])


def test_train_vec_resume_is_bit_exact(tmp_path):
    from cadre_amd import hip as h
    from ppo_agent.train import train_vec
    from tests.helpers import topology_cfgs
    N, T, EP = 2, 8, 4
    Env = _resume_env()

    def run(sub, callback, **kw):
        (tmp_path / sub).mkdir()
        train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path / sub), H=84, W=84, T=T, episodes=EP)
        env_cfg.update(num_processes=N, port=[2000 + i for i in range(N)], routes=["r%d" % i for i in range(N)],
                       scenarios=["s"] * N, town=["Town01"] * N)
        env_cfg.update({k: kw.pop(k) for k in ("start_step", "seed_base") if k in kw})
        train_cfg.update(save_interval=10 ** 6, reward_scaling=True, log_stats=True, ppo_epoch=1,
                         adaptive_lr={"desired_kl": 1e-7, "min": 1e-6, "max": 1e-2}, **kw)
        return train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, N, env_cls=Env, callback=callback)

    # run 1: straight
    straight, start = {}, {}

    def cb1(event, agent, envs, rollouts, reward_scaler, **kw):
        if event == "start":
            start["params"] = agent.arena.params.clone()
        if event == "update":
            straight[kw["episode"]] = _record(agent, rollouts, reward_scaler, kw["losses"])
    run("straight", cb1)
    assert sorted(straight) == list(range(EP))
    lrs = [float(straight[e][0]["hp"][h.HP["lr"]].item()) for e in range(EP)]
    print("lr after each episode:", lrs)
    assert any(lr != 3e-4 for lr in lrs) and len(set(lrs)) > 1, lrs          # the controller moved the lr within the run
    assert straight[EP - 1][1]["step"] == EP * 2 and straight[0][1]["hp_on"]

    # run 2: a checkpoint after every episode perturbs nothing
    seen, files = [], {}

    def cb2(event, **kw):
        if event == "update":
            _assert_episode(_record(kw["agent"], kw["rollouts"], kw["reward_scaler"], kw["losses"]),
                            straight[kw["episode"]], "checkpointing, episode %d" % kw["episode"])
            seen.append(kw["episode"])
        if event == "checkpoint":
            files[kw["episode"]] = kw["path"]
    run("ckpt", cb2, checkpoint_interval=1)
    assert seen == list(range(EP)) and sorted(files) == list(range(EP))
    assert files[1] == str(tmp_path / "ckpt" / "checkpoints" / "ckpt_1.pt")

    # run 3: another process's worth of state — a fresh call, an agent initialised from another seed — resumed from episode 1
    resumed = []

    def cb3(event, **kw):
        if event == "start":          # after the restore: the other seed's parameters are gone
            assert not same(kw["agent"].arena.params, start["params"])
            assert same(kw["agent"].arena.params, straight[1][0]["params"])
        if event == "update":
            _assert_episode(_record(kw["agent"], kw["rollouts"], kw["reward_scaler"], kw["losses"]),
                            straight[kw["episode"]], "resumed, episode %d" % kw["episode"])
            resumed.append(kw["episode"])
    # (the seed only shows before the restore: a run from it, without resume_from, starts from other parameters)
    other = {}

    def cb_other(event, **kw):
        if event == "start":
            other["params"] = kw["agent"].arena.params.clone()
            raise StopIteration
    with pytest.raises(StopIteration):
        run("other", cb_other, seed_base=31337)
    assert not same(other["params"], start["params"])
    agent = run("resumed", cb3, resume_from=files[1], start_step=2 * T, seed_base=31337)
    assert resumed == [2, 3]
    assert torch.equal(torch.get_rng_state(), straight[EP - 1][1]["rng"])    # the final generator state
    assert agent.arena.step == EP * 2


def test_train_single_env_resume_is_bit_exact(tmp_path):
    """train() (one environment): three episodes with a checkpoint after each, against a fresh call from another seed
    resumed from the file of episode 0 with the environment started at step T: parameters, moments, step count, scaler
    block and the final generator state are equal bit for bit."""
    import os
    from cadre_amd.ppo_agent import train as T_        # (the module train() resolves CadreAgent in)
    from tests.helpers import topology_cfgs
    T, EP = 8, 3
    Env = _resume_env()
    made = []

    Base = T_.CadreAgent                                # bound now: run() points T_.CadreAgent at the subclass

    class Agent(Base):
        def __init__(self, *a, **kw):
            Base.__init__(self, *a, **kw)
            made.append(self)

    def run(sub, **kw):
        (tmp_path / sub).mkdir()
        train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path / sub), H=84, W=84, T=T, episodes=EP)
        env_cfg.update({k: kw.pop(k) for k in ("start_step", "seed_base") if k in kw})
        train_cfg.update(save_interval=10 ** 6, reward_scaling=True, ppo_epoch=1, **kw)
        orig, T_.CadreAgent = T_.CadreAgent, Agent
        try:
            T_.train(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, env_cls=Env)
        finally:
            T_.CadreAgent = orig
        agent = made[-1]
        torch.cuda.synchronize()
        a = agent.arena
        return dict(params=a.params.clone(), exp_avg=a.exp_avg.clone(), exp_avg_sq=a.exp_avg_sq.clone(),
                    step_dev=a.step_dev.clone(), scaler=agent.reward_scaler.state.clone()), a.step, torch.get_rng_state()
    full, step, rng = run("full", checkpoint_interval=1)
    files = sorted(os.listdir(str(tmp_path / "full" / "checkpoints")))
    assert files == ["ckpt_0.pt", "ckpt_1.pt", "ckpt_2.pt"] and step == 2 * EP
    res, step2, rng2 = run("res", resume_from=str(tmp_path / "full" / "checkpoints" / "ckpt_0.pt"), start_step=T,
                           seed_base=4711)
    for k, v in full.items():
        assert same(res[k], v), k
    assert step2 == step and torch.equal(rng2, rng)
