"""GPU: frame-table storages.  The feature only changes where a window row is read from, so every comparison is on integer
views of the bits: the `_ft` gathers against the entry points they twin, scan + copy against tests/frame_table_ref.py, and
DemoSet / the mixed PPO step / the PPG buffer in frame-table form against their materialised form."""
import functools

import numpy as np
import pytest
import torch

from tests import frame_table_ref as ref
from tests.test_imitation_gpu import make_agent, random_demo, record_episodes

pytestmark = pytest.mark.gpu
S, D, LD = 8, 530, 544                  # window, feature columns, the storage pitch (= DP, the workspace pitch)
T, BW, NW, C = 12, 5, 2, 4              # rows per storage, minibatch rows per worker, workers, commands
BT = NW * BW
SENT = -3.25                            # what no launch wrote keeps this


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- 1. the gather twins through the C ABI
@functools.lru_cache(maxsize=None)
def sources():
    """Two workers' content, each stored materialised AND as frames (pad columns hold garbage in both: no kernel may carry it
    over), shared by the steer and throttle source of the worker; per source its own hn / cn / scalars.  The window ids hold
    id 0, id F - 1, a window of one frame eight times and two transitions that share seven frames."""
    g = torch.Generator().manual_seed(5)
    out = []
    for wi in range(NW):
        F = 23 + wi
        frames = torch.randn(F, LD, generator=g)
        win = torch.randint(0, F, (T + 1, S), generator=g, dtype=torch.int32)
        win[0, 0], win[1, 3] = 0, F - 1
        win[2, :] = 7                                                   # one frame eight times
        win[5, :7] = win[4, 1:]                                         # row 5 is row 4 slid by one
        obs = frames[win.long()]                                        # [T + 1][S][LD]
        w = dict(frames=frames.cuda(), win=win.cuda(), obs=obs.contiguous().cuda(), F=F, heads=[])
        for K in (33, 3):
            w["heads"].append(dict(hn=torch.randn(T + 1, LD, generator=g).cuda(), cn=torch.randn(T + 1, LD, generator=g).cuda(),
                                   action=torch.randint(0, K, (T + 1, 1), generator=g).cuda(),
                                   value_preds=torch.randn(T + 1, 1, generator=g).cuda(), returns=torch.randn(T + 1, 1, generator=g).cuda(),
                                   logp=torch.randn(T + 1, 1, generator=g).cuda(),
                                   command=torch.randint(0, C, (T + 1, 1), generator=g, dtype=torch.int32).cuda(),
                                   adv=torch.randn(T, 1, generator=g).cuda()))
        out.append(w)
    idx = torch.stack([torch.randperm(T, generator=g)[:BW] for _ in range(2 * NW)]).contiguous()
    idx[0, 0], idx[1, 1], idx[2, 2], idx[0, 3], idx[0, 4] = 0, 1, 2, 4, 5   # the marked rows are gathered
    return out, idx.cuda()


NINE = ("hn", "cn", "action", "value_preds", "returns", "logp", "command", "adv")


def table(srcs, framed):
    """The pointer table: nine words per source for the existing entry points (framed None), eleven for the twins, where
    framed[worker] says whether that worker rides as a frame table."""
    rows = []
    for wi, w in enumerate(srcs):
        for h in w["heads"]:
            nine = [(w["frames"] if framed and framed[wi] else w["obs"]).data_ptr()] + [h[k].data_ptr() for k in NINE]
            if framed is not None:
                nine += [w["win"].data_ptr(), w["F"]] if framed[wi] else [0, 0]
            rows.append(nine)
    return torch.tensor(rows, dtype=torch.int64).cuda()


def new_out():
    z = lambda *s, dtype=torch.float32: torch.full(s, SENT, device="cuda").to(dtype)
    return dict(X=z(2, S, BT, LD), h0=z(2, BT, LD), c0=z(2, BT, LD), actions=z(2, BT, dtype=torch.int64),
                commands=z(2, BT, dtype=torch.int32), old_values=z(2, BT), returns=z(2, BT), old_logp=z(2, BT), adv=z(2, BT),
                pos=z(2, BT, dtype=torch.int32), seg=z(2, C, 2, dtype=torch.int32))


SCALARS = ("actions", "commands", "old_values", "returns", "old_logp", "adv")


def run_multi(name, tab, idx, srt):
    from cadre_amd import hip
    o = new_out()
    p = lambda k: o[k].data_ptr()
    args = [tab.data_ptr(), 2 * NW, LD, S, LD, idx.data_ptr(), BW, D, D, BT] + ([C] if srt else []) + \
           [p("X"), o["X"].stride(0), LD, p("h0"), p("c0"), o["h0"].stride(0), LD] + [p(k) for k in SCALARS] + \
           ([p("pos"), p("seg")] if srt else []) + [hip.stream()]
    hip.check(getattr(hip.lib(), name)(*args), name)
    return o


def run_single(srcs, idx, framed):
    """Every source through the single-storage entry point, at its own row offset of the packed batch."""
    from cadre_amd import hip
    o = new_out()
    for zi in range(2 * NW):
        wi, hd = zi >> 1, zi & 1
        w, h = srcs[wi], srcs[wi]["heads"][hd]
        rest = [LD, S] + [h[k].data_ptr() for k in ("hn", "cn")] + [LD] + [h[k].data_ptr() for k in NINE[2:]] + \
               [idx[zi].data_ptr(), BW, D, D, BT, wi * BW, o["X"][hd].data_ptr(), LD, o["h0"][hd].data_ptr(), o["c0"][hd].data_ptr(), LD] + \
               [o[k][hd].data_ptr() for k in SCALARS] + [hip.stream()]
        if framed is None:
            hip.check(hip.lib().cadre_gather_minibatch(w["obs"].data_ptr(), *rest), "cadre_gather_minibatch")
        elif framed[wi]:
            hip.check(hip.lib().cadre_gather_minibatch_ft(w["frames"].data_ptr(), w["win"].data_ptr(), w["F"], *rest),
                      "cadre_gather_minibatch_ft")
        else:
            hip.check(hip.lib().cadre_gather_minibatch_ft(w["obs"].data_ptr(), None, 0, *rest), "cadre_gather_minibatch_ft")
    return o


def assert_same_outputs(got, want):
    for k in want:
        assert same(got[k], want[k]), k
    assert float(want["X"][:, :, :, D:].abs().max()) == 0.0              # the pad is zero, whatever the sources' pads held


@pytest.mark.parametrize("framed", [(True, True), (False, True), (False, False)],
                         ids=["frames", "worker0-materialised", "both-materialised"])
def test_gather_twins_equal_the_existing_entry_points(framed):
    """X with its zero pad, h0 / c0, every scalar array, pos and seg: the sorted, the unsorted and the single-storage form,
    from frame tables, from one materialised and one frame-table worker in ONE launch, and from win == NULL everywhere."""
    srcs, idx = sources()
    old_t, new_t = table(srcs, None), table(srcs, framed)
    assert old_t.shape == (2 * NW, 9) and new_t.shape == (2 * NW, 11)
    for srt in (True, False):
        base = "cadre_gather_sorted_multi" if srt else "cadre_gather_minibatch_multi"
        want, got = run_multi(base, old_t, idx, srt), run_multi(base + "_ft", new_t, idx, srt)
        assert_same_outputs(got, want)
        assert float(want["X"].abs().max()) > 0 and (not srt or int(want["seg"][:, :, 1].sum()) == 2 * BT)
    assert_same_outputs(run_single(srcs, idx, framed), run_single(srcs, idx, None))


def test_gather_obs_twin_and_the_scalar_fallback():
    from cadre_amd import hip
    srcs, idx = sources()
    L = hip.lib()
    w = srcs[0]
    want, got, nul = (torch.full((S * BW, LD), SENT, device="cuda") for _ in range(3))
    hip.check(L.cadre_gather_obs(w["obs"].data_ptr(), LD, S, idx[0].data_ptr(), BW, want.data_ptr(), LD, D, hip.stream()), "o")
    hip.check(L.cadre_gather_obs_ft(w["frames"].data_ptr(), w["win"].data_ptr(), w["F"], LD, S, idx[0].data_ptr(), BW,
                                    got.data_ptr(), LD, D, hip.stream()), "ft")
    hip.check(L.cadre_gather_obs_ft(w["obs"].data_ptr(), None, 0, LD, S, idx[0].data_ptr(), BW, nul.data_ptr(), LD, D,
                                    hip.stream()), "ft")
    assert same(got, want) and same(nul, want) and float(want[:, D:].abs().max()) == 0.0
    # pitches that are no multiple of 4 floats: S = 3, D = 37, ldo = 37, ldx = 39 (the element-wise path)
    g = torch.Generator().manual_seed(9)
    s, d, ldo, ldx, F, B = 3, 37, 37, 39, 11, 4
    frames = torch.randn(F, ldo, generator=g)
    win = torch.randint(0, F, (7, s), generator=g, dtype=torch.int32)
    win[0, 0], win[1, 1] = 0, F - 1
    obs = frames[win.long()].contiguous().cuda()
    ix = torch.tensor([0, 1, 5, 3]).cuda()
    want, got = (torch.full((s * B, ldx), SENT, device="cuda") for _ in range(2))
    hip.check(L.cadre_gather_obs(obs.data_ptr(), ldo, s, ix.data_ptr(), B, want.data_ptr(), ldx, d, hip.stream()), "o")
    fr, wn = frames.cuda(), win.cuda()
    hip.check(L.cadre_gather_obs_ft(fr.data_ptr(), wn.data_ptr(), F, ldo, s, ix.data_ptr(), B, got.data_ptr(), ldx, d,
                                    hip.stream()), "ft")
    assert same(got, want) and float(got[:, d:].abs().max()) == 0.0 and float(got[:, :d].abs().max()) > 0
    # 16-byte friendly pitches from a base that is 4 bytes off a 16-byte boundary: the element-wise path again
    wide = torch.zeros(F * 40 + 1, device="cuda")
    off = wide[1:].view(F, 40)
    off[:, :d] = fr
    got2 = torch.full((s * B, 40), SENT, device="cuda")
    hip.check(L.cadre_gather_obs_ft(off.data_ptr(), wn.data_ptr(), F, 40, s, ix.data_ptr(), B, got2.data_ptr(), 40, d,
                                    hip.stream()), "ft")
    assert off.data_ptr() % 16 == 4 and same(got2[:, :d], want[:, :d]) and float(got2[:, d:].abs().max()) == 0.0


def test_ids_outside_the_table_give_nan_rows_and_touch_nothing_else():
    srcs, idx = sources()
    good = run_multi("cadre_gather_minibatch_multi_ft", table(srcs, (True, True)), idx, False)
    bad = [dict(w) for w in srcs]
    hit = []                                                             # (worker, minibatch row b, s) per head
    for wi, (s_, val) in enumerate(((2, -1), (6, None))):
        win = srcs[wi]["win"].clone()
        t = int(idx[2 * wi, 1])                                          # a row of the steer source's minibatch
        win[t, s_] = srcs[wi]["F"] if val is None else val
        bad[wi]["win"] = win
        hit.append((wi, t, s_))
    got = run_multi("cadre_gather_minibatch_multi_ft", table(bad, (True, True)), idx, False)
    keep = torch.ones(2, S, BT, dtype=torch.bool, device="cuda")
    n_hit = 0
    for wi, t, s_ in hit:
        for hd in range(2):
            for b in torch.nonzero(idx[2 * wi + hd] == t).view(-1).tolist():
                row = got["X"][hd, s_, wi * BW + b]
                assert bool(torch.isnan(row[:D]).all()) and float(row[D:].abs().max()) == 0.0
                keep[hd, s_, wi * BW + b] = False
                n_hit += 1
    assert n_hit >= 2 and same(got["X"][keep], good["X"][keep])
    for k in ("h0", "c0") + SCALARS:
        assert same(got[k], good[k]), k


# ----------------------------------------------------------------------------- 2. scan + copy against the reference
def scan_case(P, s, d, ld_src, seed):
    """Three storages: slides on rows 1-3, a reset fill at row 4, slides on rows 5-6, row 7 all new, row 8 the slide of row 7
    but for column d - 1 of one frame; the third storage's pad columns hold garbage."""
    out = []
    for z in range(3):
        rng = np.random.RandomState(seed + z)
        obs = ref.sliding_obs(P, s, d, ld_src, rng, resets=(4,), pad_garbage=(z == 2))
        obs[7, :, :d] = rng.standard_normal((s, d)).astype(np.float32)
        obs[8, :s - 1, :d] = obs[7, 1:, :d]
        obs[8, s - 1, :d] = rng.standard_normal(d).astype(np.float32)
        obs[8, 1, d - 1] = np.float32(obs[8, 1, d - 1] + 1.0)
        out.append(obs)
    return out


@pytest.mark.parametrize("s,d,ld_src,ld", [(8, 530, 544, 544), (3, 37, 37, 64)], ids=["storage-pitch", "odd-pitch"])
def test_scan_and_copy_match_the_reference(s, d, ld_src, ld):
    from cadre_amd import frames as fr
    from cadre_amd.frames import FrameStorage
    P, n = 9, 3
    host = scan_case(P, s, d, ld_src, seed=30)
    dev = [torch.from_numpy(np.concatenate([o, np.full((1, s, ld_src), 5.0, np.float32)])).cuda() for o in host]   # [P + 1] rows
    scan = fr.scan_frames(dev, P, s, ld_src, d)
    _tab, flags, win_local, count = scan
    want = [ref.scan(o, d) for o in host]
    assert np.array_equal(flags.cpu().numpy(), np.stack([w[0] for w in want]))
    assert np.array_equal(win_local.cpu().numpy(), np.stack([w[1] for w in want]))
    counts = [w[2] for w in want]
    assert count.cpu().tolist() == counts
    if s == 8:      # row 0: 1; rows 1-3: 3; the reset: 1; rows 5-6: 2; row 7: 8; row 8: the new frame and the one that differs
        assert counts == [17, 17, 17]
    total = sum(counts)
    base = [0, counts[0], counts[0] + counts[1]]
    row0 = [0, P, 2 * P]
    frames = torch.full((total + 3, ld), SENT, device="cuda")
    win = torch.full((n * P + 1, s), -7, dtype=torch.int32, device="cuda")
    fr.copy_frames(scan, P, s, ld_src, d, base, frames, win, row0)
    want_frames = np.concatenate([ref.pack(o, d, ld)[0] for o in host])
    assert np.array_equal(frames[:total].cpu().numpy().view(np.uint32), want_frames.view(np.uint32))      # zero pad included
    assert float((frames[total:] - SENT).abs().max()) == 0.0             # rows past the frames in use are untouched
    want_win = np.concatenate([w[1] + b for w, b in zip(want, base)])
    assert np.array_equal(win[:n * P].cpu().numpy(), want_win) and int(win[n * P].max()) == -7
    # the round trip: the windows materialised again are the source rows
    st = FrameStorage(n * P, 1, d, s, d, True, 0.99, 1.0, device="cuda:0", frames=frames, win=win, n_frames=total)
    assert st._ldo == ld
    src = torch.cat([o[:P, :, :d] for o in dev])
    back = st.obs
    assert back.shape == (n * P + 1, s, d) and same(back[:n * P], src)
    assert bool(torch.isnan(back[n * P]).all())                          # ids -7: a row nobody built
    # FrameStorage.gather is the generator's gather
    ix = torch.tensor([3, 0, 26, 13])
    x = st.gather(ix, torch.zeros(n * P, 1, device="cuda"))[0]
    assert same(x, src[ix.cuda()].permute(1, 0, 2).reshape(-1, d))


# ----------------------------------------------------------------------------- helpers: a DemoSet in frame-table form
def to_frames(demo):
    """The frame-table form of a materialised DemoSet, through scan + copy (random rows: every window row is a frame)."""
    from cadre_amd import frames as fr
    from ppo_agent.imitation import DemoSet
    s0, T_ = demo.steer, demo.T
    scan = fr.scan_frames([s0._obs], T_, s0.seq_length, s0._ldo, s0.z_dims)
    n = int(scan[3].item())
    steer, throttle = fr.frame_pair(T_, s0.z_dims, s0.seq_length, s0.hid_size, demo.gamma, s0.device, frame_capacity=n)
    fr.copy_frames(scan, T_, s0.seq_length, s0._ldo, s0.z_dims, [0], steer._frames, steer._win, [0])
    steer.n_frames = throttle.n_frames = n
    for src, dst in ((demo.steer, steer), (demo.throttle, throttle)):
        for k in ("command", "action", "rewards", "masks", "returns", "_hn", "_cn"):
            getattr(dst, k).copy_(getattr(src, k))
    out = DemoSet(steer, throttle, demo.weights, demo.episodes, demo.commands, demo.gamma, demo.balance, demo.return_scale)
    assert out.frame_table and same(steer.obs[:T_], s0.obs[:T_])
    return out


def count_calls(monkeypatch, names):
    """Call counters on the library's entry points `names` (the Python side of the launch)."""
    from cadre_amd import hip
    L, n = hip.lib(), {k: 0 for k in names}
    for k in names:
        fn = getattr(L, k)

        def counted(*a, _fn=fn, _k=k):
            n[_k] += 1
            return _fn(*a)
        monkeypatch.setattr(L, k, counted)
    return n


# ----------------------------------------------------------------------------- 3. DemoSet.from_episodes(frame_table=True)
def test_demo_set_from_episodes_as_frames(tmp_path):
    from cadre_amd import replay
    from ppo_agent.imitation import DemoSet, evaluate, pretrain
    a_mat, a_ft = make_agent(tmp_path), make_agent(tmp_path)
    paths = record_episodes(tmp_path / "demos", lengths=(6, 6))
    n_frames = sum(int(replay.load_episode(p)["rgb"].shape[0]) for p in paths)
    mat = DemoSet.from_episodes(a_mat, paths, gamma=0.99)
    ft = DemoSet.from_episodes(a_ft, paths, gamma=0.99, frame_table=True)
    assert ft.frame_table and not mat.frame_table and ft.T == mat.T == 12
    assert ft.steer._obs is None and ft.steer._frames.shape == (n_frames, ft.steer._ldo) and ft.steer.n_frames == n_frames
    assert ft.throttle._frames is ft.steer._frames and ft.throttle._win is ft.steer._win
    assert n_frames < 12 * 8                                             # fewer frame rows than window rows
    assert same(ft.steer.obs[:12], mat.steer.obs[:12]) and float(ft.steer._frames[:, 530:].abs().max()) == 0.0
    for k in ("command", "action", "returns", "masks"):
        assert same(getattr(ft.steer, k), getattr(mat.steer, k)) and same(getattr(ft.throttle, k), getattr(mat.throttle, k))
    assert evaluate(a_ft, ft, 4) == evaluate(a_mat, mat, 4)
    assert a_ft._gather_entry.endswith("_ft") and not a_mat._gather_entry.endswith("_ft")
    recs = []
    for agent, demo in ((a_mat, mat), (a_ft, ft)):
        torch.manual_seed(77)
        recs.append(pretrain(agent, demo, None, epochs=1, minibatch=4, lr=1e-3, max_grad_norm=250.0, reset_optimizer=False))
    assert recs[0] == recs[1] and recs[0][0]["steps"] == 3
    for k in ("params", "grads", "exp_avg", "exp_avg_sq"):
        assert same(getattr(a_ft.arena, k), getattr(a_mat.arena, k)), k
    tr_f, va_f = ft.split(0.5, seed=0)
    tr_m, va_m = mat.split(0.5, seed=0)
    assert tr_f.steer._frames.data_ptr() == va_f.steer._frames.data_ptr() == ft.steer._frames.data_ptr()
    assert tr_f.frame_table and tr_f.steer._obs is None and tr_f.T == tr_m.T == 6
    for f_, m_ in ((tr_f, tr_m), (va_f, va_m)):
        assert same(f_.steer.obs[:6], m_.steer.obs[:6]) and same(f_.throttle.returns, m_.throttle.returns)
        assert same(f_.weights, m_.weights) and f_.episodes == m_.episodes
    with pytest.raises(ValueError, match="frame_table must be a bool"):
        DemoSet.from_episodes(a_ft, paths, gamma=0.99, frame_table=1)


# ----------------------------------------------------------------------------- 4. the mixed PPO step
@pytest.mark.parametrize("sort", [True, False], ids=["sorted", "unsorted"])
def test_mixed_ppo_step_from_a_frame_table_set(tmp_path, sort):
    """update_policy_from_storages(live materialised storages, demo=DemoMixer(frame-table set)) against the materialised set:
    the live workers ride with win == NULL beside the frame-table entries in one launch.  Two steps with the optimiser step
    between them: losses, demo losses and the arena bit for bit."""
    from ppo_agent.imitation import DemoMixer
    from tests.test_demo_mix_gpu import ppo_storages
    Bw = 32
    runs = []
    for framed in (False, True):
        agent = make_agent(tmp_path)
        lrn = agent.learner
        lrn.use_sorted = sort
        agent.gather_sorted = True if sort else None
        assert lrn.sorted_rows(2 * Bw) == sort
        (ps, pt), (adv_s, adv_t) = ppo_storages(40, seed=21)
        demo, _host = random_demo(agent, 48, seed=22)
        if framed:
            demo = to_frames(demo)
        mixer = DemoMixer(demo, blocks=1, seed=3)
        r = np.random.RandomState(6)
        out = []
        for step in range(2):
            idx_s, idx_t = (torch.from_numpy(r.permutation(40)[:Bw].astype(np.int64)) for _ in range(2))
            got = agent.update_policy_from_storages([(ps, idx_s, adv_s, pt, idx_t, adv_t)], demo=mixer.entries(Bw, 0, step),
                                                    demo_label_smoothing=0.1, demo_coeff=0.7, demo_value_coeff=0.3)
            out.append((got, lrn.workspace(2 * Bw)["demo_losses"].clone(), agent.arena.grads.clone()))
            lrn.clip_adam(lr=1e-3, max_grad_norm=250.0)
        want_entry = ("cadre_gather_sorted_multi" if sort else "cadre_gather_minibatch_multi") + ("_ft" if framed else "")
        assert agent._gather_entry == want_entry
        assert any(k and k[0] == "ft" for k in agent._gather_tables) == framed
        runs.append((out, agent.arena.params.clone(), agent.arena.exp_avg.clone()))
    (o_m, p_m, m_m), (o_f, p_f, m_f) = runs
    for (l_m, d_m, g_m), (l_f, d_f, g_f) in zip(o_m, o_f):
        assert l_m == l_f and same(d_m, d_f) and same(g_m, g_f)
    assert same(p_m, p_f) and same(m_m, m_f) and float(o_m[0][1].abs().max()) > 0


# ----------------------------------------------------------------------------- 5. the PPG buffer
def sliding_rollouts(seed, n_envs=2, T_=8):
    """(steer, throttle) RolloutStorage pairs whose windows slide (one reset inside), random states, commands and returns."""
    from ppo_agent.storage import RolloutStorage
    out = []
    for e in range(n_envs):
        rng = np.random.RandomState(seed + e)
        obs = torch.from_numpy(ref.sliding_obs(T_ + 1, S, D, LD, rng, resets=(5,))).cuda()
        pair = []
        for hd in range(2):
            st = RolloutStorage(T_, 1, D, S, D, True, 0.99, 0.95, device="cuda:0")
            st._obs.copy_(obs)
            st.hn.copy_(torch.from_numpy((rng.standard_normal((T_ + 1, D)) * 0.1).astype(np.float32)))
            st.cn.copy_(torch.from_numpy((rng.standard_normal((T_ + 1, D)) * 0.1).astype(np.float32)))
            st.command[:, 0].copy_(torch.from_numpy(rng.randint(0, 4, T_ + 1).astype(np.int32)))
            st.returns[:, 0].copy_(torch.from_numpy(rng.standard_normal(T_ + 1).astype(np.float32)))
            pair.append(st)
        pair[1].command.copy_(pair[0].command)
        out.append(tuple(pair))
    return out


def test_aux_buffer_as_frames(tmp_path):
    from cadre_amd.phasic import AuxBuffer, aux_phase
    from ppo_agent.models import Shared_grad_buffers
    sections = [sliding_rollouts(50), sliding_rollouts(60)]
    runs = []
    for fpr in (None, 1.25):
        agent = make_agent(tmp_path)
        buf = AuxBuffer(agent, 2, 16, frames_per_row=fpr)
        for sec in sections:
            buf.append(sec)
        if fpr is not None:
            # per storage of 8 rows: the filled first row 1, six slides 6, one reset 1 = 8 frames (+ S - 1 = 7 window rows saved each)
            assert buf.steer._obs is None and buf.steer._frames.shape[0] == 40 and buf.frames_used == buf.steer.n_frames == 32
            assert buf.throttle.n_frames == 32 and int(buf.steer._win[:32].min()) == 0 and int(buf.steer._win[:32].max()) == 31
            want = torch.cat([s._obs[:8] for sec in sections for s, _t in sec])
            assert same(buf.steer.obs[:32], want[:, :, :D])
        sgb = Shared_grad_buffers(agent.model_dict, agent.device)
        rec = aux_phase(agent, buf, epochs=1, minibatch=8, shared_grad_buffers=sgb, optimizer=None, max_grad_norm=250.0, lr=1e-3,
                        seed=5, rank=0, episode=1)
        assert agent._gather_entry.endswith("_ft") == (fpr is not None)
        runs.append((rec, agent.arena.params.clone(), agent.arena.grads.clone(), buf.table.clone()))
        if fpr is not None:
            buf.clear()
            assert buf.frames_used == 0 and buf.steer.n_frames == 0 and buf.filled == 0
    assert runs[0][0] == runs[1][0] and runs[0][0][0]["steps"] == 4
    for a_, b_ in zip(runs[0][1:], runs[1][1:]):
        assert same(a_, b_)
    # too small: the first section (16 frames) fits 24, the second finds 8 left; nothing of the buffer is written
    small = AuxBuffer(agent, 2, 16, frames_per_row=0.75)
    small.append(sections[0])
    state = (small.steer._win.clone(), small.steer._frames.clone(), small.steer.returns.clone(), small.steer._hn.clone())
    with pytest.raises(ValueError, match="needs 16 frames, 8 of the buffer's 24"):
        small.append(sections[1])
    assert small.filled == 1 and small.frames_used == 16 and small.steer.n_frames == 16
    for a_, b_ in zip(state, (small.steer._win, small.steer._frames, small.steer.returns, small.steer._hn)):
        assert same(a_, b_)


# ----------------------------------------------------------------------------- 6. the untouched path
def test_without_a_frame_storage_the_existing_entry_points_run(tmp_path, monkeypatch):
    names = ["cadre_gather_sorted_multi", "cadre_gather_minibatch_multi", "cadre_gather_minibatch"]
    n = count_calls(monkeypatch, names + [k + "_ft" for k in names])
    agent = make_agent(tmp_path)
    demo, _host = random_demo(agent, 72, seed=8)
    agent.learner.use_sorted = True
    agent.imitate_from_storages(demo.batch(torch.arange(64)))                # B = 64: the sorted one-launch gather
    agent.imitate_from_storages(demo.batch(torch.arange(24)))                # B = 24: the unsorted one
    assert n["cadre_gather_sorted_multi"] == 1 and n["cadre_gather_minibatch_multi"] == 1
    assert not any(n[k + "_ft"] for k in names)
    keys = list(agent._gather_tables)
    assert keys and all(len(k) == 2 * 9 and k[0] != "ft" for k in keys)      # nine words per source, as always
    framed = to_frames(demo)
    agent.imitate_from_storages(framed.batch(torch.arange(64)))
    agent.imitate_from_storages(framed.batch(torch.arange(24)))
    assert n["cadre_gather_sorted_multi_ft"] == 1 and n["cadre_gather_minibatch_multi_ft"] == 1
    assert n["cadre_gather_sorted_multi"] == 1 and n["cadre_gather_minibatch_multi"] == 1
    new = [k for k in agent._gather_tables if k not in keys]
    assert new and all(k[0] == "ft" and len(k) == 1 + 2 * 11 for k in new)
    assert framed.steer._win.data_ptr() in new[0] and framed.steer._frames.data_ptr() in new[0]


# ----------------------------------------------------------------------------- 7. the config keys through train_vec
def test_train_vec_with_the_frame_keys_is_bit_identical(tmp_path):
    """train_cfg.pretrain / demo_mix with frame_table and train_cfg.aux_phase with frames_per_row (8: whatever the synthetic
    env's windows repeat, S frames per row always fit) against the same run with the keys absent."""
    import os
    from tests.test_phasic_gpu import run_train_vec
    paths = record_episodes(tmp_path / "demos", lengths=(6, 6))
    recs = os.path.dirname(paths[0])

    def cfg(framed):
        ft = dict(frame_table=True) if framed else {}
        return dict(pretrain=dict(episodes=recs, epochs=1, minibatch=4, lr=1e-3, **ft),
                    demo_mix=dict(episodes=recs, coeff=0.5, **ft),
                    aux_phase=dict(interval=2, minibatch=8, epochs=1, **(dict(frames_per_row=8) if framed else {})))
    plain = run_train_vec(tmp_path / "a", episodes=2, **cfg(False))
    framed = run_train_vec(tmp_path / "b", episodes=2, **cfg(True))
    assert plain.arena.step == framed.arena.step and plain.arena.step > 0
    assert same(plain.arena.params, framed.arena.params) and same(plain.arena.exp_avg, framed.arena.exp_avg)
    assert list(framed._demo_sets.values())[0].frame_table and not list(plain._demo_sets.values())[0].frame_table
    assert framed._gather_entry.endswith("_ft") and not plain._gather_entry.endswith("_ft")
