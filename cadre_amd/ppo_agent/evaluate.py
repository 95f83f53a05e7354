"""Evaluation of a snapshot ensemble (reference eval.py): N environments x M snapshots per env step.

The reference evaluates one route with `[agent.act(obs) for agent in agent_group]` + `agent.avg_action(...)`: M encoder
passes, M LSTM + head chains and 2 M `.item()` syncs per env step.  Here one `EnsembleEvaluator.act` serves N routes:

  * ONE encoder pass over the fresh frames of all N windows (the evaluator's own sliding-window ring, act_batch's logic);
  * the M agents are split, in order, into groups of at most 16 // C; a group's nets are copied into one stacked
    parameter arena with Mg * C commands (agent j's net (head, c) at slot (head, j * C + c)), so the group is ONE
    LSTM + MLP launch chain over the rows of all N environments, every agent reading the same sorted rows (`tiled_seg`);
  * `cadre_sample_rows_ens` samples (or picks greedily) for every (environment, agent, head), `cadre_ensemble_controls`
    averages the controls per environment in float64 (`avg_action`), and one copy brings the [N][3] controls to the host.

`evaluate_vec` is the host loop over N environments (`EpisodeSchedule` decides who starts which episode), `evaluate` is
eval.py:12-64 on top of it."""
import os

import numpy as np
import torch

from .. import hip
from ..arena import PPOArena
from ..learner import PPOLearnerHIP
from .agent import CadreAgent, check_act_batch, command_rows

MAX_NETS = 16          # command nets per head of one arena (create_model: command_num 1 .. 16)


# ----------------------------------------------------------------------------- host logic (no device)
def group_split(M, C):
    """Sizes of the agent groups, in agent order: as many full groups of 16 // C agents as fit, then the rest."""
    M, C = int(M), int(C)
    if M < 1 or not 1 <= C <= MAX_NETS:
        raise ValueError("group_split: %d agents, command_num %d (>= 1 agent, 1 .. %d commands)" % (M, C, MAX_NETS))
    per = MAX_NETS // C
    return [per] * (M // per) + ([M % per] if M % per else [])


def ens_net(head, j, c, Mg, C):
    """Arena net of group agent j's (head, command c) in a stacked arena of Mg agents."""
    return head * Mg * C + j * C + c


def tiled_seg(seg, C, Mg):
    """row_seg of a stacked arena: seg int32 [2 C][2] (command_rows) -> [2 Mg C][2] with
    tiled[h * Mg * C + j * C + c] = seg[h * C + c]: every agent's net of a command owns that command's run of rows."""
    seg = np.asarray(seg, dtype=np.int32).reshape(2, C, 2)
    return np.ascontiguousarray(np.tile(seg[:, None], (1, Mg, 1, 1)).reshape(2 * Mg * C, 2))


class EpisodeSchedule(object):
    """Which environment runs which episode when `num_envs` environments share a budget of `episodes` episodes: exactly
    `episodes` are started and finished.  `active` lists the running environments in index order; an environment that
    finishes an episode starts the next unstarted one, or leaves the list when none is left (the positions of those
    behind it then move)."""

    def __init__(self, num_envs, episodes):
        num_envs, episodes = int(num_envs), int(episodes)
        if num_envs < 1 or episodes < 0:
            raise ValueError("EpisodeSchedule: num_envs=%d, episodes=%d (>= 1 environment, >= 0 episodes)" % (num_envs, episodes))
        self.num_envs, self.episodes = num_envs, episodes
        self.started = self.finished = 0
        self.active, self.episode_of = [], {}
        for i in range(min(num_envs, episodes)):
            self.active.append(i)
            self.episode_of[i] = self.started
            self.started += 1

    def done(self):
        return self.finished == self.episodes

    def finish(self, env):
        """Environment `env` finished its episode -> (that episode's number, whether `env` starts another one: the
        caller then resets it)."""
        ep = self.episode_of.pop(env)               # KeyError: not running
        self.finished += 1
        if self.started < self.episodes:
            self.episode_of[env] = self.started
            self.started += 1
            return ep, True
        self.active.remove(env)
        return ep, False


def control_tables(agent, n_out):
    """(steer float64 [K_steer], throttle float64 [K_throttle][2]) of an agent's STEER_CONTROL / THROTTLE_CONTROL."""
    nS, nT = n_out
    sc, tc = agent.STEER_CONTROL, agent.THROTTLE_CONTROL
    try:
        steer = np.array([float(sc[k]) for k in range(nS)], dtype=np.float64)
        thr = np.array([[float(tc[k][0]), float(tc[k][1])] for k in range(nT)], dtype=np.float64)
    except (KeyError, IndexError, TypeError, ValueError):
        raise ValueError("EnsembleEvaluator: STEER_CONTROL / THROTTLE_CONTROL must hold a value for every bin 0 .. %d / a "
                         "(throttle, brake) pair for every bin 0 .. %d" % (nS - 1, nT - 1))
    if len(sc) != nS or len(tc) != nT:
        raise ValueError("EnsembleEvaluator: STEER_CONTROL / THROTTLE_CONTROL have %d / %d entries, num_output is %d / %d"
                         % (len(sc), len(tc), nS, nT))
    return steer, thr


def check_group(agent_group):
    """The refusals of EnsembleEvaluator, before any device work: every agent must equal the lead agent in device,
    command_num, num_output, lstm_input, ordinal_rank, the control tables and the encoder checkpoint."""
    if len(agent_group) < 1:
        raise ValueError("EnsembleEvaluator: empty agent_group")
    lead = agent_group[0]
    n_out = tuple(lead.arena.n_out)
    tabs = control_tables(lead, n_out)
    for m, a in enumerate(agent_group[1:], 1):
        for field, mine, theirs in (("device", lead.device, a.device), ("vae_device", lead.vae_device, a.vae_device),
                                    ("command_num", lead.command_num, a.command_num),
                                    ("num_output", n_out, tuple(a.arena.n_out)),
                                    ("lstm_input", lead.lstm_input, a.lstm_input),
                                    ("ordinal_rank", lead.ordinal_rank, a.ordinal_rank)):
            if mine != theirs:
                raise hip.CadreHipError("EnsembleEvaluator: agent %d differs from agent 0 in %s (%r vs %r)" % (m, field, theirs, mine))
        other = control_tables(a, n_out)
        for field, x, y in (("STEER_CONTROL", tabs[0], other[0]), ("THROTTLE_CONTROL", tabs[1], other[1])):
            if not np.array_equal(x, y):
                raise hip.CadreHipError("EnsembleEvaluator: agent %d differs from agent 0 in %s" % (m, field))
        if a.vae_model is not lead.vae_model and a.vae_model.fingerprint != lead.vae_model.fingerprint:
            raise ValueError("EnsembleEvaluator: agent %d holds different encoder weights (encoder fingerprint); the ensemble "
                             "shares one encoder pass" % m)
    return n_out, tabs


class EnsembleActBatch(list):
    """EnsembleEvaluator.act's return value: out[e] is the list of M act() tuples CadreAgent.ensemble_act returns for
    environment e; `.controls` N lists [steer, throttle, brake] of Python floats (avg_action); `.feat` [N][S][DP],
    `.action` i64 / `.logp` / `.value` f32 [N][M][2] the device buffers the tuples are views of."""


class _Group(object):
    """Mg consecutive agents of the ensemble in one stacked arena."""

    def __init__(self, agents, m0, lead):
        a0 = lead.arena
        self.agents, self.m0, self.Mg = agents, m0, len(agents)
        self.arena = PPOArena(lead.device, a0.D, {"steer": a0.n_out[0], "throttle": a0.n_out[1]},
                              command_num=self.Mg * lead.command_num, hid=a0.hid, ordinal=lead.ordinal_rank)
        self.learner = PPOLearnerHIP(self.arena, seq_length=lead.frame)
        self.arena._learner = self.learner
        self.keys = [None] * self.Mg

    def sync(self):
        """Re-copy the nets of every agent whose parameters changed since the last call (an optimiser step, an in-place
        load such as load_snapshot, a replaced buffer): a host tuple compare per agent, device-to-device copies through
        the parameter views.  (A load through the modules' own parameters — `model_dict[name].load_state_dict(...)` — moves
        only those parameters' version counters; load_snapshot therefore touches the arena's, a caller who loads by hand
        does the same with `agent.arena.params[:0].zero_()`.)"""
        dst = self.arena
        for j, ag in enumerate(self.agents):
            src = ag.arena
            key = (src.step, src.params._version, src.params.data_ptr())
            if key == self.keys[j]:
                continue
            C = src.C
            with torch.no_grad():
                for h in range(2):
                    for c in range(C):
                        g, gd = h * C + c, ens_net(h, j, c, self.Mg, C)
                        for views in (PPOArena.lstm_views, PPOArena.ppo_views):
                            sv, dv = views(src, src.params, g), views(dst, dst.params, gd)
                            for name, v in sv.items():
                                dv[name].copy_(v)
            self.keys[j] = (src.step, src.params._version, src.params.data_ptr())


class EnsembleEvaluator(object):
    """`[CadreAgent.ensemble_act(agent_group, o) for o in obs_list]` + `avg_action` per environment, in one launch chain
    per agent group.  Owns its latent ring, window caches, stacked arenas and control tables; reads the agents' parameters
    and encoder only (never their window caches, act_batch state, act() graphs, `control._last_*` or learner workspaces)."""

    def __init__(self, agent_group, max_envs=None):
        agent_group = list(agent_group)
        self.n_out, (steer, thr) = check_group(agent_group)
        self.agent_group = agent_group
        lead = self.lead = agent_group[0]
        self.M, self.C = len(agent_group), lead.command_num
        self.max_envs = int(lead.max_envs if max_envs is None else max_envs)
        if self.max_envs < 1:
            raise ValueError("EnsembleEvaluator: max_envs=%r" % (max_envs,))
        self.groups, m0 = [], 0
        for n in group_split(self.M, self.C):
            self.groups.append(_Group(agent_group[m0:m0 + n], m0, lead))
            m0 += n
        self.steer_tab = torch.from_numpy(steer).to(lead.device)
        self.throttle_tab = torch.from_numpy(thr).to(lead.device)
        self._vec = None

    @staticmethod
    def _same_window(c, td):
        return CadreAgent._window_shifted_vs(c, td)

    def act(self, obs_list, shifted=None, deterministic=False, allowed=None):
        """One env step for N <= max_envs environments.  `shifted[e]`: True — environment e's window moved by one frame
        since the last call at position e; False — it is fresh (a reset, or another environment sat at this position);
        None — compare the frames on the host (what `shifted=None` does for every environment).  Sampled mode draws from
        the global torch CPU generator in the loop's order (env 0 agent 0 steer, env 0 agent 0 throttle, env 0 agent 1
        steer, ..., then env 1), one `torch.empty(1, n_out).exponential_(1)` each; `deterministic=True` draws nothing and
        takes the first largest probability.  `allowed` (action masks) is refused.  Returns an EnsembleActBatch."""
        if allowed is not None:
            raise ValueError("ensemble evaluation takes no allowed= words: cadre_sample_rows_ens does not read action masks yet "
                             "(mask inside the environment loop of one agent with act_batch(allowed=))")
        lead = self.lead
        check_act_batch(obs_list, shifted, self.max_envs, lead.device, lead.vae_device, self.C)
        N, M, C = len(obs_list), self.M, self.C
        a, enc, dev = lead.arena, lead.vae_model, lead.device
        S, H, W = obs_list[0]["rgb"].shape[:3]
        L, stream = hip.lib(), hip.stream()
        for grp in self.groups:
            grp.sync()
        vec = self._vec
        if vec is None or vec["shape"] != (S, H, W):
            vec = self._vec = dict(shape=(S, H, W), ring=torch.zeros(self.max_envs, S, 512, device=dev),
                                   cache=[None] * self.max_envs)
        cache = vec["cache"]
        commands = [int(td["command"]) for td in obs_list]
        use_cache, mutate = lead.latent_cache, lead.mutate_route
        modes, firsts, rgbs, routes = [], [], [], []
        nf = 0
        for e, td in enumerate(obs_list):
            c = cache[e]
            hint = None if shifted is None else shifted[e]
            if c is None or not use_cache:
                m = False
            elif hint is not None:
                m = bool(hint)
            else:
                m = self._same_window(c, td)
            f = S - 1 if m else 0
            modes.append(1 if m else 0)
            firsts.append(nf)
            nf += S - f
            rgbs.append(td["rgb"][f:])
            routes.append(td["route_fig"][f:])
        rgb_d = torch.from_numpy(np.concatenate(rgbs)).to(dev)
        route_d = torch.from_numpy(np.concatenate(routes)).to(dev)
        rn_d = torch.empty_like(route_d) if mutate else None
        lat = torch.empty(nf, 512, device=dev)
        for s0 in range(0, nf, enc.max_frames):
            s1 = min(nf, s0 + enc.max_frames)
            x = enc.preprocess(rgb_d[s0:s1], route_d[s0:s1], None if rn_d is None else rn_d[s0:s1])
            enc.forward_nhwc(x, lat[s0:s1])
        # small inputs: one tiled row_seg per group + window descriptors + sort (int32), measurements (f64), noise (f32)
        pos, seg = command_rows(commands, C)
        segs = [tiled_seg(seg, C, grp.Mg).reshape(-1) for grp in self.groups]
        ints = np.concatenate(segs + [np.asarray(modes, np.int32), np.asarray(firsts, np.int32), pos,
                                      np.asarray(commands, np.int32)])
        ints_d = torch.from_numpy(ints).to(dev)
        seg_d, o = [], 0
        for s in segs:
            seg_d.append(ints_d[o:o + s.size])
            o += s.size
        mode_d, first_d, pos_d, cmd_d = (ints_d[o + i * N:o + (i + 1) * N] for i in range(4))
        meas = np.stack([np.asarray(td["measurements"], dtype=np.float64) for td in obs_list])
        meas_d = torch.from_numpy(np.ascontiguousarray(meas)).to(dev)
        nS, nT = self.n_out
        q_d = None
        if not deterministic:
            q = torch.ones(N, M, 2, 64)
            for e in range(N):                              # eval.py's order, environment after environment
                for m in range(M):
                    q[e, m, 0, :nS] = torch.empty(1, nS).exponential_(1)[0]
                    q[e, m, 1, :nT] = torch.empty(1, nT).exponential_(1)[0]
            q_d = q.to(dev)
        # LSTM input rows (sorted by command) into the first group's X — the other groups read the same block
        feat = torch.empty(N, S, a.DP, device=dev)            # fresh: callers keep references
        action = torch.empty(N, M, 2, dtype=torch.int64, device=dev)
        logp = torch.empty(N, M, 2, device=dev)
        value = torch.empty(N, M, 2, device=dev)
        X = None
        for gi, grp in enumerate(self.groups):
            ga, Zg = grp.arena, grp.arena.Z
            w = grp.learner.workspace(N, Zg, S)
            if X is None:
                X = w["X"]
                hip.check(L.cadre_act_windows(hip.ptr(vec["ring"]), vec["ring"].stride(0), vec["ring"].shape[0], hip.ptr(lat),
                                              lat.stride(0), nf, hip.ptr(mode_d), hip.ptr(first_d), hip.ptr(meas_d),
                                              hip.ptr(pos_d), N, S, hip.ptr(X), a.DP, a.DP, hip.ptr(feat), a.DP, stream),
                          "cadre_act_windows")
            else:
                w = dict(w, X=X)
            w["h0"].zero_(); w["c0"].zero_()
            # every net reads head block 0 of X (x_div = Z): all agents' steer and throttle nets see the same window
            grp.learner._forward(w, N, (0, 1, Zg), Zg, S=S, seg=seg_d[gi], fused_mlp=True)
            O3 = w["O3"]
            hip.check(L.cadre_sample_rows_ens(hip.ptr(O3), O3.stride(1), O3.stride(0), hip.ptr(pos_d), hip.ptr(cmd_d), N, C,
                                              grp.Mg, grp.m0, M, hip.ptr(q_d), nS, nT, hip.ptr(action), hip.ptr(logp),
                                              hip.ptr(value), hip.ptr(ga.ord), stream), "cadre_sample_rows_ens")
        ctl_d = torch.empty(N, 3, dtype=torch.float64, device=dev)
        hip.check(L.cadre_ensemble_controls(hip.ptr(action), N, M, hip.ptr(self.steer_tab), nS, hip.ptr(self.throttle_tab), nT,
                                            hip.ptr(ctl_d), stream), "cadre_ensemble_controls")
        # route quirk + window caches (the normalised route and the controls: the step's host copies)
        rn_h = rn_d.cpu().numpy() if rn_d is not None else None
        out = EnsembleActBatch()
        out.controls = ctl_d.cpu().tolist()
        for e, td in enumerate(obs_list):
            route_np = td["route_fig"]
            keep_raw = use_cache and (shifted is None or shifted[e] is not True)
            raw_rgb = td["rgb"].copy() if keep_raw else None
            raw_route = route_np.copy() if use_cache else None
            if rn_h is not None:
                if modes[e]:
                    route_np[:-1] = cache[e]["route_norm"][1:]
                    route_np[S - 1:] = rn_h[firsts[e]:firsts[e] + 1]
                else:
                    route_np[:] = rn_h[firsts[e]:firsts[e] + S]
            if use_cache:
                cache[e] = dict(rgb=raw_rgb, route_raw=raw_route, route_norm=route_np.copy())
            f = feat[e, :, :lead.lstm_input]
            out.append([(f, [action[e, m, 0], action[e, m, 1]], [logp[e, m, 0:1].view(1, 1), logp[e, m, 1:2].view(1, 1)],
                         [value[e, m, 0:1].view(1, 1), value[e, m, 1:2].view(1, 1)], ag.hidden_state)
                        for m, ag in enumerate(self.agent_group)])
        out.feat, out.action, out.logp, out.value = feat, action, logp, value
        return out


def ensemble_act_batch(agent_group, obs_list, shifted=None, deterministic=False, allowed=None):
    """CadreAgent.ensemble_act_batch: one EnsembleEvaluator per agent group, kept on the lead agent.  `allowed` is refused."""
    if allowed is not None:
        raise ValueError("ensemble evaluation takes no allowed= words: cadre_sample_rows_ens does not read action masks yet "
                         "(mask inside the environment loop of one agent with act_batch(allowed=))")
    lead = agent_group[0]
    key = tuple(id(a) for a in agent_group)
    cache = lead.__dict__.setdefault("_ens_eval", {})
    ev = cache.get(key)
    if ev is None:
        cache.clear()                                       # (one group per lead agent in practice; the arenas are large)
        ev = cache[key] = EnsembleEvaluator(agent_group)
    return ev.act(obs_list, shifted=shifted, deterministic=deterministic)


# ----------------------------------------------------------------------------- the host loop
def evaluate_vec(agent_group, envs, episodes, deterministic=False, callback=None, evaluator=None):
    """Run `episodes` evaluation episodes over the environments `envs` (reset / step(control) as eval.py:53-63 uses
    them), one `EnsembleEvaluator.act` per env step for the environments still running.  Returns the records
    dict(episode, env, length, reward_sum=(steer, throttle), info) in finishing order (rewards summed in float64 on the
    host; `info` is the last step's).  `callback("episode", record=..., schedule=...)` after every finished episode.
    `evaluator`: an EnsembleEvaluator to re-use (default: a new one for len(envs) environments).
    Window hints: an environment that was reset, or that now sits at another position of the active list (the list shrank
    in front of it), is announced as fresh (shifted False); the others are left to the evaluator's frame comparison."""
    sched = EpisodeSchedule(len(envs), episodes)
    if evaluator is None:
        evaluator = EnsembleEvaluator(agent_group, max_envs=len(envs))
    obs = {i: envs[i].reset() for i in sched.active}
    length = {i: 0 for i in sched.active}
    rsum = {i: np.zeros(2, dtype=np.float64) for i in sched.active}
    fresh, prev, records = set(sched.active), [], []
    while sched.active:
        act = list(sched.active)
        hints = [False if (i in fresh or p >= len(prev) or prev[p] != i) else None for p, i in enumerate(act)]
        out = evaluator.act([obs[i] for i in act], shifted=hints, deterministic=deterministic)
        fresh, prev = set(), act
        for p, i in enumerate(act):
            obs[i], reward, done, info = envs[i].step(list(out.controls[p]))
            length[i] += 1
            rsum[i] += np.asarray(reward, dtype=np.float64).reshape(2)
            if not done:
                continue
            ep, again = sched.finish(i)
            rec = dict(episode=ep, env=i, length=length[i], reward_sum=(float(rsum[i][0]), float(rsum[i][1])), info=info)
            records.append(rec)
            if callback is not None:
                callback("episode", record=rec, schedule=sched)
            if again:
                obs[i] = envs[i].reset()
                length[i], rsum[i] = 0, np.zeros(2, dtype=np.float64)
                fresh.add(i)
    return records


def evaluate(eval_cfg, agent_cfg, env_cfg, rollout_cfg, num_envs=1, env_cls=None):
    """eval.py:12-64 for `num_envs` routes at once: one agent per `eval_cfg.load_episode` entry, each loading
    `<pretrained_path>/models/ppo_model_<episode>.pt`; environment i gets env_cfg[k][i] for the per-worker keys, as
    train_vec creates them; `eval_cfg.eval_episode` episodes in all.  eval_cfg["deterministic"] (optional): greedy
    actions.  Returns evaluate_vec's records."""
    if env_cls is None:
        from env_wrapper import EnvWrapper as env_cls        # needs the CARLA stack (reference env_wrapper.py)
    if num_envs < 1:
        raise ValueError("evaluate: num_envs=%r" % (num_envs,))
    pretrained_path = eval_cfg["pretrained_path"]
    envs = []
    for i in range(num_envs):
        cfg = type(env_cfg)(env_cfg)
        cfg["rank"] = i
        for k in ("port", "routes", "scenarios", "town"):
            cfg[k] = env_cfg[k][i]
        cfg["seq_length"] = rollout_cfg["seq_length"]
        cfg["pretrained_path"] = pretrained_path
        envs.append(env_cls(cfg))
    agent_cfg["rank"] = 0
    agent_group = []
    for ep in eval_cfg["load_episode"]:
        agent = CadreAgent(**agent_cfg)
        agent.load_snapshot(os.path.join(pretrained_path, "models", "ppo_model_{}.pt".format(ep)), None)
        agent_group.append(agent)
    try:
        deterministic = bool(eval_cfg["deterministic"])
    except (KeyError, AttributeError):
        deterministic = False
    return evaluate_vec(agent_group, envs, eval_cfg["eval_episode"], deterministic=deterministic)
