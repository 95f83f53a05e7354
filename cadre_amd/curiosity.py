"""Curiosity bonus on the device: random network distillation on the latent rows of the rollout storages.

Burda et al. 2018 ("Exploration by Random Network Distillation"): a fixed random target network f and a trained predictor g of the
same shape see the state; the predictor's error e = mean_k (g_k - f_k)^2 is large where the state is new and is paid as an
intrinsic reward.  Here the state is the newest frame row of a storage's window row — 512 frozen-encoder latent values and the
measurements, already in HBM — so nothing is encoded again:

    cur = Curiosity(agent, n_envs, coeff=0.5)
    learner_section_multi(agent, rollouts, dones, ..., curiosity=cur, episode=e)

begin_section() runs three launches on the section's rollouts (cadre_rnd_obs_stats merges the rows into the running feature
statistics, cadre_rnd_forward normalises, runs both towers and forms e, cadre_rnd_reward scales e by the running deviation of its
carried sums and writes `rewards_mixed` = ext_coeff r + beta e / sigma of every storage); RolloutStorage.finish_rollouts(...,
intrinsic=cur) then hands `rewards_mixed` to the GAE launch where `rewards` stood.  update() runs behind the PPO steps: epochs x
minibatches predictor steps (cadre_rnd_forward with the saved activations, cadre_rnd_backward, the arena's cadre_clip_adam_graph on
the predictor's own flat buffer, moments and step counter).  beta lives in the module's device state block: a schedule writes it
there per episode and no launch changes.

Two deliberate departures from the paper:
  * One critic.  The mixed reward goes through the existing value heads; there is no second, non-episodic value head with its own
    discount (it would add parameters to the arena and change the snapshots).
  * The state that is scored.  The bonus of row t is the novelty of the state the action was taken IN; the paper scores the state
    reached.  Within a rollout that is a shift by one row; row T of a storage is not reliably the successor of row T - 1 here (the
    cursor drift of the reference).

The defaults are the paper's where it names one and plain choices otherwise; none has been tuned for this task.
"""
import math

import torch

from . import hip
from .phasic import _is_int, _is_number

CURIOSITY_KEYS = ("coeff", "ext_coeff", "gamma", "hidden", "embed", "lr", "epochs", "minibatches", "update_proportion", "obs_clip",
                  "seed", "max_norm")
DEFAULTS = dict(ext_coeff=1.0, gamma=0.99, hidden=128, embed=64, lr=1e-4, epochs=4, minibatches=4, update_proportion=0.25,
                obs_clip=5.0, seed=0, max_norm=1e30)
EPS_OBS = 1e-8          # under the root of a feature's variance
EPS_SIGMA = 1e-8        # under the root of the variance of the carried error sums
MASK_BITS = 24          # the mask compares the generator's top 24 bits with update_proportion * 2^24


def tower_offsets(D, H, E):
    """Offsets of W1 [D][H], b1 [H], W2 [H][H], b2 [H], W3 [H][E], b3 [E] in a tower's flat buffer, and its size."""
    o = [0, D * H, D * H + H, D * H + H + H * H, D * H + 2 * H + H * H, D * H + 2 * H + H * H + H * E]
    return o, o[5] + E


def _orthogonal(n_out, n_in, gain, gen):
    """torch.nn.init.orthogonal_'s rule from the module's own generator, in float64: [n_out][n_in]."""
    a = torch.randn(max(n_out, n_in), min(n_out, n_in), generator=gen, dtype=torch.float64)
    q, r = torch.linalg.qr(a)
    q = q * torch.sign(torch.diagonal(r)).unsqueeze(0)
    if n_out < n_in:
        q = q.t()
    return gain * q


def init_tower(D, H, E, gen):
    """One tower's flat float32 buffer: orthogonal weights (gain sqrt 2 for the hidden layers, 1 for the last), zero biases,
    every matrix stored input-major (the transpose of nn.Linear's)."""
    offs, P = tower_offsets(D, H, E)
    p = torch.zeros(P, dtype=torch.float32)
    for o, (n_out, n_in, gain) in zip(offs[0::2], ((H, D, math.sqrt(2.0)), (H, H, math.sqrt(2.0)), (E, H, 1.0))):
        p[o:o + n_in * n_out] = _orthogonal(n_out, n_in, gain, gen).t().contiguous().reshape(-1).float()
    return p


def mask_threshold(update_proportion):
    return int(float(update_proportion) * float(1 << MASK_BITS))


def curiosity_config(train_cfg_value):
    """train_cfg["curiosity"]: absent / None -> None (every launch, tensor and bit is what it is without the key); else a dict
    {"coeff" (required: the bonus coefficient beta — a number >= 0, ("linear", start, end) or a callable of episode / max_episode,
    ppo_agent.train.schedule_value, written to the state block per episode), "ext_coeff" (1.0: the factor of the raw reward),
    "gamma" (0.99, in [0, 1]: the discount of the carried error sums), "hidden" (128) and "embed" (64) (multiples of 32 up to
    256), "lr" (1e-4), "epochs" (4) x "minibatches" (4) predictor steps per rollout, "update_proportion" (0.25, in [0, 1]: the
    share of a step's rows that train the predictor), "obs_clip" (5.0), "seed" (0), "max_norm" (1e30: never clips)} -> the dict
    with defaults.  The defaults are untuned."""
    cfg = train_cfg_value
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("train_cfg.curiosity: expected None or a dict (got %r)" % (cfg,))
    unknown = sorted(set(cfg) - set(CURIOSITY_KEYS))
    if unknown or "coeff" not in cfg:
        raise ValueError("train_cfg.curiosity: needs coeff; known keys %r (unknown: %r)" % (CURIOSITY_KEYS, unknown))
    out = dict(DEFAULTS, **cfg)
    coeff = out["coeff"]
    if not callable(coeff):
        if isinstance(coeff, (tuple, list)):
            ok = len(coeff) == 3 and coeff[0] == "linear" and all(_is_number(v) and v >= 0 for v in coeff[1:])
        else:
            ok = _is_number(coeff) and coeff >= 0
        if not ok:
            raise ValueError("train_cfg.curiosity: coeff must be a number >= 0, (\"linear\", start, end) with both >= 0 or a callable "
                             "(got %r)" % (coeff,))
        out["coeff"] = tuple(coeff) if isinstance(coeff, (tuple, list)) else float(coeff)

    def number(key, lo, hi, lo_open=False):
        v = out[key]
        if not _is_number(v) or not (lo < v if lo_open else lo <= v) or not v <= hi:
            raise ValueError("train_cfg.curiosity: %s must be a number in %s%r, %r] (got %r)" % (key, "(" if lo_open else "[", lo, hi, v))
        out[key] = float(v)
    number("ext_coeff", 0.0, 1e30)
    number("gamma", 0.0, 1.0)
    number("lr", 0.0, 1.0, lo_open=True)
    number("update_proportion", 0.0, 1.0)
    number("obs_clip", 0.0, 1e30, lo_open=True)
    number("max_norm", 0.0, 1e300, lo_open=True)
    for key in ("hidden", "embed"):
        v = out[key]
        if not _is_int(v) or v < 32 or v > 256 or v % 32:
            raise ValueError("train_cfg.curiosity: %s must be a multiple of 32 in 32 .. 256 (got %r)" % (key, v))
        out[key] = int(v)
    for key in ("epochs", "minibatches"):
        v = out[key]
        if not _is_int(v) or not 1 <= v <= 1024:
            raise ValueError("train_cfg.curiosity: %s must be an integer 1 .. 1024 (got %r)" % (key, v))
        out[key] = int(v)
    if not _is_int(out["seed"]) or not 0 <= out["seed"] < 2 ** 32:
        raise ValueError("train_cfg.curiosity: seed must be an integer 0 .. 2^32 - 1 (got %r)" % (out["seed"],))
    out["seed"] = int(out["seed"])
    return out


def curiosity_refusals(reward_scaling=None, self_imitation=None, sample_reuse=None, checkpoint_interval=None, resume_from=None,
                       world=1, fused_gather=True):
    """What train_cfg["curiosity"] is refused with, each ValueError naming its key, before anything is allocated or launched."""
    if reward_scaling is not None and reward_scaling is not False:
        raise ValueError("train_cfg.curiosity excludes reward_scaling: its return statistics would be taken from the mixed rewards")
    if self_imitation is not None:
        raise ValueError("train_cfg.curiosity excludes self_imitation: its buffer reads storage.rewards, not the mixed rewards")
    if sample_reuse is not None:
        raise ValueError("train_cfg.curiosity excludes sample_reuse: its window reads storage.rewards, not the mixed rewards")
    if checkpoint_interval:
        raise ValueError("train_cfg.curiosity excludes checkpoint_interval: the checkpoint format does not hold the module")
    if resume_from is not None:
        raise ValueError("train_cfg.curiosity excludes resume_from: the checkpoint format does not hold the module")
    if world > 1:
        raise ValueError("train_cfg.curiosity needs a single rank (world size %d): each rank would train its own predictor" % world)
    if not fused_gather:
        raise ValueError("train_cfg.curiosity needs fused_gather=True")


class Curiosity(object):
    """Random network distillation for `n_envs` environments of two heads each.  agent_or_dims: a CadreAgent (its arena gives the
    feature width and the device) or the feature width D itself, 1 .. 1024 (then `device`).  The other arguments are the keys of
    curiosity_config.  Owns the two towers (`target`, `predictor`: flat float32 buffers, tower_offsets), the predictor's Adam
    moments and step counter, the float64 state block (hip.RND_*: feature statistics, carries, beta, ext_coeff, sigma, the mask
    generator's key and counter) and the workspaces.  train(False) freezes statistics, carries and predictor."""

    def __init__(self, agent_or_dims, n_envs, coeff=0.0, device=None, **keys):
        cfg = curiosity_config(dict(keys, coeff=coeff))
        if _is_int(agent_or_dims):
            D, dev = int(agent_or_dims), torch.device("cuda" if device is None else device)
        else:
            D, dev = int(agent_or_dims.arena.D), agent_or_dims.arena.device if device is None else torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if not 1 <= D <= 1024:
            raise ValueError("Curiosity: the feature width must be 1 .. 1024 (got %r)" % (D,))
        if not _is_int(n_envs) or not 1 <= n_envs <= 32767:
            raise ValueError("Curiosity: n_envs must be an integer 1 .. 32767 (got %r)" % (n_envs,))
        self.cfg, self.coeff, self.D, self.n_envs, self.device = cfg, cfg["coeff"], D, int(n_envs), dev
        self.H, self.E = cfg["hidden"], cfg["embed"]
        self.training = True
        gen = torch.Generator()
        gen.manual_seed(cfg["seed"])
        self.offsets, self.P = tower_offsets(D, self.H, self.E)
        self.target = init_tower(D, self.H, self.E, gen).to(dev)
        self.predictor = init_tower(D, self.H, self.E, gen).to(dev)
        self.grads = torch.zeros(self.P, device=dev)
        self.exp_avg = torch.zeros(self.P, device=dev)
        self.exp_avg_sq = torch.zeros(self.P, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self._seg_off = torch.tensor([0, self.P], dtype=torch.int64).to(dev)
        self._norms2 = torch.zeros(3, dtype=torch.float64, device=dev)
        state = torch.zeros(hip.RND_HEAD + 2 * D + self.n_envs, dtype=torch.float64)
        state[hip.RND_BETA] = coeff if _is_number(coeff) else 0.0
        state[hip.RND_EXT] = cfg["ext_coeff"]
        state[hip.RND_SIGMA] = 1.0
        state[hip.RND_KEY] = float(cfg["seed"])
        self.state = state.to(dev)
        self._beta = None
        self._tables = {}
        self._section = None        # (obs table, N, T, S, ldo) of the last begin_section
        self._err = None            # float32 [N][T] of the last begin_section
        self._ws = None
        self._loss = None           # float32 [steps][2] of the last update(): masked loss and mask count of every step
        self._loss_spare = torch.zeros(2, device=dev)
        self._after = None
        self._steps = 0
        self._rows = None

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def set_coeff(self, beta):
        """beta into the state block (one small asynchronous copy; no launch depends on the value)."""
        beta = float(beta)
        if not (beta >= 0.0 and math.isfinite(beta)):
            raise ValueError("Curiosity: the coefficient must be a finite number >= 0 (got %r)" % (beta,))
        if beta != self._beta:
            self.state[hip.RND_BETA:hip.RND_BETA + 1].fill_(beta)
            self._beta = beta
        return beta

    # ------------------------------------------------------------------ the section's chain
    def _table(self, key, rows):
        t = self._tables.get(key)
        if t is None:
            if len(self._tables) > 16:
                self._tables.clear()
            t = self._tables[key] = torch.tensor(rows, dtype=torch.int64).to(self.device)
        return t

    @staticmethod
    def mixed_of(storage):
        """`rewards_mixed` [T + 1, 1] of a storage, allocated the first time it is asked for."""
        m = getattr(storage, "rewards_mixed", None)
        if m is None or m.device != storage.rewards.device:
            m = storage.rewards_mixed = torch.zeros_like(storage.rewards)
        return m

    def begin_section(self, rollouts):
        """rollouts = [(steer_storage, throttle_storage), ...] of the section: statistics -> forward -> reward, three launches (two
        when frozen).  Afterwards errors() holds e [N][T] and every storage's `rewards_mixed` rows 0 .. T - 1 are written."""
        if len(rollouts) != self.n_envs:
            raise ValueError("Curiosity: built for %d environments, the section has %d" % (self.n_envs, len(rollouts)))
        flat = [s for pair in rollouts for s in pair]
        s0 = flat[0]
        if any(getattr(s, "_win", None) is not None for s in flat):
            raise ValueError("Curiosity: a frame-table storage keeps no window rows to read")
        # (the device of the tensors themselves: a storage built on "cuda" says so, its tensors say "cuda:0")
        geo = (s0.num_steps, s0.seq_length, s0._ldo, s0.z_dims, s0._obs.device)
        if any((s.num_steps, s.seq_length, s._ldo, s.z_dims, s._obs.device) != geo for s in flat):
            raise ValueError("Curiosity: every storage needs the same geometry and device")
        if s0.z_dims != self.D or s0._obs.device != self.state.device:
            raise ValueError("Curiosity: built for %d features on %s, the storages hold %d on %s"
                             % (self.D, self.state.device, s0.z_dims, s0._obs.device))
        N, T, S, ldo = self.n_envs, s0.num_steps, s0.seq_length, s0._ldo
        obs = tuple(hip.ptr(pair[0]._obs) for pair in rollouts)
        otab = self._table(("obs",) + obs, list(obs))
        rows = [[hip.ptr(s.rewards), hip.ptr(self.mixed_of(s))] for s in flat]
        rtab = self._table(("rows",) + tuple(p for r in rows for p in r), rows)
        if self._err is None or tuple(self._err.shape) != (N, T):
            self._err = torch.zeros(N, T, device=self.device)
        L, up = hip.lib(), 1 if self.training else 0
        hip.check(L.cadre_rnd_obs_stats(hip.ptr(otab), N, T, S, ldo, self.D, up, hip.ptr(self.state), hip.stream()), "cadre_rnd_obs_stats")
        self._section = (otab, N, T, S, ldo)
        self._forward(0, N * T, self._err, save=False)
        hip.check(L.cadre_rnd_reward(hip.ptr(self._err), N, T, hip.ptr(rtab), hip.ptr(self.state), self.D, self.cfg["gamma"], EPS_SIGMA,
                                     up, hip.stream()), "cadre_rnd_reward")
        self._rows, self._after, self._steps = flat, None, 0
        return self._err

    def _forward(self, row0, rows, err, save):
        otab, N, T, S, ldo = self._section
        ws = self._workspace(rows) if save else None
        sp = [hip.ptr(ws[k]) for k in ("xh", "h1", "h2", "diff")] if save else [None] * 4
        hip.check(hip.lib().cadre_rnd_forward(hip.ptr(otab), N, T, S, ldo, self.D, self.H, self.E, row0, rows, hip.ptr(self.state), EPS_OBS,
                                              self.cfg["obs_clip"], hip.ptr(self.target), hip.ptr(self.predictor), hip.ptr(err), *sp,
                                              hip.stream()), "cadre_rnd_forward")

    def _workspace(self, rows):
        ws = self._ws
        if ws is None or ws["rows"] < rows:
            z = lambda *s: torch.zeros(*s, device=self.device)
            ws = self._ws = dict(rows=rows, xh=z(rows, self.D), h1=z(rows, self.H), h2=z(rows, self.H), diff=z(rows, self.E), err=z(rows),
                                 scratch=z(rows * (self.E + 2 * self.H + 1) + 2))
        return ws

    def backward(self, rows):
        """cadre_rnd_backward on the activations the last saving forward left: the gradient buffer and loss[2] (masked loss, count)."""
        ws = self._ws
        loss = self._loss[self._steps] if self._loss is not None and self._steps < self._loss.shape[0] else self._loss_spare
        hip.check(hip.lib().cadre_rnd_backward(hip.ptr(ws["xh"]), hip.ptr(ws["h1"]), hip.ptr(ws["h2"]), hip.ptr(ws["diff"]), hip.ptr(ws["err"]),
                                               rows, self.D, self.H, self.E, hip.ptr(self.predictor), hip.ptr(self.state),
                                               mask_threshold(self.cfg["update_proportion"]), hip.ptr(self.grads), hip.ptr(loss),
                                               hip.ptr(ws["scratch"]), hip.stream()), "cadre_rnd_backward")
        return loss

    def adam(self):
        """The existing optimiser step (cadre_clip_adam_graph, one model) on the predictor's flat buffer."""
        hip.check(hip.lib().cadre_clip_adam_graph(hip.ptr(self.predictor), hip.ptr(self.grads), hip.ptr(self.exp_avg), hip.ptr(self.exp_avg_sq),
                                                  hip.ptr(self._seg_off), 1, hip.ptr(self._norms2), self.cfg["max_norm"], self.cfg["lr"], 0.9,
                                                  0.999, 1e-8, hip.ptr(self.step_dev), hip.stream()), "cadre_clip_adam_graph")

    def steps_per_section(self, rows):
        return self.cfg["epochs"] * sum(1 for lo, hi in self._chunks(rows) if hi > lo)

    def _chunks(self, rows):
        mb = self.cfg["minibatches"]
        return [(j * rows // mb, (j + 1) * rows // mb) for j in range(mb)]

    def update(self, stats=False):
        """The predictor steps of the section begin_section opened: `epochs` passes over the rollout's rows in `minibatches`
        contiguous runs of the (worker, time) order; each step is forward (activations kept) -> backward -> Adam.  Nothing runs
        when frozen.  stats: one more forward afterwards, whose mean error summary() reports as the loss after the steps."""
        if self._section is None:
            raise ValueError("Curiosity.update: no section is open (begin_section first)")
        if not self.training:
            return 0
        _otab, N, T, _S, _ldo = self._section
        R = N * T
        self._loss = torch.zeros(self.steps_per_section(R), 2, device=self.device)
        self._steps = 0
        self._workspace(max(hi - lo for lo, hi in self._chunks(R)))      # (sized once, for the section's largest run of rows)
        for _epoch in range(self.cfg["epochs"]):
            for lo, hi in self._chunks(R):
                if hi <= lo:
                    continue
                self._forward(lo, hi - lo, self._workspace(hi - lo)["err"], save=True)
                self.backward(hi - lo)
                self.adam()
                self._steps += 1
        if stats:
            self._after = torch.zeros(N, T, device=self.device)
            self._forward(0, R, self._after, save=False)
        return self._steps

    # ------------------------------------------------------------------ what it reports
    def errors(self):
        """e [N][T] of the last begin_section (device float32)."""
        return self._err

    def sigma(self):
        return self.state[hip.RND_SIGMA]

    def summary(self):
        """The "curiosity" entry of a section's `stats`: mean and max e, sigma, beta, mean |beta r_int|, mean |ext_coeff r| over
        the section's rows, the predictor steps taken and the predictor's mean error before and after them (after: None unless
        update(stats=True) ran).  One small device-to-host copy."""
        if self._err is None:
            return dict(steps=0)
        e = self._err.double()
        st = self.state
        sig = st[hip.RND_SIGMA].float().double()
        r = torch.stack([s.rewards[:s.num_steps, 0] for s in self._rows]).double()
        vals = torch.stack([e.mean(), e.max(), st[hip.RND_SIGMA], st[hip.RND_BETA], (st[hip.RND_BETA] * e / sig).abs().mean(),
                            (st[hip.RND_EXT] * r).abs().mean(),
                            self._after.double().mean() if self._after is not None else e.new_tensor(float("nan"))]).cpu().tolist()
        return dict(steps=self._steps, mean_e=vals[0], max_e=vals[1], sigma=vals[2], beta=vals[3], mean_abs_bonus=vals[4],
                    mean_abs_ext=vals[5], loss_before=vals[0], loss_after=None if math.isnan(vals[6]) else vals[6])

    # ------------------------------------------------------------------ plain-tensor state
    def state_dict(self):
        return dict(target=self.target.clone(), predictor=self.predictor.clone(), exp_avg=self.exp_avg.clone(),
                    exp_avg_sq=self.exp_avg_sq.clone(), step=self.step_dev.clone(), state=self.state.clone(),
                    dims=torch.tensor([self.D, self.H, self.E, self.n_envs], dtype=torch.int64))

    def load_state_dict(self, sd):
        missing = sorted({"target", "predictor", "exp_avg", "exp_avg_sq", "step", "state", "dims"} - set(sd))
        if missing:
            raise ValueError("Curiosity.load_state_dict: missing %r" % (missing,))
        if sd["dims"].tolist() != [self.D, self.H, self.E, self.n_envs]:
            raise ValueError("Curiosity.load_state_dict: a state for (features, hidden, embed, environments) = %r does not fit %r"
                             % (sd["dims"].tolist(), [self.D, self.H, self.E, self.n_envs]))
        for k, dst in (("target", self.target), ("predictor", self.predictor), ("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq),
                       ("step", self.step_dev), ("state", self.state)):
            if tuple(sd[k].shape) != tuple(dst.shape):
                raise ValueError("Curiosity.load_state_dict: %s has shape %r, expected %r" % (k, tuple(sd[k].shape), tuple(dst.shape)))
            dst.copy_(sd[k].to(dst.device, dst.dtype))
        self._beta = None


def curiosity_stats_text(stats):
    """What stats_line appends for a section that ran with the curiosity bonus."""
    c = stats["curiosity"]
    if "mean_e" not in c:
        return ", curiosity: no rows"
    after = "n/a" if c["loss_after"] is None else "{:.4e}".format(c["loss_after"])
    return (", curiosity: e {:.4e} (max {:.4e}), sigma {:.4e}, beta {:.4f}, |bonus| {:.4e} vs |reward| {:.4e}, predictor loss {:.4e} -> {} "
            "in {} steps").format(c["mean_e"], c["max_e"], c["sigma"], c["beta"], c["mean_abs_bonus"], c["mean_abs_ext"],
                                  c["loss_before"], after, c["steps"])


def curiosity_runner(agent, train_cfg_value, n_envs, **refusal_args):
    """The Curiosity of a training loop, or None when the key is absent / None.  curiosity_refusals(**refusal_args) first."""
    cfg = curiosity_config(train_cfg_value)
    if cfg is None:
        return None
    curiosity_refusals(**refusal_args)
    return Curiosity(agent, n_envs, **cfg)
