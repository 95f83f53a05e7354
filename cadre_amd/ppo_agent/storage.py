"""Mirror of reference ppo_agent/storage.py: per-worker, per-head rollout buffer living in HBM.

Same constructor, attributes, cursor semantics (including the modulo-(T+1) drift: `after_update`
is never called by the reference train loop, storage.py:57-66) and generator contract.  The
math is HIP: GAE + advantage normalisation = cadre_gae (strict fp32 order, bit-exact with
storage.py:69-76), the time-major minibatch gather = cadre_gather_obs.  Feature rows are
stored with a 544-float pitch (530 + zero pad) so they feed the GEMMs without re-packing;
`.obs` / `.hn` / `.cn` expose the reference's [.., 530] shapes as views."""
import torch

from .. import hip

PAD = 32


def _rup(x, m):
    return (x + m - 1) // m * m


class RolloutStorage(object):
    _insert_tables = {}          # insert_batch: device pointer tables of storage sets, keyed by the pointers
    _finish_tables = {}          # finish_rollouts: likewise

    def __init__(self, num_steps, mini_batch_num, feature_dims, seq_length, hidden_size, use_gae, gamma, tau, device="cpu"):
        """`device` (not in the reference, which allocates on the CPU and moves with .to()): allocate there at once."""
        T = num_steps
        self.mini_batch_num = mini_batch_num
        self.num_steps = T
        self.z_dims = feature_dims
        self.seq_length = seq_length
        self.hid_size = hidden_size
        self.use_gae = use_gae
        self.gamma = gamma
        self.tau = tau
        self.step = 0
        self._tl_used = False        # a time-limit flag was ever written: the finishing stage then reads time_limits
        self._ldo = _rup(feature_dims, PAD)
        self._ldh = _rup(hidden_size, PAD)
        self._alloc(torch.device(device))

    def _alloc(self, device):
        T = self.num_steps
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=device)
        self.device = device
        self._alloc_obs(device)
        self._hn = z(T + 1, self._ldh)
        self._cn = z(T + 1, self._ldh)
        self.hn = self._hn[:, :self.hid_size]
        self.cn = self._cn[:, :self.hid_size]
        self.command = z(T + 1, 1, dtype=torch.int)
        self.rewards = z(T + 1, 1)
        self.value_preds = z(T + 1, 1)
        self.returns = z(T + 1, 1)
        self.action_log_probs = z(T + 1, 1)
        self.action = z(T + 1, 1, dtype=torch.long)
        self.masks = z(T + 1, 1)
        self.time_limits = z(T + 1, 1)       # 1 where the row's episode was cut by a step limit (insert(time_limit=True))
        self.advantages = z(T, 1)            # filled by compute_returns (train.py:82-88)
        self._next = z(1)

    def _alloc_obs(self, device):
        """The window rows (cadre_amd.frames.FrameStorage keeps frames and window ids in their place)."""
        self._obs = torch.zeros(self.num_steps + 1, self.seq_length, self._ldo, dtype=torch.float32, device=device)
        self.obs = self._obs[:, :, :self.z_dims]

    def to(self, device):
        device = torch.device(device)
        old = {k: getattr(self, k) for k in ("_obs", "_hn", "_cn", "command", "rewards", "value_preds", "returns",
                                             "action_log_probs", "action", "masks", "advantages", "time_limits")}
        self._alloc(device)
        for k, v in old.items():
            getattr(self, k).copy_(v)
        if getattr(self, "events", None) is not None:        # (exploration suggestions: the two tensors travel along)
            self.events, self.suggest = self.events.to(device), self.suggest.to(device)
        if getattr(self, "allowed", None) is not None:       # (action masks: the words travel along)
            self.allowed = self.allowed.to(device)
        if getattr(self, "costs", None) is not None:         # (cost constraints: the costs travel along)
            self.costs = self.costs.to(device)

    def _costs_tensor(self):
        """`costs` float32 [T + 1] (the cost of each row for this head; 0: none; see cadre_amd.constraint), allocated the first
        time a cost is passed: a storage that never saw one has no such tensor and keeps today's launches and tensors."""
        if getattr(self, "costs", None) is None:
            self.costs = torch.zeros(self.num_steps + 1, dtype=torch.float32, device=self.device)
        return self.costs

    @staticmethod
    def _cost_value(c):
        import math
        if isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or c < 0:
            raise ValueError("cost %r: expected a finite number >= 0" % (c,))
        return float(c)

    def _allowed_tensor(self):
        """`allowed` int64 [T + 1] (the allowed-bin word of each row; 0: unmasked), allocated the first time a word is passed: a
        storage that never saw one has no such tensor and keeps today's launches and tensors."""
        if getattr(self, "allowed", None) is None:
            self.allowed = torch.zeros(self.num_steps + 1, dtype=torch.int64, device=self.device)
        return self.allowed

    @staticmethod
    def _allowed_word(w, K=None):
        """A Python-int word -> its int64 bit pattern (cadre_amd.actmask.check_word / word_i64: the one statement of the check).  A
        word that allows none of the head's K bins is refused: the kernels would read it as 'unmasked'.  A storage does not know its
        head's K: without `K` only the all-zero word can be refused (K = 64)."""
        from ..actmask import check_word, word_i64
        return word_i64(check_word(w, 64 if K is None else K, "allowed word"))

    def _event_tensors(self):
        """`events` int32 [T + 1] (the terminal-event code of each row, 0: none) and `suggest` int32 [T] (the kind
        cadre_suggest_mark gives each row), allocated the first time an event argument is passed: a storage that never saw
        one has neither attribute and keeps today's launches and tensors."""
        if getattr(self, "events", None) is None:
            self.events = torch.zeros(self.num_steps + 1, dtype=torch.int32, device=self.device)
            self.suggest = torch.zeros(self.num_steps, dtype=torch.int32, device=self.device)
        return self.events

    @staticmethod
    def _event_code(e):
        if isinstance(e, bool) or not isinstance(e, int) or not 0 <= e < 2 ** 31:
            raise ValueError("event code %r: expected a small non-negative integer (0: none)" % (e,))
        return e

    def insert(self, obs, action, action_log_probs, value_preds, rewards, masks, hidden_state, command, time_limit=False,
               event=0, allowed=None, allowed_bins=None, cost=None):
        """storage.py:45-58.  `time_limit`: this row's episode was cut by a step budget, not ended (see finish_rollouts).
        `event`: the code of the terminal event this row ends with for this head (0: none; see cadre_amd.suggest).  Once a
        storage has seen a code every insert writes the slot, zeros included: a stale code never survives the cursor's
        drift.  `allowed` (action masks): the word this head's action was sampled under (a Python int; None: unmasked).  Once
        a storage has seen a word every insert writes the slot, 0 = unmasked included.  `allowed_bins`: the head's K; with it a
        word without a bit among the K bins is refused, without it only the all-zero word (the storage does not know K).
        `cost` (cost constraints): this head's cost of the row, a finite number >= 0 (None: none).  Once a storage has seen a
        cost every insert writes the slot, 0 included."""
        s = self.step
        event = self._event_code(event)
        cost = None if cost is None else self._cost_value(cost)                            # (checked before anything is written)
        word = None if allowed is None else self._allowed_word(allowed, allowed_bins)      # (checked before anything is written)
        if allowed is not None or getattr(self, "allowed", None) is not None:
            self._allowed_tensor()[s] = 0 if word is None else word
        if event or getattr(self, "events", None) is not None:
            self._event_tensors()[s] = event
        if cost is not None or getattr(self, "costs", None) is not None:
            self._costs_tensor()[s] = 0.0 if cost is None else cost
        if time_limit or self._tl_used:          # (a storage that never saw a flag keeps the reference's launches)
            self.time_limits[s] = 1.0 if time_limit else 0.0
            self._tl_used = True
        self.action[s].copy_(torch.as_tensor(action).reshape(-1)[:1])
        self.action_log_probs[s].copy_(torch.as_tensor(action_log_probs).reshape(-1)[:1])
        self.value_preds[s].copy_(torch.as_tensor(value_preds).reshape(-1)[:1])
        self.rewards[s].copy_(torch.as_tensor(rewards, dtype=torch.float32).reshape(-1)[:1])
        self.obs[s].copy_(obs.reshape(self.seq_length, self.z_dims))
        if hidden_state is not None and s < self.num_steps:
            hn, cn = hidden_state
            self.hn[s + 1].copy_(hn.reshape(-1))
            self.cn[s + 1].copy_(cn.reshape(-1))
        self.masks[s].copy_(torch.as_tensor(masks).reshape(-1)[:1])
        self.command[s] = command
        self.step = (s + 1) % (self.num_steps + 1)

    @staticmethod
    def insert_batch(storages, outputs, rewards, masks, commands, time_limits=None, events=None, allowed=None, n_out=None,
                     costs=None):
        """`insert` (storage.py:45-58) of one env step of N environments into their 2N storages in ONE launch
        (cadre_insert_rows; with `time_limits` its twin cadre_insert_rows_tl, which writes the flags in the same launch):
        time_limits = None, or per environment a bool or a (steer, throttle) pair of bools.  storages = [(steer_rollout, throttle_rollout), ...] per environment, outputs = what
        CadreAgent.act_batch returned for them, rewards / masks = [N][2] (steer, throttle) host values, commands = the N
        host-side commands.  The hidden state written is act()'s zeros.  The cursors (and their modulo-(T+1) drift) stay
        host-side ints, exactly as `insert` keeps them.
        `events` (exploration suggestions): None, or per environment an int code or a (steer, throttle) pair of codes (0:
        none).  All 2N codes of the step are written by ONE extra launch (cadre_suggest_note), which is not issued when
        `events` is None and no storage has the tensor.
        `allowed` (action masks): None, per environment a (steer, throttle) pair of Python-int words, or the device int64
        [N][2] tensor act_batch sampled under.  All 2N words of the step are written by ONE extra launch (cadre_allowed_note),
        which is not issued when `allowed` is None and no storage has the tensor (it then writes 0 = unmasked).  `n_out` =
        (K_steer, K_throttle): with it a Python-int word without a bit among its head's bins is refused, without it only the
        all-zero word (the storages do not know K); a device tensor is taken as it is, as act_batch took it.
        `costs` (cost constraints): None, or per environment a finite number >= 0 (written to both heads) or a (steer,
        throttle) pair.  All 2N costs of the step are written by ONE extra launch (cadre_cost_note), which is not issued when
        `costs` is None and no storage has the tensor (it then writes 0)."""
        N = len(storages)
        co = None
        if costs is not None:                # (checked before anything is launched)
            if len(costs) != N or any(isinstance(c, (tuple, list)) and len(c) != 2 for c in costs):
                raise ValueError("insert_batch: %d storage pairs, costs must hold as many numbers or (steer, throttle) pairs" % N)
            co = [RolloutStorage._cost_value(v) for c in costs for v in (c if isinstance(c, (tuple, list)) else (c, c))]
        al = None
        if allowed is not None:              # (checked before anything is launched)
            if torch.is_tensor(allowed):
                if allowed.dtype != torch.int64 or tuple(allowed.shape) != (N, 2) or not allowed.is_cuda:
                    raise ValueError("insert_batch: allowed must be a device int64 [%d][2] tensor or %d (steer, throttle) pairs" % (N, N))
                al = allowed.contiguous()
            else:
                if len(allowed) != N or any(not isinstance(e, (tuple, list)) or len(e) != 2 for e in allowed):
                    raise ValueError("insert_batch: %d storage pairs, allowed must hold as many (steer, throttle) pairs of words" % N)
                al = [RolloutStorage._allowed_word(w, None if n_out is None else n_out[h]) for e in allowed for h, w in enumerate(e)]
        if events is not None and len(events) != N:
            raise ValueError("insert_batch: %d storage pairs, %d event codes" % (N, len(events)))
        ev = None
        if events is not None:               # (checked before anything is launched)
            if any(isinstance(e, (tuple, list)) and len(e) != 2 for e in events):
                raise ValueError("insert_batch: an event entry is an int or a (steer, throttle) pair")
            ev = [RolloutStorage._event_code(c) for e in events for c in (e if isinstance(e, (tuple, list)) else (e, e))]
        if time_limits is not None and len(time_limits) != N:
            raise ValueError("insert_batch: %d storage pairs, %d time-limit flags" % (N, len(time_limits)))
        if N < 1 or len(outputs) != N or len(rewards) != N or len(masks) != N or len(commands) != N:
            raise ValueError("insert_batch: %d storage pairs, %d outputs, %d rewards, %d masks, %d commands"
                             % (N, len(outputs), len(rewards), len(masks), len(commands)))
        flat = [s for pair in storages for s in pair]
        if len(flat) != 2 * N:
            raise ValueError("insert_batch: storages must be (steer, throttle) pairs")
        if any(getattr(s, "_win", None) is not None for s in flat):
            raise ValueError("insert_batch: a frame-table storage is not filled row by row (insert gets no frame identity); "
                             "DemoSet.from_episodes(frame_table=True) and AuxBuffer(frames_per_row=) build one")
        s0 = flat[0]
        geo = (s0.num_steps, s0.seq_length, s0._ldo, s0._ldh, s0.z_dims, s0.hid_size, s0.device)
        if any((s.num_steps, s.seq_length, s._ldo, s._ldh, s.z_dims, s.hid_size, s.device) != geo for s in flat):
            raise ValueError("insert_batch: every storage needs the same geometry and device")
        if s0.device.type != "cuda":
            raise hip.CadreHipError("RolloutStorage.insert_batch runs on the HIP device: call .to('cuda:N') first")
        dev = s0.device
        feat = getattr(outputs, "feat", None)
        if feat is not None:
            action, logp, value = outputs.action, outputs.logp, outputs.value
        else:                                   # a plain list of act() tuples: one buffer per output kind
            feat = torch.stack([o[0].reshape(s0.seq_length, -1) for o in outputs])
            action = torch.stack([torch.stack([o[1][0].reshape(()), o[1][1].reshape(())]) for o in outputs]).to(torch.int64)
            logp = torch.stack([torch.stack([o[2][0].reshape(()), o[2][1].reshape(())]) for o in outputs]).float()
            value = torch.stack([torch.stack([o[3][0].reshape(()), o[3][1].reshape(())]) for o in outputs]).float()
        feat, action, logp, value = (t.to(dev).contiguous() for t in (feat, action, logp, value))
        if feat.dim() != 3 or feat.shape[0] != N or feat.shape[1] != s0.seq_length or feat.shape[2] < s0.z_dims:
            raise ValueError("insert_batch: features of shape %s for %d environments x %d x %d"
                             % (tuple(feat.shape), N, s0.seq_length, s0.z_dims))
        if time_limits is None and any(s._tl_used for s in flat):       # (flags of an earlier pass must not stay in the rows)
            time_limits = [False] * N
        tl = None
        if time_limits is not None:
            tl = [[bool(f[0]), bool(f[1])] if isinstance(f, (tuple, list)) else [bool(f), bool(f)] for f in time_limits]
        ptrs = [[hip.ptr(s._obs), hip.ptr(s._hn), hip.ptr(s._cn), hip.ptr(s.action), hip.ptr(s.action_log_probs),
                 hip.ptr(s.value_preds), hip.ptr(s.rewards), hip.ptr(s.masks), hip.ptr(s.command)] +
                ([hip.ptr(s.time_limits)] if tl is not None else []) for s in flat]
        key = tuple(p for row in ptrs for p in row)
        tables = RolloutStorage._insert_tables
        table = tables.get(key)
        if table is None:
            if len(tables) > 16:
                tables.clear()
            table = tables[key] = torch.tensor(ptrs, dtype=torch.int64).to(dev)
        slots = [s.step for s in flat]
        ints = torch.tensor(slots + [int(c) for c in commands], dtype=torch.int32).to(dev)
        rm = torch.tensor([[float(rewards[e][h]), float(torch.as_tensor(masks[e][h]).reshape(-1)[0])] +
                           ([float(tl[e][h])] if tl is not None else [])
                           for e in range(N) for h in (0, 1)], dtype=torch.float32).to(dev)
        name = "cadre_insert_rows" if tl is None else "cadre_insert_rows_tl"
        hip.check(getattr(hip.lib(), name)(hip.ptr(table), hip.ptr(ints), 2 * N, s0.seq_length, s0._ldo, s0._ldh,
                                           s0.z_dims, s0.hid_size, s0.num_steps, hip.ptr(feat), feat.stride(1),
                                           hip.ptr(action), hip.ptr(logp), hip.ptr(value), hip.ptr(rm),
                                           hip.ptr(ints[2 * N:]), hip.stream()), name)
        if tl is not None:
            for s in flat:
                s._tl_used = True
        if events is not None or any(getattr(s, "events", None) is not None for s in flat):
            ev = [0] * (2 * N) if ev is None else ev
            eptrs = tuple(hip.ptr(s._event_tensors()) for s in flat)
            etable = tables.get(("events",) + eptrs)
            if etable is None:
                etable = tables[("events",) + eptrs] = torch.tensor(eptrs, dtype=torch.int64).to(dev)
            codes = torch.tensor(ev, dtype=torch.int32).to(dev)
            hip.check(hip.lib().cadre_suggest_note(hip.ptr(etable), hip.ptr(ints), hip.ptr(codes), 2 * N, s0.num_steps,
                                                   hip.stream()), "cadre_suggest_note")
        if al is not None or any(getattr(s, "allowed", None) is not None for s in flat):
            aptrs = tuple(hip.ptr(s._allowed_tensor()) for s in flat)
            atable = tables.get(("allowed",) + aptrs)
            if atable is None:
                atable = tables[("allowed",) + aptrs] = torch.tensor(aptrs, dtype=torch.int64).to(dev)
            if al is None:
                words = torch.zeros(2 * N, dtype=torch.int64, device=dev)
            elif torch.is_tensor(al):
                words = al.to(dev).reshape(-1)
            else:
                words = torch.tensor(al, dtype=torch.int64).to(dev)
            hip.check(hip.lib().cadre_allowed_note(hip.ptr(atable), hip.ptr(ints), hip.ptr(words), 2 * N, s0.num_steps,
                                                   hip.stream()), "cadre_allowed_note")
        if co is not None or any(getattr(s, "costs", None) is not None for s in flat):
            cptrs = tuple(hip.ptr(s._costs_tensor()) for s in flat)
            ctable = tables.get(("costs",) + cptrs)
            if ctable is None:
                ctable = tables[("costs",) + cptrs] = torch.tensor(cptrs, dtype=torch.int64).to(dev)
            vals = torch.tensor([0.0] * (2 * N) if co is None else co, dtype=torch.float32).to(dev)
            hip.check(hip.lib().cadre_cost_note(hip.ptr(ctable), hip.ptr(ints), hip.ptr(vals), 2 * N, s0.num_steps,
                                                hip.stream()), "cadre_cost_note")
        for s in flat:
            s.step = (s.step + 1) % (s.num_steps + 1)

    def after_update(self, hidden_state):
        self.step = 0
        if hidden_state is not None:
            hn, cn = hidden_state
            self.hn[0].copy_(hn.reshape(-1))
            self.cn[0].copy_(cn.reshape(-1))

    def compute_returns(self, next_value, normalise=True, explained_variance=None):
        """storage.py:68-76 (GAE branch) + the caller-side advantage lines train.py:82-88.
        `self.advantages` holds (ret[:-1]-V[:-1]) normalised with the unbiased std when `normalise`.
        `explained_variance` (optional device float64 tensor of one element): receives 1 - Var(R - V) / Var(R) of the
        value head over the T GAE rows, computed on the device after the GAE launch (RolloutStorage.explained_variance)."""
        if not self.use_gae:
            raise NotImplementedError("use_gae=False branch (storage.py:77-86) is dead in the reference config")
        if not self.returns.is_cuda:
            raise hip.CadreHipError("RolloutStorage.compute_returns runs on the HIP device: call .to('cuda:N') first")
        if self._tl_used:                        # time-limit flags were written: the scan that knows them, n = 1
            return RolloutStorage.finish_rollouts([self], [next_value], normalise=normalise,
                                                  explained_variance=explained_variance)[0]
        import numpy as np
        self._next.copy_(torch.as_tensor(next_value, dtype=torch.float32).reshape(-1)[:1])
        g32 = float(np.float32(self.gamma))
        gt32 = float(np.float32(self.gamma * self.tau))          # double product, then one rounding (storage.py:75)
        hip.check(hip.lib().cadre_gae(hip.ptr(self.rewards), hip.ptr(self.value_preds), hip.ptr(self.masks),
                                      hip.ptr(self._next), hip.ptr(self.returns), hip.ptr(self.advantages), 1,
                                      self.num_steps, g32, gt32, 1 if normalise else 0, hip.stream()), "cadre_gae")
        if explained_variance is not None:
            RolloutStorage.explained_variance([self], explained_variance)
        return self.advantages

    @staticmethod
    def finish_rollouts(storages, next_values, normalise=True, reward_scaler=None, explained_variance=None, consensus=None,
                        intrinsic=None):
        """compute_returns of every storage of a learner section in ONE launch (cadre_gae_multi): storages = the flat list
        [steer_0, throttle_0, steer_1, ...] (storage k belongs to head k & 1), next_values = one bootstrap value each.
        Returns the list of `advantages` tensors.  Without time-limit flags and without a scaler, returns, advantages and
        value_preds[T] are bit-identical to compute_returns per storage.
        Time limits (`insert(time_limit=True)`): in the scan, after gae_t = delta_t + gamma tau m_t gae_{t+1}, a cut row
        gets gae_t = 0, so returns[t] == value_preds[t]; the chain restarts behind the cut and row t - 1 bootstraps from
        value_preds[t].  A cut row's advantage is 0 before normalisation and is NOT excluded from the mean / std.
        `reward_scaler` (a ReturnScaler): one cadre_return_stats launch first updates the running statistics of the
        discounted returns (when scaler.training) and the scale of each head; the scan then reads every reward as
        clamp(r * scale_head, -clip, clip).  `storage.rewards` keeps the raw rewards.
        `explained_variance` (device float64 [len(storages)]): filled by RolloutStorage.explained_variance afterwards.
        `consensus` (a Shared_grad_buffers, with a `reward_scaler`; several ranks): after cadre_return_stats has grown THIS
        rank's statistics, every rank puts its six numbers (count, mean, M2 per head) into its own row of a zeroed
        [world][6] float64 buffer, the buffer is summed over the ranks (consensus.all_reduce_small: a gather, x + 0 is
        exact) and cadre_return_scale_merge forms the scale of each head from the ranks' statistics merged in rank order —
        the same two scales on every rank.  The rank's own statistics and carries stay its own.  Every rank must pass it
        at the same rollouts (the collective is issued whenever the scaler is training); a no-op without an exchange.
        `intrinsic` (a cadre_amd.curiosity.Curiosity whose begin_section ran on these storages; excludes `reward_scaler`): the
        first pointer of every row of the table is the storage's `rewards_mixed` in place of `rewards`; the launch and every
        other pointer are today's.  `storage.rewards` keeps the raw rewards."""
        import numpy as np
        n = len(storages)
        if intrinsic is not None and reward_scaler is not None:
            raise ValueError("finish_rollouts: intrinsic excludes reward_scaler (its statistics would be taken from the mixed rewards)")
        if n < 1 or len(next_values) != n:
            raise ValueError("finish_rollouts: %d storages, %d next values" % (n, len(next_values)))
        s0 = storages[0]
        if any((s.num_steps, s.gamma, s.tau, s.device) != (s0.num_steps, s0.gamma, s0.tau, s0.device) for s in storages):
            raise ValueError("finish_rollouts: every storage needs the same num_steps, gamma, tau and device")
        if not all(s.use_gae for s in storages):
            raise NotImplementedError("use_gae=False branch (storage.py:77-86) is dead in the reference config")
        if reward_scaler is not None:
            if 2 * reward_scaler.n_envs != n:
                raise ValueError("finish_rollouts: a ReturnScaler for %d environments with %d storages (two per environment)"
                                 % (reward_scaler.n_envs, n))
            if reward_scaler.state.device != s0.device:
                raise ValueError("finish_rollouts: the ReturnScaler lives on %s, the storages on %s"
                                 % (reward_scaler.state.device, s0.device))
        if s0.device.type != "cuda":
            raise hip.CadreHipError("RolloutStorage.finish_rollouts runs on the HIP device: call .to('cuda:N') first")
        for s, v in zip(storages, next_values):
            s._next.copy_(torch.as_tensor(v, dtype=torch.float32).reshape(-1)[:1])
        flags = any(s._tl_used for s in storages)
        rows = [[hip.ptr(s.rewards if intrinsic is None else intrinsic.mixed_of(s)), hip.ptr(s.value_preds), hip.ptr(s.masks),
                 hip.ptr(s._next), hip.ptr(s.returns),
                 hip.ptr(s.advantages), hip.ptr(s.time_limits) if flags else 0] for s in storages]
        key = tuple(p for row in rows for p in row)
        tables = RolloutStorage._finish_tables
        table = tables.get(key)
        if table is None:
            if len(tables) > 16:
                tables.clear()
            table = tables[key] = torch.tensor(rows, dtype=torch.int64).to(s0.device)
        L, T = hip.lib(), s0.num_steps
        state = None
        if reward_scaler is not None:
            state = reward_scaler.state
            hip.check(L.cadre_return_stats(hip.ptr(table), n, T, float(reward_scaler.gamma), float(reward_scaler.epsilon),
                                           1 if reward_scaler.training else 0, hip.ptr(state),
                                           hip.ptr(reward_scaler._scratch), hip.stream()), "cadre_return_stats")
            if consensus is not None and reward_scaler.training and consensus.dist_world():
                import torch.distributed as dist
                world, rank = dist.get_world_size(), dist.get_rank()
                buf = reward_scaler._rank_stats
                if buf is None or buf.shape[0] != world or buf.device != state.device:
                    buf = reward_scaler._rank_stats = torch.zeros(world, 6, dtype=torch.float64, device=state.device)
                buf.zero_()
                buf[rank].copy_(state[:6])
                consensus.all_reduce_small(buf)
                hip.check(L.cadre_return_scale_merge(hip.ptr(buf), world, float(reward_scaler.epsilon), hip.ptr(state), None,
                                                     hip.stream()), "cadre_return_scale_merge")
        g32 = float(np.float32(s0.gamma))
        gt32 = float(np.float32(s0.gamma * s0.tau))              # double product, then one rounding (storage.py:75)
        hip.check(L.cadre_gae_multi(hip.ptr(table), n, T, g32, gt32, 1 if normalise else 0, hip.ptr(state),
                                    float(reward_scaler.clip) if reward_scaler is not None else 0.0, hip.stream()),
                  "cadre_gae_multi")
        if explained_variance is not None:
            RolloutStorage.explained_variance(storages, explained_variance)
        return [s.advantages for s in storages]

    _mark_tables = {}

    @staticmethod
    def mark_suggestions(storages, Z, horizon):
        """After finish_rollouts / compute_returns: `suggest` of every storage of a section from its `events`, masks and
        time-limit flags in ONE launch (cadre_suggest_mark; see include/cadre_hip.h for the scan).  storages = the flat list
        [steer_0, throttle_0, ...] (storage k belongs to head k & 1); horizon = device int32 [2][Z + 1].  A storage that
        never recorded an event gets its two tensors here (all rows kind 0)."""
        n = len(storages)
        s0 = storages[0]
        if n < 1 or any((s.num_steps, s.device) != (s0.num_steps, s0.device) for s in storages):
            raise ValueError("mark_suggestions: every storage needs the same num_steps and device")
        if horizon.dtype != torch.int32 or tuple(horizon.shape) != (2, Z + 1) or not horizon.is_contiguous() or horizon.device != s0.device:
            raise ValueError("mark_suggestions: horizon must be a contiguous int32 [2][Z + 1] tensor on the storages' device")
        rows = [[hip.ptr(s._event_tensors()), hip.ptr(s.masks), hip.ptr(s.time_limits) if s._tl_used else 0, hip.ptr(s.suggest)]
                for s in storages]
        key = tuple(p for row in rows for p in row)
        tables = RolloutStorage._mark_tables
        table = tables.get(key)
        if table is None:
            if len(tables) > 16:
                tables.clear()
            table = tables[key] = torch.tensor(rows, dtype=torch.int64).to(s0.device)
        hip.check(hip.lib().cadre_suggest_mark(hip.ptr(table), n, s0.num_steps, Z, hip.ptr(horizon), hip.stream()),
                  "cadre_suggest_mark")

    _ev_tables = {}

    @staticmethod
    def explained_variance(storages, out):
        """Explained variance of the value head, 1 - Var(R - V) / Var(R) (population variances, fp64) over rows 0..T-1 of
        every storage after compute_returns, in ONE launch (cadre_explained_variance): out = device float64 [len(storages)];
        NaN where the returns are constant.  Nothing is read back on the host."""
        if not storages or out.dtype != torch.float64 or out.numel() < len(storages) or not out.is_contiguous():
            raise ValueError("explained_variance: %d storages into %s %s" % (len(storages), out.dtype, tuple(out.shape)))
        rows = [[hip.ptr(s.returns), hip.ptr(s.value_preds), s.num_steps] for s in storages]
        key = tuple(v for r in rows for v in r)
        table = RolloutStorage._ev_tables.get(key)
        if table is None:
            if len(RolloutStorage._ev_tables) > 16:
                RolloutStorage._ev_tables.clear()
            table = RolloutStorage._ev_tables[key] = torch.tensor(rows, dtype=torch.int64).to(out.device)
        hip.check(hip.lib().cadre_explained_variance(hip.ptr(table), len(storages), hip.ptr(out), hip.stream()),
                  "cadre_explained_variance")
        return out

    def get_last(self, as_tensor=False):
        """storage.py:88-91: (obs[-1], command[-1].item()).  `.item()` on a device tensor is a host sync — in the learner
        section it waits for the whole encoder pass and leaves the GPU idle while the host then enqueues the bootstrap
        values, GAE and the first minibatch (traced: 1.2-2 ms per round).  as_tensor=True returns the command as the
        0-dim device tensor instead; `CadreAgent.get_value(s)` then pick the command net on the device."""
        if as_tensor:
            return self.obs[-1], self.command[-1]
        return self.obs[-1], int(self.command[-1].item())

    def sample_indices(self):
        """BatchSampler(SubsetRandomSampler(range(T)), T // mini_batch_num, drop_last=False)
        (storage.py:94-97): ONE torch.randperm(T) from the global CPU generator."""
        T = self.num_steps
        bs = T // self.mini_batch_num
        perm = torch.randperm(T)
        return [perm[i:i + bs] for i in range(0, T, bs)]

    def gather(self, indices, advantages):
        idx = indices.to(self.device, non_blocking=True)
        B, S = idx.numel(), self.seq_length
        x = torch.empty(S * B, self._ldo, device=self.device)
        hip.check(hip.lib().cadre_gather_obs(hip.ptr(self._obs), self._ldo, S, hip.ptr(idx), B, hip.ptr(x),
                                             self._ldo, self.z_dims, hip.stream()), "cadre_gather_obs")
        hidden = [self._hn.index_select(0, idx)[:, :self.hid_size], self._cn.index_select(0, idx)[:, :self.hid_size]]
        return (x[:, :self.z_dims], self.action[idx], self.value_preds[idx], self.returns[idx], self.masks[idx],
                self.action_log_probs[idx], advantages[idx], hidden, self.command[idx])

    def feed_forward_generator(self, advantages):
        """storage.py:93-120: yields (obs [S*B,D] time-major, action, V_old, ret, mask, logp_old, adv,
        [hn, cn], command)."""
        for indices in self.sample_indices():
            yield self.gather(indices, advantages)


class ReturnScaler(object):
    """Return-based reward scaling (the VecNormalize(norm_reward=True) rule) for `n_envs` environments of two heads each:
    rewards are divided by the running standard deviation of the discounted return G_t = r_t + gamma m'_{t-1} G_{t-1},
    m' = mask (1 - time_limit), kept per head.  Everything lives in one float64 device block (layout: CADRE_RS_* of
    include/cadre_hip.h) that cadre_return_stats updates and cadre_gae_multi reads, with no host sync:
    RolloutStorage.finish_rollouts(..., reward_scaler=self).  `training` False freezes statistics, carries and scale
    (evaluation, replay).  The scaled reward is clamped to [-clip, clip]; scale = 1 / sqrt(var + epsilon)."""

    def __init__(self, n_envs, gamma, clip=10.0, epsilon=1e-8, device="cpu"):
        if isinstance(n_envs, bool) or not isinstance(n_envs, int) or not 1 <= n_envs <= 32767:
            raise ValueError("ReturnScaler: n_envs must be an integer 1 .. 32767 (got %r)" % (n_envs,))
        gamma, clip, epsilon = float(gamma), float(clip), float(epsilon)
        if not 0.0 <= gamma <= 1.0:
            raise ValueError("ReturnScaler: gamma must be in [0, 1] (got %r)" % (gamma,))
        if not 0.0 < clip < float("inf"):
            raise ValueError("ReturnScaler: clip must be a positive finite number (got %r)" % (clip,))
        if not 0.0 <= epsilon < float("inf"):
            raise ValueError("ReturnScaler: epsilon must be a finite number >= 0 (got %r)" % (epsilon,))
        self.n_envs, self.gamma, self.clip, self.epsilon = n_envs, gamma, clip, epsilon
        self.training = True
        device = torch.device(device)
        self.state = torch.zeros(hip.RS_CARRY + 4 * n_envs, dtype=torch.float64, device=device)
        self.state[hip.RS_SCALE:hip.RS_CARRY] = 1.0
        self._scratch = torch.zeros(1 + 4 * n_envs, dtype=torch.float64, device=device)
        self._rank_stats = None    # rank consensus: the [world][6] gather buffer of finish_rollouts(consensus=)

    def to(self, device):
        self.state = self.state.to(device)
        self._scratch = torch.zeros_like(self._scratch, device=device)
        return self

    def scale(self):
        """The two float32 scales (steer, throttle) the next scan multiplies rewards with."""
        return self.state[hip.RS_SCALE:hip.RS_CARRY].to(torch.float32)

    def count(self):
        return self.state[0:6:3].clone()

    def state_dict(self):
        st = self.state.detach()
        return dict(count=st[0:6:3].clone(), mean=st[1:6:3].clone(), M2=st[2:6:3].clone(), scale=self.scale().clone(),
                    carry=st[hip.RS_CARRY:].view(2 * self.n_envs, 2).clone())

    def load_state_dict(self, sd):
        missing = sorted({"count", "mean", "M2", "scale", "carry"} - set(sd))
        if missing:
            raise ValueError("ReturnScaler.load_state_dict: missing %r" % (missing,))
        if tuple(sd["carry"].shape) != (2 * self.n_envs, 2) or any(sd[k].numel() != 2 for k in ("count", "mean", "M2", "scale")):
            raise ValueError("ReturnScaler.load_state_dict: a state for %d environments does not fit %d"
                             % (sd["carry"].shape[0] // 2, self.n_envs))
        for i, k in enumerate(("count", "mean", "M2")):
            self.state[i:6:3] = sd[k].to(self.state.device, torch.float64)
        self.state[hip.RS_SCALE:hip.RS_CARRY] = sd["scale"].to(self.state.device, torch.float32).double()
        self.state[hip.RS_CARRY:] = sd["carry"].to(self.state.device, torch.float64).reshape(-1)
