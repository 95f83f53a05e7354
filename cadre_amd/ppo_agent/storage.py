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

    def __init__(self, num_steps, mini_batch_num, feature_dims, seq_length, hidden_size, use_gae, gamma, tau):
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
        self._ldo = _rup(feature_dims, PAD)
        self._ldh = _rup(hidden_size, PAD)
        self._alloc(torch.device("cpu"))

    def _alloc(self, device):
        T = self.num_steps
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=device)
        self.device = device
        self._obs = z(T + 1, self.seq_length, self._ldo)
        self._hn = z(T + 1, self._ldh)
        self._cn = z(T + 1, self._ldh)
        self.obs = self._obs[:, :, :self.z_dims]
        self.hn = self._hn[:, :self.hid_size]
        self.cn = self._cn[:, :self.hid_size]
        self.command = z(T + 1, 1, dtype=torch.int)
        self.rewards = z(T + 1, 1)
        self.value_preds = z(T + 1, 1)
        self.returns = z(T + 1, 1)
        self.action_log_probs = z(T + 1, 1)
        self.action = z(T + 1, 1, dtype=torch.long)
        self.masks = z(T + 1, 1)
        self.advantages = z(T, 1)            # filled by compute_returns (train.py:82-88)
        self._next = z(1)

    def to(self, device):
        device = torch.device(device)
        old = {k: getattr(self, k) for k in ("_obs", "_hn", "_cn", "command", "rewards", "value_preds", "returns",
                                             "action_log_probs", "action", "masks", "advantages")}
        self._alloc(device)
        for k, v in old.items():
            getattr(self, k).copy_(v)

    def insert(self, obs, action, action_log_probs, value_preds, rewards, masks, hidden_state, command):
        """storage.py:45-58."""
        s = self.step
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
    def insert_batch(storages, outputs, rewards, masks, commands):
        """`insert` (storage.py:45-58) of one env step of N environments into their 2N storages in ONE launch
        (cadre_insert_rows): storages = [(steer_rollout, throttle_rollout), ...] per environment, outputs = what
        CadreAgent.act_batch returned for them, rewards / masks = [N][2] (steer, throttle) host values, commands = the N
        host-side commands.  The hidden state written is act()'s zeros.  The cursors (and their modulo-(T+1) drift) stay
        host-side ints, exactly as `insert` keeps them."""
        N = len(storages)
        if N < 1 or len(outputs) != N or len(rewards) != N or len(masks) != N or len(commands) != N:
            raise ValueError("insert_batch: %d storage pairs, %d outputs, %d rewards, %d masks, %d commands"
                             % (N, len(outputs), len(rewards), len(masks), len(commands)))
        flat = [s for pair in storages for s in pair]
        if len(flat) != 2 * N:
            raise ValueError("insert_batch: storages must be (steer, throttle) pairs")
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
        ptrs = [[hip.ptr(s._obs), hip.ptr(s._hn), hip.ptr(s._cn), hip.ptr(s.action), hip.ptr(s.action_log_probs),
                 hip.ptr(s.value_preds), hip.ptr(s.rewards), hip.ptr(s.masks), hip.ptr(s.command)] for s in flat]
        key = tuple(p for row in ptrs for p in row)
        tables = RolloutStorage._insert_tables
        table = tables.get(key)
        if table is None:
            if len(tables) > 16:
                tables.clear()
            table = tables[key] = torch.tensor(ptrs, dtype=torch.int64).to(dev)
        slots = [s.step for s in flat]
        ints = torch.tensor(slots + [int(c) for c in commands], dtype=torch.int32).to(dev)
        rm = torch.tensor([[float(rewards[e][h]), float(torch.as_tensor(masks[e][h]).reshape(-1)[0])]
                           for e in range(N) for h in (0, 1)], dtype=torch.float32).to(dev)
        hip.check(hip.lib().cadre_insert_rows(hip.ptr(table), hip.ptr(ints), 2 * N, s0.seq_length, s0._ldo, s0._ldh,
                                              s0.z_dims, s0.hid_size, s0.num_steps, hip.ptr(feat), feat.stride(1),
                                              hip.ptr(action), hip.ptr(logp), hip.ptr(value), hip.ptr(rm),
                                              hip.ptr(ints[2 * N:]), hip.stream()), "cadre_insert_rows")
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
