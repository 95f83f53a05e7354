"""Frame-table storages: every distinct frame row once, windows as frame ids.

A RolloutStorage keeps its windows materialised: S = 8 frames x `_ldo` floats per transition, seven of them copies of the
transition before (the window slides).  A `FrameStorage` holds `_frames` float32 [F_cap, _ldo] and `_win` int32 [T + 1, S]
in place of `_obs`; the minibatch gathers read `frames + win[t, s] * ldo` where they read `obs + (t * S + s) * ldo`
(csrc/frame_table.hip), so everything behind the gather sees the same bits.

Who builds one: `DemoSet.from_episodes(..., frame_table=True)` (a record holds frames and window indices already) and
`AuxBuffer(..., frames_per_row=)` (materialised rollouts packed by scan_frames / copy_frames: cadre_frames_scan, cadre_frames_copy).
Live rollouts stay materialised: `insert` gets no frame identity.
"""
import math

import torch

from . import hip
from .ppo_agent.storage import RolloutStorage

MAX_S = 16            # windows of at most 16 frames (cadre_frames_scan)


def frames_per_row_ok(v, S=None):
    """A finite number in [1 / S, S] (S None: the widest window the kernels take, MAX_S)."""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
        return False
    S = MAX_S if S is None else int(S)
    return 1.0 / S <= float(v) <= float(S)


def capacity_for(rows, frames_per_row, S):
    """Frames of a buffer of `rows` window rows at `frames_per_row`: ceil(rows * frames_per_row)."""
    if not frames_per_row_ok(frames_per_row, S):
        raise ValueError("frames_per_row must be a finite number in [1/S, S] = [%g, %d] (got %r): a window row holds S frames, "
                         "of which S - 1 are usually the row before's" % (1.0 / S, S, frames_per_row))
    return int(math.ceil(int(rows) * float(frames_per_row)))


class FrameStorage(RolloutStorage):
    """A RolloutStorage (same fields, same geometry: `_ldo`, `seq_length`, `_ldh`, `z_dims`) whose window rows are
    `_frames` float32 [F_cap, _ldo] (rows [0, n_frames) are in use; pad columns zero) and `_win` int32 [T + 1, S] (the frame
    id of every window row; -1: none, which gathers as NaN).  `_obs` is None; `obs` materialises [T + 1, S, D] through
    cadre_gather_obs_ft on every access — for tests and debugging.  Two FrameStorages may share `_frames` and `_win` (the two
    heads see the same windows), and sets cut from one another share `_frames`."""

    def __init__(self, num_steps, mini_batch_num, feature_dims, seq_length, hidden_size, use_gae, gamma, tau, device="cpu",
                 frames=None, win=None, n_frames=None, frame_capacity=None):
        """frames / win: existing tensors to stand on (shared, not copied); else `frame_capacity` zero rows are allocated
        and every window id starts at -1."""
        if frames is None and (isinstance(frame_capacity, bool) or not isinstance(frame_capacity, int) or frame_capacity < 1):
            raise ValueError("FrameStorage: needs `frames` or a frame_capacity >= 1 (got %r)" % (frame_capacity,))
        self._given = (frames, win)
        self._cap = int(frames.shape[0]) if frames is not None else int(frame_capacity)
        RolloutStorage.__init__(self, num_steps, mini_batch_num, feature_dims, seq_length, hidden_size, use_gae, gamma, tau,
                                device=device)
        self.n_frames = int(n_frames) if n_frames is not None else (self._cap if frames is not None else 0)
        if not 0 <= self.n_frames <= self._cap:
            raise ValueError("FrameStorage: n_frames=%r for %d frame rows" % (n_frames, self._cap))

    def _alloc_obs(self, device):
        frames, win = self._given
        self._given = (None, None)
        T, S = self.num_steps, self.seq_length
        if frames is None:
            frames = torch.zeros(self._cap, self._ldo, dtype=torch.float32, device=device)
        if win is None:
            win = torch.full((T + 1, S), -1, dtype=torch.int32, device=device)
        if frames.dtype != torch.float32 or frames.dim() != 2 or frames.shape[1] != self._ldo or not frames.is_contiguous():
            raise ValueError("FrameStorage: frames must be a contiguous float32 [F, %d] tensor (got %s %s)"
                             % (self._ldo, frames.dtype, tuple(frames.shape)))
        if win.dtype != torch.int32 or tuple(win.shape) != (T + 1, S) or not win.is_contiguous():
            raise ValueError("FrameStorage: win must be a contiguous int32 [%d, %d] tensor (got %s %s)"
                             % (T + 1, S, win.dtype, tuple(win.shape)))
        if frames.device != win.device or frames.device.type != device.type:
            raise ValueError("FrameStorage: frames on %s, win on %s, the storage on %s" % (frames.device, win.device, device))
        self._obs = None
        self._frames, self._win = frames, win

    def to(self, device):
        """Moves the frames and the window ids with everything else (a pair that shared them shares them no longer, as two
        RolloutStorages that shared `_obs`)."""
        device = torch.device(device)
        self._given = (self._frames.to(device), self._win.to(device))
        old = {k: getattr(self, k) for k in ("_hn", "_cn", "command", "rewards", "value_preds", "returns", "action_log_probs",
                                             "action", "masks", "advantages", "time_limits")}
        self._alloc(device)
        for k, v in old.items():
            getattr(self, k).copy_(v)
        if getattr(self, "events", None) is not None:
            self.events, self.suggest = self.events.to(device), self.suggest.to(device)

    def _gather_obs(self, idx, ldx):
        """Window rows idx (device int64 [B]) -> time-major [S * B, ldx] (cadre_gather_obs_ft)."""
        B, S = idx.numel(), self.seq_length
        x = torch.empty(S * B, ldx, device=self.device)
        hip.check(hip.lib().cadre_gather_obs_ft(hip.ptr(self._frames), hip.ptr(self._win), self.n_frames, self._ldo, S,
                                                hip.ptr(idx), B, hip.ptr(x), ldx, self.z_dims, hip.stream()),
                  "cadre_gather_obs_ft")
        return x

    @property
    def obs(self):
        T, S = self.num_steps, self.seq_length
        x = self._gather_obs(torch.arange(T + 1, device=self.device), self._ldo)          # [S][T + 1][ldo]
        return x.view(S, T + 1, self._ldo).permute(1, 0, 2)[:, :, :self.z_dims]

    def insert(self, *args, **kwargs):
        raise ValueError("FrameStorage.insert: a frame-table storage is not filled row by row (insert gets no frame identity); "
                         "DemoSet.from_episodes(frame_table=True) and AuxBuffer(frames_per_row=) build one")

    # (insert_batch is a static method of RolloutStorage: it refuses a FrameStorage among its storages itself)

    def get_last(self, as_tensor=False):
        raise ValueError("FrameStorage.get_last: a frame-table storage holds finished rows, not a rollout in progress")

    def gather(self, indices, advantages):
        idx = indices.to(self.device, non_blocking=True)
        x = self._gather_obs(idx, self._ldo)
        hidden = [self._hn.index_select(0, idx)[:, :self.hid_size], self._cn.index_select(0, idx)[:, :self.hid_size]]
        return (x[:, :self.z_dims], self.action[idx], self.value_preds[idx], self.returns[idx], self.masks[idx],
                self.action_log_probs[idx], advantages[idx], hidden, self.command[idx])

    def frame_bytes(self):
        """Device bytes of the window rows in this form: the frames and the ids."""
        return self._frames.numel() * 4 + self._win.numel() * 4


def frame_pair(T, feature_dims, seq_length, hidden_size, gamma, device, frames=None, win=None, n_frames=None,
               frame_capacity=None):
    """(steer, throttle) FrameStorages of T rows that share `_frames` and `_win` (DemoSet._storages in this form)."""
    steer = FrameStorage(T, 1, feature_dims, seq_length, hidden_size, True, gamma, 1.0, device=device, frames=frames, win=win,
                         n_frames=n_frames, frame_capacity=frame_capacity)
    throttle = FrameStorage(T, 1, feature_dims, seq_length, hidden_size, True, gamma, 1.0, device=device, frames=steer._frames,
                            win=steer._win, n_frames=steer.n_frames)
    return steer, throttle


def scan_frames(obs_list, P, S, ldo, D):
    """cadre_frames_scan over rows [0, P) of the materialised `obs_list` (device float32 tensors of pitch ldo, one per
    storage) -> (pointer table, flags, win_local int32 [n][P][S], count int32 [n]), all on the device."""
    n, dev = len(obs_list), obs_list[0].device
    table = torch.tensor([hip.ptr(o) for o in obs_list], dtype=torch.int64).to(dev)
    flags = torch.empty(n, P, S, dtype=torch.int32, device=dev)
    win_local = torch.empty(n, P, S, dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    hip.check(hip.lib().cadre_frames_scan(hip.ptr(table), n, P, S, ldo, D, hip.ptr(flags), hip.ptr(win_local), hip.ptr(count),
                                          hip.stream()), "cadre_frames_scan")
    return table, flags, win_local, count


def copy_frames(scan, P, S, ldo, D, base, frames, win_dst, row0):
    """cadre_frames_copy of a scan_frames result: new rows to frames[base[z] + id], global ids to win_dst rows row0[z] ..
    (base, row0: host int lists)."""
    table, flags, win_local, _count = scan
    n, dev = flags.shape[0], flags.device
    br = torch.tensor([list(base), list(row0)], dtype=torch.int32).to(dev)
    hip.check(hip.lib().cadre_frames_copy(hip.ptr(table), n, P, S, ldo, D, hip.ptr(flags), hip.ptr(win_local), hip.ptr(br[0]),
                                          hip.ptr(frames), frames.stride(0), frames.shape[0], hip.ptr(win_dst), hip.ptr(br[1]),
                                          hip.stream()), "cadre_frames_copy")
