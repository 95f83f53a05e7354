"""numpy statement of the frame scan (cadre_frames_scan, include/cadre_hip.h) and of a window-row gather from frames.

Rows are compared as 32-bit patterns over columns 0 .. D-1 only: the pad is ignored, -0.0 differs from +0.0, identical NaN
bits are equal.  For window row (t, s) of a storage, in (t, s) order:
    1. t > 0, s < S - 1 and row (t, s) == row (t - 1, s + 1): flag 1, the id of that row (the window slid)
    2. else s > 0 and row (t, s) == row (t, s - 1):            flag 2, the id of that row (a reset filled the window)
    3. else:                                                   flag 0, a new frame: id = new rows before it
"""
import numpy as np

NEW, SLIDE, FILL = 0, 1, 2


def _bits(obs, D):
    a = np.ascontiguousarray(np.asarray(obs, dtype=np.float32)[..., :D])
    return a.view(np.uint32)


def scan(obs, D):
    """obs float32 [P][S][>= D] -> (flags int32 [P][S], ids int32 [P][S], count)."""
    b = _bits(obs, D)
    P, S = b.shape[:2]
    flags = np.zeros((P, S), np.int32)
    ids = np.zeros((P, S), np.int32)
    count = 0
    for t in range(P):
        for s in range(S):
            if t > 0 and s < S - 1 and np.array_equal(b[t, s], b[t - 1, s + 1]):
                flags[t, s], ids[t, s] = SLIDE, ids[t - 1, s + 1]
            elif s > 0 and np.array_equal(b[t, s], b[t, s - 1]):
                flags[t, s], ids[t, s] = FILL, ids[t, s - 1]
            else:
                flags[t, s], ids[t, s] = NEW, count
                count += 1
    return flags, ids, count


def pack(obs, D, ld):
    """(frames float32 [count][ld] — columns < D as they are, zeros up to ld —, ids [P][S]) of one storage."""
    flags, ids, count = scan(obs, D)
    frames = np.zeros((count, ld), np.float32)
    src = np.asarray(obs, dtype=np.float32)
    fb = frames.view(np.uint32)
    fb[ids[flags == NEW], :D] = _bits(src, D)[flags == NEW]
    return frames, ids


def materialise(frames, win, D):
    """Window rows [P][S][D] from frames [F][>= D] and ids [P][S]; an id outside [0, F) gives NaN."""
    frames = np.asarray(frames, dtype=np.float32)
    win = np.asarray(win)
    out = np.full(win.shape + (D,), np.nan, np.float32)
    ok = (win >= 0) & (win < frames.shape[0])
    out.view(np.uint32)[ok] = _bits(frames, D)[win[ok]]
    return out


def sliding_obs(P, S, D, ld, rng, resets=(), pad_garbage=False):
    """A materialised storage [P][S][ld] of a sliding window over fresh random frames: row 0 is a reset fill (one frame S
    times), every row in `resets` too; every other row drops its oldest frame and appends a new one."""
    obs = np.zeros((P, S, ld), np.float32)
    for t in range(P):
        new = rng.standard_normal(D).astype(np.float32)
        if t == 0 or t in resets:
            obs[t, :, :D] = new
        else:
            obs[t, :S - 1, :D] = obs[t - 1, 1:, :D]
            obs[t, S - 1, :D] = new
    if pad_garbage and ld > D:
        obs[:, :, D:] = rng.standard_normal((P, S, ld - D)).astype(np.float32)
    return obs
