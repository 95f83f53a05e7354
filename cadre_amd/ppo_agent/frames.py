"""Frame-table storages (cadre_amd/frames.py) on the `ppo_agent` import path: FrameStorage and the packing helpers."""
from ..frames import (MAX_S, FrameStorage, capacity_for, copy_frames, frame_pair, frames_per_row_ok,  # noqa: F401
                      scan_frames)
