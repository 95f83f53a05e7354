"""Sample reuse (cadre_amd/reuse.py) on the `ppo_agent` import path: ReuseWindow / reuse_config / reuse_runner."""
from ..reuse import (DIAG_FIELDS, REUSE_KEYS, ReuseRunner, ReuseWindow, reuse_config, reuse_permutation,  # noqa: F401
                     reuse_runner, reuse_stats_text)
