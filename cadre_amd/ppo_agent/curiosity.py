"""Curiosity bonus (cadre_amd/curiosity.py) on the `ppo_agent` import path: the module / curiosity_config / the helpers."""
from ..curiosity import (CURIOSITY_KEYS, Curiosity, curiosity_config, curiosity_refusals, curiosity_runner,  # noqa: F401
                         curiosity_stats_text, init_tower, mask_threshold, tower_offsets)
