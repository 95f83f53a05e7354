"""Temporal action smoothness (cadre_amd/smooth.py) on the `ppo_agent` import path: the runner / smooth_config / the helpers."""
from ..smooth import (SMOOTH_KEYS, STATS_FIELDS, Smoothness, control_values, smooth_config, smooth_runner,  # noqa: F401
                      smooth_stats_text, smooth_tables, smooth_worker, successor_index)
