"""Weight averaging (cadre_amd/average.py) on the `ppo_agent` import path: the module / average_config / soup / the helpers."""
from ..average import (AVERAGE_KEYS, WeightAverage, average_config, average_refusals, average_runner,  # noqa: F401
                       average_stats_text, averaged_weights, check_soup_layouts, check_soup_weights, soup, warmup_decay)
