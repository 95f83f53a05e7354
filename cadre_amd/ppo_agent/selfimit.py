"""Self-imitation learning (cadre_amd/selfimit.py) on the `ppo_agent` import path: the buffer / sil_config / the helpers."""
from ..selfimit import (SIL_KEYS, STATS_FIELDS, TAILS, SelfImitationBuffer, SilRunner, sil_config, sil_runner,  # noqa: F401
                        sil_stats_text, sil_words)
