"""Action masks (cadre_amd/actmask.py) on the `ppo_agent` import path: ActionMasks / actmask_config / the helpers."""
from ..actmask import (ACTMASK_KEYS, ActionMasks, actmask_config, actmask_runner, actmask_stats_text, all_word,  # noqa: F401
                       allowed_from_controls, allowed_word, check_composition, check_word, word_i64, word_pair, words_tensor)
