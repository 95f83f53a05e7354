"""Exploration suggestions (cadre_amd/suggest.py) on the `ppo_agent` import path: Suggestions / suggest_config / the helpers."""
from ..suggest import (MESSAGE_EVENTS, STANDARD_EVENTS, SUGGEST_KEYS, Suggestions, events_from_message, log_prior,  # noqa: F401
                       peaked_prior, suggest_config, suggest_runner, suggest_stats_text, uniform_prior)
