"""Training checkpoints (cadre_amd/checkpoint.py) on the `ppo_agent` import path: capture / Capture / load / restore."""
from ..checkpoint import FORMAT_VERSION, Capture, capture, load, reference_digest, restore, write_state  # noqa: F401
