"""The decoder branches (cadre_amd/decoder.py) on the `ppo_agent` import path."""
from ..decoder import (Decoded, DANetDecoderHIP, has_decoder)  # noqa: F401
