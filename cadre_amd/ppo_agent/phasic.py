"""PPG auxiliary phase (cadre_amd/phasic.py) on the `ppo_agent` import path: AuxBuffer / aux_phase / aux_config."""
from ..phasic import (AUX_KEYS, AuxBuffer, AuxRunner, aux_config, aux_line, aux_phase, aux_runner,  # noqa: F401
                      aux_summary_line, check_intervals, epoch_permutation, record_starts, slot_rows)
