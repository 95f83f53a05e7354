"""Cost constraints (cadre_amd/constraint.py) on the `ppo_agent` import path: the module / constraint_config / the helpers."""
from ..constraint import (CONSTRAINT_KEYS, CostConstraint, constraint_config, constraint_refusals, constraint_runner,  # noqa: F401
                          constraint_stats_text, cost_from_message, cost_pair, cost_tower_offsets, costs_of, init_cost_tower)
