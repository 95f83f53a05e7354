from cadre_amd.ppo_agent.constraint import *  # noqa: F401,F403
from cadre_amd.ppo_agent import constraint as _m
globals().update({k: v for k, v in vars(_m).items() if not k.startswith('__')})
