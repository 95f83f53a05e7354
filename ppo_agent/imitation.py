from cadre_amd.imitation import *  # noqa: F401,F403
from cadre_amd import imitation as _m
globals().update({k: v for k, v in vars(_m).items() if not k.startswith('__')})
