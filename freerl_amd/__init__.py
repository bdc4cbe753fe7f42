"""freerl_amd — MI355X-native replay-sample + batched-update engine behind FreeRL's class surface.

The hot path of FreeRL's DQN / DDPG / TD3 / SAC / PPO / MADDPG / MASAC / MAPPO / IPPO / HAPPO scripts (`Buffer.sample` ->
`Agent.learn` -> soft update, plus `select_action` and PPO's GAE) runs in hand-written HIP
kernels for gfx950 behind the C ABI of `include/freerl_hip.h`.  This package is the
reference-side binding: same class names, constructor arguments, method signatures and
checkpoint layout as the reference scripts, no CPU fallback.  A class is imported from its module, named like the reference's script
(`from freerl_amd.MASAC import MASAC`, `from freerl_amd.SAC import SAC`, ...): module and class share the name, so the package does not
re-export the classes.
"""
from . import _native  # noqa: F401

__all__ = ["_native"]
