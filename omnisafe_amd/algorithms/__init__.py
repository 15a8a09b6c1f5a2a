"""Accelerated on-policy algorithms; same names as the reference's registry entries."""
from . import registry
from .policy_gradient import PPO, PolicyGradient, PPOLag
from .trust_region_algos import CPO, TRPO, NaturalPG, TRPOLag
from .siblings import (CPPOPID, CUP, FOCOPS, IPO, P3O, PCPO, PDO, RCPO, TRPOPID, OnCRPO, PPOSaute,
                       PPOSimmerPID, TRPOSaute, TRPOSimmerPID)

ALGORITHMS = {'on-policy': tuple(sorted(registry.REGISTRY._module_dict))}  # noqa: SLF001
from .offline import BCQ, CCRR, CRR, VAEBC, BCQLag, COptiDICE  # noqa: E402  (after the on-policy tuple: the registry holds every family)

from .off_policy import DDPG, DDPGPID, SAC, TD3, TD3PID, DDPGLag, TD3Lag  # noqa: E402

ALGORITHMS['offline'] = ('CCRR', 'CRR')
ALGORITHMS['offline-bc'] = ('VAEBC',)
ALGORITHMS['offline-dice'] = ('COptiDICE',)
ALGORITHMS['offline-bcq'] = ('BCQ', 'BCQLag')
ALGORITHMS['off-policy'] = ('DDPG', 'TD3')
ALGORITHMS['off-policy-sac'] = ('SAC',)
ALGORITHMS['off-policy-lag'] = ('DDPGLag', 'DDPGPID', 'TD3Lag', 'TD3PID')
__all__ = ['DDPG', 'TD3', 'SAC', 'DDPGLag', 'TD3Lag', 'DDPGPID', 'TD3PID', 'CRR', 'CCRR', 'VAEBC', 'BCQ', 'BCQLag', 'COptiDICE', 'PolicyGradient', 'PPO', 'PPOLag', 'NaturalPG', 'TRPO', 'TRPOLag', 'CPO', 'PDO', 'RCPO', 'IPO',
           'OnCRPO', 'CPPOPID', 'TRPOPID', 'PCPO', 'FOCOPS', 'CUP', 'P3O', 'PPOSaute', 'TRPOSaute',
           'PPOSimmerPID', 'TRPOSimmerPID', 'registry', 'ALGORITHMS']
