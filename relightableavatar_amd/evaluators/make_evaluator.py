"""make_evaluator(cfg): lib/evaluators/make_evaluator.py:4-14."""
import importlib

from .. import config


def make_evaluator(cfg):
    if cfg.get('skip_eval', False):
        return None
    config.check_supported(cfg)
    config.set_active_cfg(cfg)
    return importlib.import_module(cfg.get('evaluator_module', 'relightableavatar_amd.evaluators.base_evaluator')).Evaluator()
