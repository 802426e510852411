from .base_evaluator import Evaluator  # noqa: F401
from .make_evaluator import make_evaluator  # noqa: F401
