"""The TasNet example (examples/tasnet): the evaluation data pipeline and `eval`.  Training and `preprocess.py` are not built."""
from .data import DatasetGenerator  # noqa: F401
