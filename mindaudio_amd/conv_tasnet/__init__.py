"""The Conv-TasNet example (examples/conv_tasnet): the evaluation data pipeline and `eval`.  Training and `preprocess.py` are not
built."""
from .data import DatasetGenerator  # noqa: F401
