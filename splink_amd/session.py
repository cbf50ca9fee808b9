"""AmdSession: the `spark` argument of the reference API, pointing at a GPU instead.

The reference detects the jar's UDF by name in `spark.catalog.listFunctions()`
(case_statements.py:12-14) to choose Jaro-Winkler defaults.  On an AmdSession the string
comparison functions are native gfx950 kernels, so `jaro_winkler_sim` is always listed.
Passing None or 'supress_warnings' keeps the reference's behaviour for those values
(equality / Levenshtein defaults).
"""
from collections import namedtuple

from .engine import default_device

Function = namedtuple("Function", ["name", "description", "className", "isTemporary"])

NATIVE_FUNCTIONS = ("jaro_winkler_sim", "jaccard_sim", "cosine_distance", "levenshtein", "length", "substr", "ifnull",
                    "abs")


class _Catalog:
    def listFunctions(self):  # noqa: N802 (Spark name)
        return [Function(n, "gfx950 kernel in libsplink_hip.so", "splink_amd", True) for n in NATIVE_FUNCTIONS]


class AmdSession:
    """Device handle accepted wherever the reference takes a SparkSession."""

    def __init__(self, device: int = None):
        self.device = default_device() if device is None else int(device)
        self.catalog = _Catalog()

    def __repr__(self):
        return f"AmdSession(device={self.device})"


def session(device: int = None) -> AmdSession:
    return AmdSession(device)
