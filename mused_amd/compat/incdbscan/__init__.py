"""`from incdbscan import IncrementalDBSCAN` (main.py:11) under the drop-in path: the device class of mused_amd/incdbscan.py."""
from mused_amd.incdbscan import IncrementalDBSCAN  # noqa: F401

__all__ = ["IncrementalDBSCAN"]
