"""Drop-in for the reference's real-time demo parser, ``nano_demo/fast_utils`` (``fast_utils.group.HeatmapParser``):
find_peaks + assign on the device (lp_fast_parse), no adjust and no refine."""
from . import group  # noqa: F401
from .group import HeatmapParser, Params  # noqa: F401
