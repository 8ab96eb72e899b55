"""Training-mode layers on the device: ``litepose_amd.nn.functional``."""
from . import functional  # noqa: F401
