"""Drop-in for the part of ``dataset`` (reference lib/dataset) the architecture search reads: the ``calibrate`` split's
image side, resident on the device (``calibration.CalibrationSet``)."""
from .calibration import CalibrationSet, draw_transform  # noqa: F401
