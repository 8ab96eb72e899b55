"""Drop-in for the part of ``dataset`` (reference lib/dataset) that runs on the device: the ``calibrate`` split's image
side (``calibration.CalibrationSet``) and the labelled train loader -- images, heatmaps, masks, joints
(``targets.LabelledSet``)."""
from .calibration import CalibrationSet, draw_sample, draw_transform  # noqa: F401
from .targets import LabelledSet, gaussian_table, get_joints  # noqa: F401
