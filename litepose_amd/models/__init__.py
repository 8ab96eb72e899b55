from . import pose_mobilenet  # noqa: F401
from . import pose_simplenet  # noqa: F401
from . import pose_resnet  # noqa: F401
from . import pose_supermobilenet  # noqa: F401
