from . import multiatlas  # noqa: F401
from . import cardiac  # noqa: F401
from . import bronchus  # noqa: F401
from .bronchus import BRONCHUS_SETTINGS_DEFAULTS, run_bronchus_segmentation  # noqa: F401
