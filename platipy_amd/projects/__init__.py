from . import multiatlas  # noqa: F401
from . import cardiac  # noqa: F401
from . import bronchus  # noqa: F401
from .bronchus import BRONCHUS_SETTINGS_DEFAULTS, run_bronchus_segmentation  # noqa: F401
from . import dirqa  # noqa: F401
from .dirqa import DIRQA_SETTINGS_DEFAULTS, dir_qa  # noqa: F401
