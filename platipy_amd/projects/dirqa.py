"""The reference's DIR QA service (services/dirqa/service.py) as a function of Images: platipy_amd/registration/qa.py holds it."""
from ..registration.qa import DIRQA_SETTINGS_DEFAULTS, PointTable, dir_qa  # noqa: F401
