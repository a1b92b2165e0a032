"""Drop-in for platipy/imaging/utils: crop.py, geometry.py, vessel.py, valve.py, conduction.py."""
from . import conduction, crop, geometry, valve, vessel  # noqa: F401
