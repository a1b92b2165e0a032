"""Drop-in for platipy/imaging/utils: crop.py, geometry.py, vessel.py, valve.py, conduction.py, lung.py."""
from . import conduction, crop, geometry, lung, valve, vessel  # noqa: F401
