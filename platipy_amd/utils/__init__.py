"""Drop-in for platipy/imaging/utils: crop.py, geometry.py, vessel.py, valve.py, conduction.py, lung.py, ventricle.py."""
from . import conduction, crop, geometry, lung, valve, ventricle, vessel  # noqa: F401
from .ventricle import generate_left_ventricle_segments  # noqa: F401
