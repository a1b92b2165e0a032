"""Drop-in for platipy/imaging/dose/: dose-volume histograms (dvh) and dose metrics (metric) of structures on a dose grid."""
from . import dvh, metric  # noqa: F401
from .dvh import (  # noqa: F401
    calculate_d_cc_x, calculate_d_x, calculate_dvh, calculate_dvh_for_labels, calculate_v_x, dvh_table)
from .metric import (  # noqa: F401
    calculate_d_max, calculate_d_mean, calculate_d_to_volume, calculate_d_to_volume_for_labels, calculate_v_receiving_dose,
    calculate_v_receiving_dose_for_labels)
