"""Same names as the reference's R/csv_eval.py (compute_overlap, _compute_ap, evaluate), on the device.  See
retinanet_mi355x/csv_eval.py."""
from retinanet_mi355x.csv_eval import (compute_overlap, _compute_ap, _get_annotations, evaluate,  # noqa: F401
                                       evaluate_detections)
