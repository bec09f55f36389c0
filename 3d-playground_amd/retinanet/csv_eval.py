"""Same names as the reference's D/csv_eval.py (compute_overlap, _compute_ap, evaluate), on the device; evaluate reads
the directional model's [K,20] rows through box_cols=(16, 20) by default.  See retinanet_mi355x/csv_eval.py."""
from retinanet_mi355x.csv_eval import (compute_overlap, _compute_ap, _get_annotations, evaluate,  # noqa: F401
                                       evaluate_detections)
