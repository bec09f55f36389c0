"""Validation of the directional detector in 3D (cuboid AP, corner errors) beside the drop-in's csv_eval: the reference
has no such module.  See retinanet_mi355x/eval3d.py."""
from retinanet_mi355x.eval3d import evaluate_3d, evaluate_cuboids, split_labels, validator  # noqa: F401
