from .metrics import (calculate_ap, calculate_iou, calculate_iou_batch, evaluate_detections,
                      evaluate_detections_per_class, evaluate_packed, evaluate_packed_cls)

__all__ = ["evaluate_detections", "evaluate_packed", "calculate_ap", "calculate_iou", "calculate_iou_batch",
           "evaluate_detections_per_class", "evaluate_packed_cls"]
