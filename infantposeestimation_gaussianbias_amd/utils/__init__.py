"""Utils module."""
from .metrics import (AverageMeter, COCOEvaluator, KeypointErrorAnalyzer, MetricLogger, PCKAccumulator, calculate_movement_amplitude,
                      calculate_pck, calculate_temporal_consistency, keypoint_error_report, movement_heatmap, movement_report,
                      movement_spectrum)
from . import kinematics
from .kinematics import COCO_ANGLES, joint_angle_series, kinematics_report, limb_coordination, sample_entropy
from . import activations
from .activations import ActivationAnalyzer, ActivationCollector, activation_report
from . import feature_maps
from .feature_maps import (FeatureCollector, FeatureVisualizer, HeatmapQualityAccumulator, feature_sheet, heatmap_quality,
                           heatmap_quality_sheet)
from . import postprocess
from .postprocess import oks_nms, soft_oks_nms
from . import sensitivity
from .sensitivity import GradCAMVisualizer, GradientCollector, SensitivityAnalyzer, attribution_maps, occlusion_sensitivity_maps
from . import tensor_stats
from .tensor_stats import gradient_flow, gradient_statistics, tensor_statistics, weight_statistics
from . import uncertainty
from .uncertainty import UncertaintyAnalyzer, mc_uncertainty
from . import visualization
from .visualization import (COCO_COLORS, COCO_SKELETON, create_grid_image, draw_bbox, draw_heatmaps, draw_person_heatmaps, draw_poses,
                            draw_skeleton, save_person_visualization, save_visualization)

__all__ = ['AverageMeter', 'COCOEvaluator', 'MetricLogger', 'postprocess', 'visualization', 'draw_skeleton', 'draw_heatmaps', 'draw_bbox',
           'draw_poses', 'draw_person_heatmaps', 'create_grid_image', 'save_visualization', 'save_person_visualization', 'COCO_SKELETON',
           'COCO_COLORS', 'PCKAccumulator', 'calculate_movement_amplitude', 'calculate_pck', 'calculate_temporal_consistency',
           'movement_heatmap', 'movement_report', 'movement_spectrum', 'oks_nms', 'soft_oks_nms', 'tensor_stats', 'tensor_statistics',
           'gradient_statistics', 'gradient_flow', 'weight_statistics', 'KeypointErrorAnalyzer',
           'keypoint_error_report', 'sensitivity', 'SensitivityAnalyzer', 'occlusion_sensitivity_maps', 'activations',
           'ActivationAnalyzer', 'ActivationCollector', 'activation_report', 'uncertainty', 'UncertaintyAnalyzer', 'mc_uncertainty',
           'attribution_maps', 'GradCAMVisualizer', 'GradientCollector', 'feature_maps', 'FeatureCollector', 'FeatureVisualizer',
           'HeatmapQualityAccumulator', 'feature_sheet', 'heatmap_quality', 'heatmap_quality_sheet', 'kinematics', 'COCO_ANGLES',
           'joint_angle_series', 'kinematics_report', 'limb_coordination', 'sample_entropy']
