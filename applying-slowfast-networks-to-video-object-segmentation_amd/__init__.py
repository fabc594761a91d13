"""sfvos_amd -- MI355X-native SlowFastLayers hot path (hand-written HIP behind a C ABI).

Public surface mirrors the reference's `helpers/model.py` for this path:
    SlowFastLayers(input_size, device, slow_pathway_size, fast_pathway_size)
plus the pieces the reference's train.py builds around it (SGD step, gradient averaging for
one-process-per-GPU data parallelism)."""
from .plan import SlowFastPlan, calc_fuse_kernel_size, calc_kernel_sizes, davis_pyramid  # noqa: F401
from .module import PackedClip, SlowFastLayers, union_mask  # noqa: F401
from .optim import FusedSGD  # noqa: F401
from .losses import MSEProxyLoss  # noqa: F401
from .stream import SlowFastStream  # noqa: F401
from .windows import SlowFastWindows  # noqa: F401
from .mask_head import (MaskBranch, MaskRCNNHeads, MaskRCNNPredictor, maskrcnn_inference,  # noqa: F401
                        maskrcnn_loss, paste_masks_in_image)
from .box_head import (BoxBranch, FastRCNNPredictor, RoIHeadsInference, TwoMLPHead, decode_boxes,  # noqa: F401
                       encode_boxes, fastrcnn_loss, resize_boxes)
from .parallel import GradBucket, init_distributed  # noqa: F401
from .roi_align import MultiScaleRoIAlign, roi_align  # noqa: F401
from .graph import GraphedStep  # noqa: F401
from .rpn import AnchorGenerator, RegionProposalNetwork, RPNHead  # noqa: F401
from .roi_heads import RoIHeads, project_masks_on_boxes, select_training_samples  # noqa: F401
from .fpn import FeaturePyramidNetwork  # noqa: F401
from .body import BackboneWithFPN, FrozenBatchNorm2d, ResNetBody  # noqa: F401
from .transform import GeneralizedRCNNTransform, ImageList, MaskRCNN  # noqa: F401

__all__ = ['SlowFastLayers', 'PackedClip', 'SlowFastPlan', 'FusedSGD', 'GradBucket', 'init_distributed',
           'MSEProxyLoss', 'calc_kernel_sizes', 'calc_fuse_kernel_size', 'davis_pyramid', 'union_mask', 'SlowFastStream', 'SlowFastWindows', 'MaskBranch', 'MaskRCNNHeads', 'MaskRCNNPredictor',
           'maskrcnn_inference', 'maskrcnn_loss', 'paste_masks_in_image', 'MultiScaleRoIAlign', 'roi_align', 'GraphedStep', 'BoxBranch', 'TwoMLPHead', 'FastRCNNPredictor',
           'RoIHeadsInference', 'fastrcnn_loss', 'encode_boxes', 'decode_boxes', 'resize_boxes', 'AnchorGenerator', 'RPNHead',
           'RegionProposalNetwork', 'RoIHeads', 'select_training_samples', 'project_masks_on_boxes',
           'FeaturePyramidNetwork', 'ResNetBody', 'BackboneWithFPN', 'FrozenBatchNorm2d', 'GeneralizedRCNNTransform', 'ImageList',
           'MaskRCNN']
