"""Layer registry of the hot path (mirrors reference engine/layers/__init__.py:5-8)."""
from .detection import *  # noqa: F401,F403
from .detection import (AssignBoxes, BoxRegressionSubNet, CalculateIOU, ClassificationSubNet, DetectionProposal, FeaturePyramid,
                        NormalizeBoxes, PriorLayer, RestoreBoxes)
from .instance import AssignMasks, MaskDistribute, MaskSubNet, PyramidRoiAlign, TrimInstances
from .misc import (CalculateInstanceSize, CrackToInstance, CropAndPadMask, DecodeImageContent, DownSampleInput, DrawBoxes,
                   DrawInstance, DrawSegmentation, EncodeImageContent, Identity, IncludeMyRoad, MobileSeparableConv2D,
                   MoldBatch, ReLU, ResizeLike, SqueezeExcite, SummaryOutput, UpSampleOutput)
from .semantic import ASPPNetwork, AssignSeg, AtrousSeparableConv2D, SegmentationSubNet, SemanticSmoothing
