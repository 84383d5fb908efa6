"""masklab_hip -- MI355X-native (gfx950) implementation of the MaskLab inference hot path of
craftsangjae/instance-segmentation-road-project.  Python host code mirrors the reference's
`engine` package (same class / function names); all arithmetic runs in hand-written HIP kernels
behind the C ABI of include/masklab_hip.h.  PyTorch supplies device memory and streams only."""
from .config import ModelConfiguration
from .keras_like import clear_session
from .normalization import GroupNormalization
from .prior import PriorBoxes

__version__ = "0.1.0"


def get_custom_objects():
    """Name -> class registry, like the dict reference engine/__init__.py:17-73 fills."""
    from . import layers as L
    from .backbone import BackBonePreProcess
    names = ["RestoreBoxes", "PriorLayer", "Identity", "FeaturePyramid", "ClassificationSubNet",
             "BoxRegressionSubNet", "MaskSubNet", "NormalizeBoxes", "DetectionProposal", "MoldBatch",
             "MaskDistribute", "PyramidRoiAlign", "ResizeLike", "AtrousSeparableConv2D", "ASPPNetwork",
             "SegmentationSubNet", "SqueezeExcite", "MobileSeparableConv2D", "DownSampleInput", "UpSampleOutput",
             "TrimInstances", "SemanticSmoothing", "CropAndPadMask", "CrackToInstance", "SummaryOutput",
             "IncludeMyRoad", "CalculateInstanceSize", "DrawSegmentation", "DrawInstance", "DrawBoxes", "EncodeImageContent",
             "DecodeImageContent", "CalculateIOU", "AssignBoxes", "AssignMasks", "AssignSeg"]
    reg = {n: getattr(L, n) for n in names}
    reg["BackBonePreProcess"] = BackBonePreProcess
    reg["GroupNormalization"] = GroupNormalization
    from . import metrics
    reg.update({n: getattr(metrics, n) for n in metrics.__all__})
    from . import losses
    reg.update({n: getattr(losses, n) for n in losses.__all__})
    from . import optimizers
    reg.update({n: getattr(optimizers, n) for n in optimizers.__all__})
    return reg
