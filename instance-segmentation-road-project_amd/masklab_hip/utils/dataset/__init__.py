"""The reference's `engine.utils.dataset`: the abstract `Dataset`, the file-reading `MaskLabDataset` (polygon labels drawn
on the device per batch, csrc/polygon.hip) and the label tables it is built from."""
from .dataset import Dataset
from .labels import load_labels
from .masklab import MaskLabDataset, get_image_cases

__all__ = ["Dataset", "MaskLabDataset", "get_image_cases", "load_labels"]
