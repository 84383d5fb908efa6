"""The reference's `engine.utils`: what feeds the trainer network -- the file-reading dataset (polygon labels drawn on the
device per batch) and the generator that scales its batches."""
from .dataset import Dataset, MaskLabDataset, get_image_cases
from .generator import MaskLabGenerator

__all__ = ["Dataset", "MaskLabDataset", "MaskLabGenerator", "get_image_cases"]
