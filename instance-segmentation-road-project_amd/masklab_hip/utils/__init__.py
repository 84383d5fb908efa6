"""The reference's `engine.utils`: what feeds the trainer network (the dataset's file reading is out of scope)."""
from .generator import MaskLabGenerator

__all__ = ["MaskLabGenerator"]
