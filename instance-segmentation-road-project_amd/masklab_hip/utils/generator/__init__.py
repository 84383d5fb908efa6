"""The reference's `engine.utils.generator`."""
from .masklab import MaskLabGenerator

__all__ = ["MaskLabGenerator"]
