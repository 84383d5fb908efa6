"""The serving model of reference road_project/setup/serving.py:17-53: the bytes of an image file in,
[JPEG content of the rendered frame, summary] out.

    DecodeImageContent (baseline JPEG: Huffman decoding on the host, everything per pixel on the device; any other
    content: host, Pillow) -> deploy model -> DrawBoxes / DrawInstance / DrawSegmentation (one kernel)
    -> EncodeImageContent (baseline JPEG, encoded on the device) and SummaryOutput

The reference saves this graph as a TensorFlow SavedModel for its gRPC front end (save_serving_model, :56-72); here it
is a callable.  A baseline JPEG request needs no Pillow; entropy decoding on the device, 4:2:2 and progressive streams
are open."""
import numpy as np

from . import retinamasklab as R
from .config import ModelConfiguration
from .layers import DecodeImageContent


class ContentServingModel:
    """`predict(content)` / `__call__(content)`: content = `bytes` of one image file (or a length-1 sequence / array of
    them, the reference's string tensor of shape [1]) -> [NumPy object array [1] holding the JPEG `bytes` of the
    rendered frame, summary float32 [1,n,11]] -- the outputs 'visualize' and 'summarize' of the reference."""

    def __init__(self, configuration, deploy_model, device="cuda"):
        self.decode = DecodeImageContent(device=device)
        self.serving = R.ServingModel(configuration, deploy_model, visualize=True, encode=True)
        self.output_names = self.serving.output_names
        self.name = "serving"

    def predict(self, content):
        contents, summary = self.serving.predict(self.decode(content))
        out = np.empty((1,), dtype=object)
        out[0] = contents[0]
        return [out, summary]

    __call__ = predict


def load_serving_model_from_h5(weight_path, config: ModelConfiguration, device="cuda"):
    """Same name and arguments as the reference (:17): the checkpoint at `weight_path` (a Keras .h5, or the .npz
    tools/convert_keras_h5.py makes of it) -> the serving model."""
    deploy = R.load_masklab_inference_model_from_h5(weight_path, config, serving=False, device=device)
    return ContentServingModel(config, deploy, device=device)


__all__ = ["load_serving_model_from_h5", "ContentServingModel"]
