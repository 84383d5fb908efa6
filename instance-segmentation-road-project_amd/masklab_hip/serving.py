"""The serving model of reference road_project/setup/serving.py:17-53: the bytes of an image file in,
[JPEG content of the rendered frame, summary] out.

    DecodeImageContent (baseline JPEG: Huffman decoding on the host or, entropy="device", in kernels; everything per
    pixel on the device; any other content: host, Pillow) -> deploy model -> DrawBoxes / DrawInstance / DrawSegmentation (one kernel)
    -> EncodeImageContent (baseline JPEG, encoded on the device) and SummaryOutput

The reference saves this graph as a TensorFlow SavedModel for its gRPC front end (save_serving_model, :56-72); here it
is a callable.  A baseline JPEG request needs no Pillow; 4:2:2 and progressive streams are open."""
import numpy as np

from . import retinamasklab as R
from .config import ModelConfiguration
from .layers import DecodeImageContent


class ContentServingModel:
    """`predict(content)` / `__call__(content)`: content = `bytes` of one image file (or a length-1 sequence / array of
    them, the reference's string tensor of shape [1]) -> [NumPy object array [1] holding the JPEG `bytes` of the
    rendered frame, summary float32 [1,n,11]] -- the outputs 'visualize' and 'summarize' of the reference."""

    def __init__(self, configuration, deploy_model, device="cuda", entropy=None):
        self.decode = DecodeImageContent(device=device, entropy=entropy)
        self.serving = R.ServingModel(configuration, deploy_model, visualize=True, encode=True)
        self.output_names = self.serving.output_names
        self.name = "serving"

    @property
    def entropy(self):
        """Where a baseline JPEG request is Huffman-decoded: "host", "device" or None for ops.JPEG_ENTROPY_DEFAULT."""
        return self.decode.entropy

    @entropy.setter
    def entropy(self, entropy):
        self.decode = DecodeImageContent(device=self.decode.device, on_device=self.decode.on_device, entropy=entropy)

    def predict(self, content):
        contents, summary = self.serving.predict(self.decode(content))
        out = np.empty((1,), dtype=object)
        out[0] = contents[0]
        return [out, summary]

    __call__ = predict


def load_serving_model_from_h5(weight_path, config: ModelConfiguration, device="cuda"):
    """Same name and arguments as the reference (:17): the checkpoint at `weight_path` (a Keras .h5, or the .npz
    tools/convert_keras_h5.py makes of it) -> the serving model.  The signature is the reference's; where a baseline
    JPEG request is Huffman-decoded is the model's `entropy` attribute: `served.entropy = "device"`."""
    deploy = R.load_masklab_inference_model_from_h5(weight_path, config, serving=False, device=device)
    return ContentServingModel(config, deploy, device=device)


__all__ = ["load_serving_model_from_h5", "ContentServingModel"]
