"""kpx -- MI355X-native detector_translator hot path.

Importing the package loads libkpx_hip.so and fails loudly if it has not been built (no CPU / PyTorch fallback).
"""
from . import _lib  # noqa: F401  (raises ImportError when the HIP library is missing)
from . import layers, model_utils, networks, ops, summary, variables  # noqa: F401
from .base_model import BaseModel  # noqa: F401
from .detector_translator_model import DetectorTranslatorModel  # noqa: F401
from .keypoint_model import KeypointModel  # noqa: F401
from .final_model import FinalModel  # noqa: F401
from .motion_generator_model import MotionGeneratorModel  # noqa: F401
from .action_classifier_model import ActionClassifierModel  # noqa: F401
from .vgg import FeatureScorer, Vgg19, synthetic_vgg19_weights  # noqa: F401
from . import data  # noqa: F401
from . import resident  # noqa: F401
from . import frechet  # noqa: F401
from . import stability  # noqa: F401
from . import joints  # noqa: F401
from . import gif  # noqa: F401
from . import mjpeg  # noqa: F401
from . import stills  # noqa: F401
from . import novelty  # noqa: F401
from . import resample  # noqa: F401
from . import prdc  # noqa: F401
from .data import ImagePairDataLoader, KeypointDataLoader, SequenceDataLoader  # noqa: F401

__all__ = ['BaseModel', 'DetectorTranslatorModel', 'KeypointModel', 'FinalModel', 'MotionGeneratorModel', 'ActionClassifierModel', 'Vgg19', 'FeatureScorer', 'synthetic_vgg19_weights', 'ImagePairDataLoader', 'KeypointDataLoader', 'SequenceDataLoader', 'data', 'resident', 'frechet', 'stability', 'joints', 'layers', 'model_utils',
           'networks', 'ops', 'summary', 'variables']
