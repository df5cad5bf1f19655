from .utils import MODEL_REGISTRY
from .res_slimvit import Res_Slim_ViT
from .interpolation import Interpolation, Resampled
