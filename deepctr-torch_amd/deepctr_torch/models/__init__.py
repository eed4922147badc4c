"""Drop-in model classes of the MI355X hot path.  Constructor signatures
and ``state_dict`` keys are the reference's (``deepctr_torch/models/*.py``)."""
from .afm import AFM
from .afn import AFN
from .autoint import AutoInt
from .basemodel import BaseModel, Linear
from .ccpm import CCPM
from .dcn import DCN
from .dcnmix import DCNMix
from .deepfm import DeepFM
from .dien import DIEN
from .difm import DIFM
from .din import DIN
from .fibinet import FiBiNET
from .ifm import IFM
from .mlr import MLR
from .multitask import ESMM, MMOE, PLE, SharedBottom
from .nfm import NFM
from .onn import ONN
from .pnn import PNN
from .wdl import WDL
from .xdeepfm import xDeepFM

__all__ = ["BaseModel", "Linear", "DeepFM", "xDeepFM", "FiBiNET", "DCN", "PNN", "NFM", "AFM", "WDL", "AutoInt", "DCNMix",
           "IFM", "DIFM", "ONN", "CCPM", "DIN", "DIEN", "AFN", "MLR", "SharedBottom", "ESMM", "MMOE", "PLE"]
