"""Layer zoo of the hot path.  ★ interaction layers call hand-written gfx950 kernels through
``deepctr_torch._hip``; the MLP tower / activations are the boundary and stay ordinary PyTorch-ROCm
modules."""
from .activation import Dice, Identity, activation_layer
from .core import DNN, Conv2dSame, LocalActivationUnit, PredictionLayer
from .interaction import *  # noqa: F401,F403
from .sequence import (AGRUCell, AttentionSequencePoolingLayer, AUGRUCell, DynamicGRU, KMaxPooling,
                       SequencePoolingLayer)
from .utils import concat_fun, slice_arrays
