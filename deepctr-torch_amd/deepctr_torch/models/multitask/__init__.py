"""The multi-task models of the reference (``deepctr_torch/models/multitask``): several prediction heads over shared
bottoms, experts and gates.  The output is ``[B, num_tasks]``, ``compile`` takes one loss per task."""
from .esmm import ESMM
from .mmoe import MMOE
from .ple import PLE
from .sharedbottom import SharedBottom

__all__ = ["SharedBottom", "ESMM", "MMOE", "PLE"]
