"""autograd.Function wrappers over the C-ABI (include/dctr.h), one module per kernel family; tensors become C arguments
in ``_hip/marshal.py``.  This package only re-exports what the layers, models, tests and tools use."""
from ..marshal import ptr as _ptr  # noqa: F401
from .attention import (DIN_ACT, DINAttentionFunction, GRU_MODE, GRUSeqFunction, InteractFunction,  # noqa: F401
                        din_attention_supported, gru_seq_supported, interacting_supported)
from .ccpm import CCPMConvFunction  # noqa: F401
from .cin import CINLayerFunction, CINStackFunction, cin_layer_forward  # noqa: F401
from .cross import CrossNetMatFunction, CrossNetMixFunction, CrossNetVecFunction  # noqa: F401
from .embed import (EmbedFunction, PairEmbedFunction, SplitGatheredFunction, embed, gather_columns,  # noqa: F401
                    pair_embed, split_gathered)
from .fm import AFMFunction, BiPoolFunction, FMFunction, IAFMFunction, iafm, iafm_supported  # noqa: F401
from .gate_mix import GateMixFunction, gate_mix, gate_mix_fused, gate_mix_torch  # noqa: F401
from .log_transform import LogTransformFunction  # noqa: F401
from .mlr import MLRFunction, MLRHeads, mlr, mlr_composed, mlr_route  # noqa: F401
from .pairwise import (BilinearFunction, BilinearMeta, BilinearStackedFunction, InnerProductFunction,  # noqa: F401
                       SENETFunction, disjoint_groups, slab_ld, tournament_schedule)
