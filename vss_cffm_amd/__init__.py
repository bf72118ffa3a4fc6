"""vss_cffm_amd -- MI355X-native (gfx950) implementation of the CFFM decode head's coarse-to-fine
cross-frame attention path (CFFA + CFM, and the CFFM++ prototype attention), behind the
reference's own module / registry names.  See DESIGN.md and include/cffm_hip.h."""
from .modules import (BasicLayer3d3, BasicLayer_cluster, CffmTransformerBlock3d3, Mlp,  # noqa: F401
                      SwinTransformerBlock_cluster, WindowAttention3d3, WindowAttention_cluster)
from .cluster import kmeans, kmeans_workspace  # noqa: F401,E402
from .ops import dwconv_gelu, ln_rows, ln_rows_nchw, mit_infer, mit_stage_infer, nchw_ln_rows, patch_embed, predict, sr_reduce, sra_attention  # noqa: F401,E402
from .ops import layer_norm_rows, layer_norm_rows_nchw, nchw_layer_norm_rows, overlap_patch_embed  # noqa: F401,E402
from .ops import linear_rows, linear_rows_supported  # noqa: F401,E402
from .ops import mit_blocks_train, mit_blocks_train_supported  # noqa: F401,E402
from . import head  # noqa: F401,E402  (registers the three CFFM heads and CrossEntropyLoss)
from .config import Config  # noqa: F401,E402
from . import optim  # noqa: F401,E402
from . import distributed  # noqa: F401,E402
from . import evaluation  # noqa: F401,E402
from . import segmentor  # noqa: F401,E402  (registers EncoderDecoder_clips)
from .stream import ClipStream  # noqa: F401,E402
from . import backbone  # noqa: F401,E402  (registers mit_b0 ... mit_b5)
from .registry import (BACKBONES, HEADS, LOSSES, NECKS, SEGMENTORS, Registry, build_backbone,  # noqa: F401,E402
                       build_from_cfg, build_head, build_loss, build_neck, build_segmentor)
from .checkpoint import load_reference_checkpoint  # noqa: F401,E402
from . import data  # noqa: F401,E402
