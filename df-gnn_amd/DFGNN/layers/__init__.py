from .AGNN import AGNNConv_beta, AGNNConv_forward  # noqa: F401
from .GAT import GATConv_edge, GATConv_forward, index_ops_gat_edge  # noqa: F401
from .GAT_DOT import DOTGATConv_forward  # noqa: F401
from .GatedGCN import GatedGCNConv, index_ops_gatedgcn  # noqa: F401
from .GATv2 import GATv2Conv_edge, GATv2Conv_forward, GATv2Conv_tiling, GATv2ConvDGL  # noqa: F401
from .GT.gtconv_layer_bias import SparseMHA_bias  # noqa: F401
from .GT.gtconv_layer_edge import SparseMHA_edge  # noqa: F401
from .GT.gtconv_layer_gate import SparseMHA_gate  # noqa: F401
from .GT.gtconv_layer_typed import SparseMHA_typed, preprocess_types  # noqa: F401
from .GT.gtconv_layer_tbias import SparseMHA_tbias  # noqa: F401
from .GT.gtconv_layer_forward import SparseMHA_forward  # noqa: F401
from .GT.gtconv_layer_rowstats import SparseMHA_rowstats  # noqa: F401
from .model import Model, choose_Inproj  # noqa: F401
from .util import (load_graphconv_layer, load_layer_AGNN, load_layer_DOTGAT, load_layer_GAT, load_layer_GATv2, load_layer_GatedGCN, load_layer_GT, load_prepfunc,  # noqa: F401
                   preprocess_block, preprocess_CSR, preprocess_Hyper, preprocess_Hyper_fw_bw, preprocess_softmax)
