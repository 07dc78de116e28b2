from .gatedgcn_layers import (GatedGCNConv, GatedGCNConv_plain_timing, GatedGCNConv_timing,  # noqa: F401
                              index_ops_gatedgcn)
