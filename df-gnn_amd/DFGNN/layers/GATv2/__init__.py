from .gatv2conv_layers import (GATv2Conv_edge, GATv2Conv_edge_timing, GATv2Conv_forward, GATv2Conv_tiling,  # noqa: F401
                               GATv2ConvDGL)
