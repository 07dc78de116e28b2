from .gatv2conv_layers import GATv2Conv_forward, GATv2Conv_tiling, GATv2ConvDGL  # noqa: F401
