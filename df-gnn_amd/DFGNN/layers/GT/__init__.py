from .gtconv_layer import SparseMHA  # noqa: F401
from .gtconv_layer_bias import SparseMHA_bias, SparseMHA_bias_timing  # noqa: F401
from .gtconv_layer_edge import SparseMHA_edge, SparseMHA_edge_timing  # noqa: F401
from .gtconv_layer_gate import SparseMHA_gate, SparseMHA_gate_timing  # noqa: F401
from .gtconv_layer_typed import SparseMHA_typed, SparseMHA_typed_timing, preprocess_types  # noqa: F401
from .gtconv_layer_tbias import SparseMHA_tbias, SparseMHA_tbias_timing  # noqa: F401
from .gtconv_layer_csr_gm import SparseMHA_CSR_GM  # noqa: F401
from .gtconv_layer_forward import SparseMHA_forward, SparseMHA_forward_timing  # noqa: F401
from .gtconv_layer_fused import SparseMHA_CSR, SparseMHA_hyper, SparseMHA_softmax  # noqa: F401
from .gtconv_layer_rowstats import SparseMHA_rowstats, SparseMHA_rowstats_timing  # noqa: F401
from .gtconv_layer_softmax_gm import SparseMHA_softmax_gm  # noqa: F401
from .gtconv_layer_tiling import SparseMHA_tiling  # noqa: F401
