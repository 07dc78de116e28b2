"""The reference of the AGNN / dot-product attention conv with tied keys and values (dfgnn_agnn_fwd / dfgnn_agnn_bwd), shared
by tests/test_gpu_agnn.py and tests/test_gpu_guarded.py: a torch formulation with index ops over the edge list, differentiable,
in the dtype of its inputs (the tests run it in float64 on the CPU and take the gradients from torch.autograd.grad)."""
import torch


def ref_conv(rows, cols, m, beta, x_row, x_col, cosine):
    """-> out, row_max, row_sum in the dtype of the inputs; differentiable."""
    norm = (lambda x: torch.nn.functional.normalize(x, p=2, dim=-1, eps=1e-12)) if cosine else (lambda x: x)
    s = (norm(x_row)[rows] * norm(x_col)[cols]).sum(-1) * beta                            # [E, h]
    mx = torch.full((m, s.size(1)), float("-inf"), dtype=s.dtype)
    mx = mx.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax", include_self=True)
    p = torch.exp(s - mx[rows])
    den = torch.zeros_like(mx).index_add_(0, rows, p)
    out = torch.zeros_like(x_row).index_add_(0, rows, x_col[cols] * (p / den[rows])[:, :, None])
    return out, mx, den
