"""The reference of GATv2 with a per-edge feature vector inside the LeakyReLU (dfgnn_gatv2_fwd_edge / dfgnn_gatv2_bwd_edge),
shared by tests/test_gpu_gatv2_edge.py and tests/test_gpu_guarded.py: a torch formulation with index ops over the edge list,
gradients from torch.autograd.grad, in float64 on the CPU."""
import torch

SLOPE = 0.2


def ref_conv(rows, cols, m, attn, x_row, x_col, e):
    """-> out, row_max, row_sum in the dtype of the inputs; differentiable.  x_col may have other rows than x_row."""
    z = x_row[rows] + x_col[cols] + e
    s = (torch.nn.functional.leaky_relu(z, SLOPE) * attn).sum(-1)                         # [nnz, h]
    mx = torch.full((m, s.size(1)), float("-inf"), dtype=s.dtype)
    mx = mx.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax", include_self=True)
    p = torch.exp(s - mx[rows])
    den = torch.zeros_like(mx).index_add_(0, rows, p)
    out = torch.zeros_like(x_row).index_add_(0, rows, x_col[cols] * (p / den[rows])[:, :, None])
    return out, mx, den


def ref_all(rows, cols, m, attn, x_row, x_col, e, dO, shared=False):
    """float64 CPU: out, row_max, row_sum and torch.autograd.grad's dX_row, dX_col, dattn, dE (shared: dX, dattn, dE)."""
    a = attn.double().requires_grad_(True)
    xr = x_row.double().requires_grad_(True)
    xc = xr if shared else x_col.double().requires_grad_(True)
    ee = e.double().requires_grad_(True)
    out, mx, den = ref_conv(rows, cols, m, a, xr, xc, ee)
    leaves = (xr, a, ee) if shared else (xr, xc, a, ee)
    grads = torch.autograd.grad(out, leaves, dO.double()) if len(rows) else [torch.zeros_like(t) for t in leaves]
    return dict(out=out.detach(), row_max=mx, row_sum=den.detach(), grads=[t.detach() for t in grads])
