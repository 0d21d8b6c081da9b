"""TEST INFRASTRUCTURE — plain-torch (CPU, fp32 or fp64) restatements of the attention weights ``glam_amd.explain`` exports,
"reference-shaped" like ``oracle/glam_oracle.py``: materialised gathers, the concatenated triplet of src_1gp/layer.py:48-51, scatter
based segment softmax.  Every function works in the dtype of its float arguments."""
import torch
import torch.nn.functional as F

import oracle.glam_oracle as O


def separable_alpha(a_ij, edge_attr, M, edge_index, N, heads, slope=0.2):
    """The kernel's contract: ``leaky(a_ij[dst, h] + <edge_attr, M[:, h]> + a_ij[src, 4 + h])`` soft-maxed over the edges into ``dst``."""
    src, dst = edge_index[0], edge_index[1]
    logit = a_ij[dst, :heads] + edge_attr @ M[:, :heads] + a_ij[src, 4:4 + heads]
    return O.segment_softmax(F.leaky_relu(logit, slope), dst, N)


def triplet_alpha(x, edge_index, edge_attr, weight_node, weight_edge, att, heads, slope=0.2):
    """``TripletMessage``: ``(alpha[E, H], e_ij[E, H, C], x_j[E, H, C])`` in the concatenated form (src_1gp/layer.py:37-51)."""
    N, C = x.shape
    src, dst = edge_index[0], edge_index[1]
    xw = torch.matmul(x, weight_node)                                   # layer.py:37
    e_ij = torch.matmul(edge_attr, weight_edge).view(-1, heads, C)      # layer.py:38, :46
    x_j, x_i = xw[src].view(-1, heads, C), xw[dst].view(-1, heads, C)
    triplet = torch.cat([x_i, e_ij, x_j], dim=-1)                       # layer.py:48
    alpha = F.leaky_relu((triplet * att).sum(dim=-1), slope)            # layer.py:49-50
    return O.segment_softmax(alpha, dst, N), e_ij, x_j                  # layer.py:51


def triplet_out_from_alpha(alpha, e_ij, x_j, edge_index, N, weight_scale, bias):
    """The layer's output rebuilt from a given alpha: messages ``alpha * e_ij * x_j`` (layer.py:55), add-aggregate, ``update`` (:57-61)."""
    aggr = O.scatter(alpha.unsqueeze(-1) * e_ij * x_j, edge_index[1], N, "sum")
    return torch.matmul(aggr.reshape(N, weight_scale.size(0)), weight_scale) + bias


def light_alpha(x, edge_index, edge_attr, weight_node, att, slope=0.2):
    """``TripletMessageLight``: ``(alpha[E, 1], x_j[E, C])`` (src_1gp/layer.py:84-95)."""
    src, dst = edge_index[0], edge_index[1]
    xw = torch.matmul(x, weight_node)
    triplet = torch.cat([xw[dst], edge_attr, xw[src]], dim=-1)          # layer.py:92
    alpha = F.leaky_relu((triplet * att).sum(dim=-1), slope)
    return O.segment_softmax(alpha.view(-1, 1), dst, x.size(0)), xw[src]


def gat_alpha(x, edge_index, lin_weight, att_l, att_r, slope=0.2):
    """PyG ``GATConv(heads=1, return_attention_weights=True)``: ``(edge_index with self loops, alpha[E', 1], x_l[src])``."""
    N = x.size(0)
    ei = O._with_self_loops(edge_index, N)
    src, dst = ei[0], ei[1]
    xl = F.linear(x, lin_weight)
    al, ar = (xl * att_l.view(1, -1)).sum(-1), (xl * att_r.view(1, -1)).sum(-1)
    alpha = F.leaky_relu(al[src] + ar[dst], slope)
    return ei, O.segment_softmax(alpha.view(-1, 1), dst, N), xl[src]


def set2set_weights(x, batch, num_graphs, lstm, steps):
    """PyG ``Set2Set``: ``(a[steps, N], q_star[B, 2C])`` — ``O.set2set`` with the per-step attention kept."""
    C = x.size(1)
    h = (x.new_zeros(1, num_graphs, C), x.new_zeros(1, num_graphs, C))
    q_star = x.new_zeros(num_graphs, 2 * C)
    ws = []
    for _ in range(steps):
        q, h = lstm(q_star.unsqueeze(0), h)
        q = q.view(num_graphs, C)
        a = O.segment_softmax((x * q[batch]).sum(dim=-1, keepdim=True), batch, num_graphs)
        ws.append(a.view(-1))
        q_star = torch.cat([q, O.scatter(a * x, batch, num_graphs, "sum")], dim=-1)
    return torch.stack(ws), q_star
